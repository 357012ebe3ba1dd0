#!/usr/bin/env python3
"""afx_harmonic_ratio.hip as emulated device code through the C host object harmonicRatioObj: the smallest case of each class
(tests/harmonic_ratio_cases.py: SMALL) by the rule of the GPU tests (tests/harmonic_ratio_check.py) -- values through
harmonicRatio() and harmonicRatioBatchDevice with lag and first, the curve through curveBatchDevice --, a strided batch
bitwise equal to single calls with no inherited minIndex crossing a clip boundary, a call split in two, refusals.
AFX_LIB = the library tests/test_harmonic_ratio_emulated.py builds.  Arguments: case names (default: SMALL) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import harmonic_ratio_cases as hc  # noqa: E402
from tests import harmonic_ratio_restate as hr  # noqa: E402
from tests.harmonic_ratio_check import check_case  # noqa: E402

lib = hc.bind_device(C.CDLL(os.environ["AFX_LIB"]))


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fixture_case(name, gold):
    c = hc.CASES[name]
    r, hop = c[2], c[3]
    x = hc.case_input(name)
    st, p = hc.plan(lib, *hc.ctor_args(name))
    assert st == 0, (name, st)
    N, L, slide, mx = (int(v) for v in gold[name + "/plan"])
    assert (p["windowLength"], p["fftLength"], p["slideLength"], p["maxLength"]) == (N, L, slide, mx), name
    st, obj = hc.new(lib, *hc.ctor_args(name))
    assert st == 0 and obj, (name, st)
    assert (lib.harmonicRatioObj_maxLength(obj), lib.harmonicRatioObj_windowLength(obj)) == (mx, N)
    value = hc.call(lib, obj, x)
    T = len(value)
    dval = np.full(T + 2, 7.0, np.float32)
    dlag, dfirst = np.full(T + 2, 77, np.int32), np.full(T + 2, 77, np.int32)
    assert lib.harmonicRatioObj_harmonicRatioBatchDevice(obj, P(x), 1, len(x), len(x), P(dval), P(dlag), P(dfirst), T + 2, None) == 0
    curve = np.full((T, mx), 9.0, np.float32)
    assert lib.harmonicRatioObj_curveBatchDevice(obj, P(x), 1, len(x), len(x), P(curve), None) == 0
    only = np.full(T, 7.0, np.float32)  # the optional outputs NULL
    assert lib.harmonicRatioObj_harmonicRatioBatchDevice(obj, P(x), 1, len(x), len(x), P(only), None, None, T, None) == 0
    lib.harmonicRatioObj_free(obj)
    assert same_bits(dval[:T], value) and same_bits(only, value), name
    assert (dval[T:] == 7).all() and (dlag[T:] == 77).all() and (dfirst[T:] == 77).all(), name
    frames = hr.harmonic_ratio(x, p["window"], r, hop, mx)
    w = check_case(name, frames, gold[name + "/eps"], value, mx, dlag[:T], dfirst[:T], curve, hc.cap(name))
    consistent(name, value, dlag[:T], dfirst[:T], curve, mx)
    print(f"harmonic_ratio {name}: window {N}, hop {hop}, {T} frames: curve {w['worst_curve']:.3f}, value {w['worst_value']:.3f} "
          f"of their bars, explained {w['explained']}, first {dfirst[:T].tolist()}", flush=True)


def consistent(name, value, lag, first, curve, mx):
    """dValue against the exported curve and dLag: zeros at and below first, the first maximum above it, the value the entry
    itself at the ends of the range and the reference's parabola through the three entries elsewhere"""
    for t in range(len(value)):
        f, row = int(first[t]), curve[t]
        assert not row[:f + 1].any(), (name, t)
        if f + 1 >= mx:
            assert lag[t] == -1 and value[t] == 0, (name, t)
            continue
        j = f + 1 + int(np.argmax(row[f + 1:]))  # numpy's argmax is the first maximum
        assert lag[t] == j, (name, t, lag[t], j)
        if j in (f + 1, mx - 1):
            assert same_bits(value[t:t + 1], row[j:j + 1]), (name, t)
        else:
            v1, v2, v3 = (np.float32(v) for v in row[j - 1:j + 2])
            p = np.float32(np.float64(v3 - v1) / (np.float64(np.float32(2) * (np.float32(2) * v2 - v3 - v1)) + 1e-16))
            want = np.float32(np.float64(v2) - 0.25 * np.float64(v1 - v3) * np.float64(p))
            assert same_bits(value[t:t + 1], np.array([want])), (name, t, value[t], want)


def extras():
    # three clips, dc behind noise: bitwise the single calls, nothing beyond a row's frames, no minIndex leaks into dc
    names = ("carry_r8", "noise_r8", "dc_r8")
    xs = [hc.case_input(n)[:256 + 64 * 5 + 5] for n in names]
    n, clips, stride = len(xs[0]), 3, len(xs[0]) + 12
    buf = np.zeros(clips * stride + 1, np.float32)
    rows = buf[1:].reshape(clips, stride)
    for c in range(clips):
        rows[c, :n] = xs[c]
    st, obj = hc.new(lib, 16000, 1000.0, 8, None, 64)
    assert st == 0
    T = lib.harmonicRatioObj_calTimeLength(obj, n)
    single = [hc.call(lib, obj, x) for x in xs]
    v = np.full((clips + 1, T + 2), np.nan, np.float32)
    lag, first = np.full((clips + 1, T + 2), 77, np.int32), np.full((clips + 1, T + 2), 77, np.int32)
    assert lib.harmonicRatioObj_harmonicRatioBatchDevice(obj, P(rows), clips, n, stride, P(v), P(lag), P(first), T + 2, None) == 0
    for c in range(clips):
        assert same_bits(v[c, :T], single[c]), c
    assert np.isnan(v[:clips, T:]).all() and np.isnan(v[clips]).all() and (lag[:clips, T:] == 77).all() and (first[clips] == 77).all()
    assert first[1, :T].any() and not first[2, :T].any(), first
    f = lib.harmonicRatioObj_harmonicRatioBatchDevice
    assert f(obj, P(rows), clips, n, stride, None, None, None, T, None) == -6
    assert f(obj, P(rows), clips, n, stride, P(v), None, None, T - 1, None) == -6
    assert f(obj, P(rows), clips, n, n - 1, P(v), None, None, T, None) == -6
    assert f(obj, P(rows), 0, n, stride, P(v), None, None, T, None) == -6
    assert f(obj, None, clips, n, stride, P(v), None, None, T, None) == -6
    g = np.full(4, 3.0, np.float32)
    assert f(obj, P(rows), 1, 100, stride, P(g), None, None, 4, None) == 0 and (g == 3).all()
    # carry_r8 in one call and split at a frame boundary: the second call starts from minIndex 0 again
    x = hc.case_input("carry_r8")
    whole = hc.call(lib, obj, x)
    a, b = hc.call(lib, obj, x[:256 + 64 * 4]), hc.call(lib, obj, x[64 * 5:])
    assert len(a) + len(b) == len(whole) == 10 and same_bits(a, whole[:5])
    assert not same_bits(b, whole[5:])  # frames 5 ... inherit 2 in one call, 0 after the split
    lib.harmonicRatioObj_free(obj)
    print("harmonic_ratio: a batch of 3 strided clips bitwise the single calls, dc behind noise keeps minIndex 0; a split call "
          "restarts from 0; refusals", flush=True)


def main(argv):
    gold = np.load(os.path.join(hc.GOLDEN, "harmonic_ratio.npz"))
    for name in [a for a in argv if a != "extras"] or (list(hc.SMALL) if not argv else []):
        fixture_case(name, gold)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
