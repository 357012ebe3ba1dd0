#!/usr/bin/env python3
"""afx_pitch_pef.hip as emulated device code through the C host object: the smallest case of each class
(tests/pitch_pef_cases.py: SMALL) by the rule of the GPU tests (tests/pitch_pef_check.py) -- fre through pitch() and
pitchBatchDevice, the curve through curveBatchDevice --, a strided batch bitwise equal to single calls, streaming in
pieces == one call, refusals.
AFX_LIB = the library tests/test_pitch_pef_emulated.py builds.  Arguments: case names (default: SMALL) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import pitch_pef_cases as pc  # noqa: E402
from tests import pitch_pef_restate as pr  # noqa: E402
from tests.pitch_cases import signal  # noqa: E402
from tests.pitch_pef_check import check_case  # noqa: E402

lib = pc.bind_device(C.CDLL(os.environ["AFX_LIB"]))


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fixture_case(name, gold):
    c = pc.CASES[name]
    sr, r, hop = c[0], c[4], c[5]
    x = pc.case_input(name)
    st, tables = pc.plan(lib, *pc.ctor_args(name))
    assert st == 0, (name, st)
    tables["lin"] = pc.lin_table(sr, 1 << r)
    mn, mx, pad = (int(v) for v in gold[name + "/plan"])
    st, obj = pc.new(lib, *pc.ctor_args(name))
    assert st == 0 and obj, (name, st)
    assert (lib.pitchPEFObj_minIndex(obj), lib.pitchPEFObj_maxIndex(obj), lib.pitchPEFObj_filterPadNum(obj),
            lib.pitchPEFObj_logLength(obj)) == (mn, mx, pad, 2 << r), name
    fre = pc.call(lib, obj, x)
    T = len(fre)
    dfre, dval = np.full(T + 2, 7.0, np.float32), np.full(T + 2, 7.0, np.float32)
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(x), 1, len(x), len(x), P(dfre), P(dval), T + 2, None) == 0
    curve = np.full((T, mx + 1), np.nan, np.float32)
    assert lib.pitchPEFObj_curveBatchDevice(obj, P(x), 1, len(x), len(x), P(curve), None) == 0
    lib.pitchPEFObj_free(obj)
    assert same_bits(dfre[:T], fre) and (dfre[T:] == 7).all() and (dval[T:] == 7).all(), name
    frames = pr.pitch(x, tables, r, hop, pad, mn, mx)
    w = check_case(name, frames, gold[name + "/eps"], gold[name + "/fre"], fre, tables["lg"], mn, curve)
    lgbits = tables["lg"].view(np.uint32)
    for t in range(T):  # the value is the curve's entry at the chosen index, bit for bit
        i = mn + int(np.flatnonzero(lgbits[mn:] == fre[t:t + 1].view(np.uint32)[0])[0])
        assert same_bits(dval[t:t + 1], curve[t, i:i + 1]), (name, t, i)
    print(f"pitch_pef {name}: n_fft {1 << r}, hop {hop}, P {pad}, {T} frames: curve {w['worst_curve']:.3f} of its bar, "
          f"explained {w['explained']}", flush=True)


def extras():
    # a strided batch from a misaligned base: bitwise the single calls, nothing written beyond a row's frames
    sr, r, hop = 16000, 9, 128
    n, clips, stride = 512 + 128 * 5 + 5, 3, 512 + 128 * 5 + 17
    buf = np.zeros(clips * stride + 1, np.float32)
    xs = buf[1:].reshape(clips, stride)
    for c, sig in enumerate(("tone:330", "stack:196", "glide")):
        xs[c, :n] = signal(sig, n, sr, seed=70 + c)
    st, obj = pc.new(lib, sr, 40.0, 2000.0, None, r, hop, pc.HANN)
    assert st == 0
    T = lib.pitchPEFObj_calTimeLength(obj, n)
    single = [pc.call(lib, obj, xs[c, :n]) for c in range(clips)]
    f, v = np.full((clips + 1, T + 2), np.nan, np.float32), np.full((clips + 1, T + 2), np.nan, np.float32)
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(xs), clips, n, stride, P(f), P(v), T + 2, None) == 0
    for c in range(clips):
        assert same_bits(f[c, :T], single[c]), c
    assert np.isnan(f[:clips, T:]).all() and np.isnan(f[clips]).all() and np.isnan(v[:clips, T:]).all() and np.isnan(v[clips]).all()
    assert not np.isnan(v[:clips, :T]).any()
    # setFilterParams: validated, then no change
    lib.pitchPEFObj_setFilterParams(obj, 5.0, 0.7, 2.5)
    lib.pitchPEFObj_setFilterParams(obj, -1.0, 0.7, 2.5)
    assert same_bits(pc.call(lib, obj, xs[0, :n]), single[0])
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(xs), clips, n, stride, None, None, T, None) == -6
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(xs), clips, n, stride, P(f), None, T - 1, None) == -6
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(xs), clips, n, n - 1, P(f), None, T, None) == -6
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(xs), 0, n, stride, P(f), None, T, None) == -6
    g = np.full(4, 3.0, np.float32)
    assert lib.pitchPEFObj_pitchBatchDevice(obj, P(xs), 1, 100, stride, P(g), None, 4, None) == 0 and (g == 3).all()
    lib.pitchPEFObj_free(obj)
    # streaming: three uneven pieces and random pieces == one call, hop below and above the frame length
    rng = np.random.default_rng(12)
    for r, hop in ((8, 64), (8, 100), (8, 300), (8, 700)):
        N = 1 << r
        x = signal("glide", N + hop * 9 + 31, sr, seed=90)
        st, one = pc.new(lib, sr, 60.0, 2000.0, None, r, hop)
        whole = pc.call(lib, one, x)
        lib.pitchPEFObj_free(one)
        for cuts in ([len(x) // 5, len(x) // 5 + 2 * N + 3], sorted(rng.integers(1, len(x), 6).tolist())):
            st, obj = pc.new(lib, sr, 60.0, 2000.0, None, r, hop, cont=1)
            assert st == 0
            parts = [pc.call(lib, obj, p) for p in np.split(x, cuts) if len(p)]
            assert lib.pitchPEFObj_pitchBatchDevice(obj, P(x), 1, len(x), len(x), P(f), None, 1000, None) == -4
            lib.pitchPEFObj_free(obj)
            got = np.concatenate(parts)
            assert same_bits(got, whole), (r, hop, len(got), len(whole))
    print("pitch_pef batches of 3 strided clips bitwise the single calls; streaming in pieces == one call at hops 64 / 100 / 300 / "
          "700 of 256; set_filter_params changes nothing; refusals", flush=True)


def main(argv):
    gold = np.load(os.path.join(pc.GOLDEN, "pitch_pef.npz"))
    names = [a for a in argv if a != "extras"] or (list(pc.SMALL) if not argv else [])
    for name in names:
        fixture_case(name, gold)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
