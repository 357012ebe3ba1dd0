#!/usr/bin/env python3
"""afx_pitch_hs.hip as emulated device code through the C host object: the smallest case of each D = M / fftLength class and
of both placements of the spectrum slice (tests/pitch_hs_cases.py: SMALL), both kinds, by the rule of the GPU tests
(tests/pitch_hs_check.py) -- fre through pitch() and pitchBatchDevice, the curve through curveBatchDevice --, a strided
batch bitwise equal to single calls, streaming in pieces == one call, refusals.
AFX_LIB = the library tests/test_pitch_hs_emulated.py builds.  Arguments: case names (default: SMALL) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import pitch_hs_cases as hc  # noqa: E402
from tests import pitch_hs_restate as hr  # noqa: E402
from tests.pitch_cases import signal  # noqa: E402
from tests.pitch_hs_check import check_case  # noqa: E402

lib = hc.bind_device(C.CDLL(os.environ["AFX_LIB"]))


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fn(kind, what):
    return getattr(lib, f"pitch{hc.KIND_NAME[kind]}Obj_{what}")


def fixture_case(name, kind, gold):
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
    x = hc.case_input(name)
    M, mn, mx, cnt, wt = hc.plan(kind, sr, lo, hi, r, hop, window, count)
    st, obj = hc.new(lib, kind, sr, lo, hi, r, hop, window, count)
    assert st == 0 and obj, (name, st)
    assert (fn(kind, "interpLength")(obj), fn(kind, "minIndex")(obj), fn(kind, "maxIndex")(obj), fn(kind, "harmonicCount")(obj)) == \
        (M, mn, mx, cnt), name
    fre = hc.call(lib, kind, obj, x)
    T = len(fre)
    dfre, dval = np.full(T + 2, 7.0, np.float32), np.full(T + 2, 7.0, np.float32)
    assert fn(kind, "pitchBatchDevice")(obj, P(x), 1, len(x), len(x), P(dfre), P(dval), T + 2, None) == 0
    curve = np.full((T, mx + 1), np.nan, np.float32)
    assert fn(kind, "curveBatchDevice")(obj, P(x), 1, len(x), len(x), P(curve), None) == 0
    hc.free(lib, kind, obj)
    assert same_bits(dfre[:T], fre) and (dfre[T:] == 7).all() and (dval[T:] == 7).all(), name
    key = f"{name}/{hc.KIND_NAME[kind]}"
    frames = hr.pitch(kind, x, sr, r, hop, wt, M, mn, mx, cnt)
    w = check_case(key, frames, gold[key + "/eps"], gold[key + "/fre"], fre, sr, M, curve)
    for t in range(T):  # the value is the curve's entry at the chosen index, bit for bit
        i = int(round(float(fre[t]) / (1.0 * sr / M))) - 1
        assert same_bits(dval[t:t + 1], curve[t, i:i + 1]), (key, t, i)
    print(f"pitch_hs {key}: n_fft {1 << r}, M {M}, hop {hop}, {T} frames: curve {w['worst_curve']:.2f} of its bar, "
          f"explained {w['explained']}", flush=True)


def extras():
    for kind in (hc.HPS, hc.LHS):
        # a strided batch from a misaligned base: bitwise the single calls, nothing written beyond a row's frames
        sr, r, hop = 16000, 9, 128
        n, clips, stride = 512 + 128 * 5 + 5, 3, 512 + 128 * 5 + 17
        buf = np.zeros(clips * stride + 1, np.float32)
        xs = buf[1:].reshape(clips, stride)
        for c, sig in enumerate(("tone:330", "stack:196", "glide")):
            xs[c, :n] = signal(sig, n, sr, seed=70 + c)
        st, obj = hc.new(lib, kind, sr, 40.0, 2000.0, r, hop, hc.HANN, 4)
        assert st == 0
        T = hc.cal_time_length(lib, kind, obj, n)
        single = [hc.call(lib, kind, obj, xs[c, :n]) for c in range(clips)]
        f, v = np.full((clips + 1, T + 2), np.nan, np.float32), np.full((clips + 1, T + 2), np.nan, np.float32)
        assert fn(kind, "pitchBatchDevice")(obj, P(xs), clips, n, stride, P(f), P(v), T + 2, None) == 0
        for c in range(clips):
            assert same_bits(f[c, :T], single[c]), (kind, c)
        assert np.isnan(f[:clips, T:]).all() and np.isnan(f[clips]).all() and np.isnan(v[:clips, T:]).all() and np.isnan(v[clips]).all()
        assert not np.isnan(v[:clips, :T]).any()
        assert fn(kind, "pitchBatchDevice")(obj, P(xs), clips, n, stride, None, None, T, None) == -6
        assert fn(kind, "pitchBatchDevice")(obj, P(xs), clips, n, stride, P(f), None, T - 1, None) == -6
        assert fn(kind, "pitchBatchDevice")(obj, P(xs), clips, n, n - 1, P(f), None, T, None) == -6
        assert fn(kind, "pitchBatchDevice")(obj, P(xs), 0, n, stride, P(f), None, T, None) == -6
        g = np.full(4, 3.0, np.float32)
        assert fn(kind, "pitchBatchDevice")(obj, P(xs), 1, 100, stride, P(g), None, 4, None) == 0 and (g == 3).all()
        hc.free(lib, kind, obj)
        # streaming: three uneven pieces and random pieces == one call, hop below and above the frame length
        rng = np.random.default_rng(12)
        for r, hop in ((8, 64), (8, 100), (8, 300), (8, 700)):
            N = 1 << r
            x = signal("glide", N + hop * 9 + 31, sr, seed=90)
            st, one = hc.new(lib, kind, sr, 60.0, 2000.0, r, hop, hc.HAMM, 3)
            whole = hc.call(lib, kind, one, x)
            hc.free(lib, kind, one)
            for cuts in ([len(x) // 5, len(x) // 5 + 2 * N + 3], sorted(rng.integers(1, len(x), 6).tolist())):
                st, obj = hc.new(lib, kind, sr, 60.0, 2000.0, r, hop, hc.HAMM, 3, cont=1)
                assert st == 0
                parts = [hc.call(lib, kind, obj, p) for p in np.split(x, cuts) if len(p)]
                assert fn(kind, "pitchBatchDevice")(obj, P(x), 1, len(x), len(x), P(f), None, 1000, None) == -4
                hc.free(lib, kind, obj)
                got = np.concatenate(parts)
                assert same_bits(got, whole), (kind, r, hop, len(got), len(whole))
    print("pitch_hs batches of 3 strided clips bitwise the single calls; streaming in pieces == one call at hops 64 / 100 / 300 / 700 "
          "of 256; refusals", flush=True)


def main(argv):
    gold = np.load(os.path.join(hc.GOLDEN, "pitch_hs.npz"))
    names = [a for a in argv if a != "extras"] or (list(hc.SMALL) if not argv else [])
    for name in names:
        for kind in hc.CASES[name][0]:
            fixture_case(name, kind, gold)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
