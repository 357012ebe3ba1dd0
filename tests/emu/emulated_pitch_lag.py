#!/usr/bin/env python3
"""afx_pitch_lag.hip as emulated device code through the C host objects pitchNCFObj / pitchCEPObj: the smallest case of
each class (tests/pitch_lag_cases.py: SMALL) by the rule of the GPU tests (tests/pitch_lag_check.py) -- fre through pitch()
and pitchBatchDevice, the curve through curveBatchDevice --, a strided batch bitwise equal to single calls, streaming in
pieces == one call, refusals.
AFX_LIB = the library tests/test_pitch_lag_emulated.py builds.  Arguments: case names (default: SMALL) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import pitch_lag_cases as pc  # noqa: E402
from tests import pitch_lag_restate as pr  # noqa: E402
from tests.pitch_cases import signal  # noqa: E402
from tests.pitch_lag_check import check_case, index_of  # noqa: E402

lib = pc.bind_device(C.CDLL(os.environ["AFX_LIB"]))


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fixture_case(kind, name, gold):
    c = pc.CASES[name]
    sr, r, hop = c[0], c[3], c[4]
    x = pc.case_input(name)
    st, p = pc.plan(lib, kind, *pc.ctor_args(name))
    assert st == 0, (kind, name, st)
    mn, mx = (int(v) for v in gold[f"{kind}/{name}/plan"])
    st, obj = pc.new(lib, kind, *pc.ctor_args(name))
    assert st == 0 and obj, (kind, name, st)
    assert (pc.fn(lib, kind, "minIndex")(obj), pc.fn(lib, kind, "maxIndex")(obj)) == (mn, mx) == (p["minIndex"], p["maxIndex"]), name
    fre = pc.call(lib, kind, obj, x)
    T = len(fre)
    dfre, dval = np.full(T + 2, 7.0, np.float32), np.full(T + 2, 7.0, np.float32)
    assert pc.fn(lib, kind, "pitchBatchDevice")(obj, P(x), 1, len(x), len(x), P(dfre), P(dval), T + 2, None) == 0
    curve = np.full((T, mx + 1), 9.0, np.float32)
    assert pc.fn(lib, kind, "curveBatchDevice")(obj, P(x), 1, len(x), len(x), P(curve), None) == 0
    pc.fn(lib, kind, "free")(obj)
    assert same_bits(dfre[:T], fre) and (dfre[T:] == 7).all() and (dval[T:] == 7).all(), name
    frames = pr.pitch(kind, x, pc.restate_window(p), r, hop, mn, mx)
    w = check_case(f"{kind}/{name}", frames, gold[f"{kind}/{name}/eps"], gold[f"{kind}/{name}/fre"], fre, sr, curve)
    for t in range(T):  # the value is the curve's entry at the chosen index, bit for bit
        i = index_of(fre[t], sr)
        assert same_bits(dval[t:t + 1], curve[t, i:i + 1]), (kind, name, t, i)
    print(f"pitch_lag {kind} {name}: n_fft {1 << r}, hop {hop}, {T} frames: curve {w['worst_curve']:.3f} of its bar, "
          f"explained {w['explained']}", flush=True)


def extras(kind):
    new, call, fn = pc.new, pc.call, lambda what: pc.fn(lib, kind, what)
    # a strided batch from a misaligned base: bitwise the single calls, nothing written beyond a row's frames
    sr, r, hop = 16000, 9, 128
    n, clips, stride = 512 + 128 * 5 + 5, 3, 512 + 128 * 5 + 17
    buf = np.zeros(clips * stride + 1, np.float32)
    xs = buf[1:].reshape(clips, stride)
    for c, sig in enumerate(("tone:330", "stack:196", "glide")):
        xs[c, :n] = signal(sig, n, sr, seed=70 + c) + 0.01 * signal("noise", n, sr, seed=80 + c)  # (no empty bins under the log)
    st, obj = new(lib, kind, sr, 40.0, 2000.0, r, hop, pc.HAMM)
    assert st == 0
    T = fn("calTimeLength")(obj, n)
    single = [call(lib, kind, obj, xs[c, :n]) for c in range(clips)]
    f, v = np.full((clips + 1, T + 2), np.nan, np.float32), np.full((clips + 1, T + 2), np.nan, np.float32)
    assert fn("pitchBatchDevice")(obj, P(xs), clips, n, stride, P(f), P(v), T + 2, None) == 0
    for c in range(clips):
        assert same_bits(f[c, :T], single[c]), c
    assert np.isnan(f[:clips, T:]).all() and np.isnan(f[clips]).all() and np.isnan(v[:clips, T:]).all() and np.isnan(v[clips]).all()
    assert not np.isnan(v[:clips, :T]).any()
    assert fn("pitchBatchDevice")(obj, P(xs), clips, n, stride, None, None, T, None) == -6
    assert fn("pitchBatchDevice")(obj, P(xs), clips, n, stride, P(f), None, T - 1, None) == -6
    assert fn("pitchBatchDevice")(obj, P(xs), clips, n, n - 1, P(f), None, T, None) == -6
    assert fn("pitchBatchDevice")(obj, P(xs), 0, n, stride, P(f), None, T, None) == -6
    g = np.full(4, 3.0, np.float32)
    assert fn("pitchBatchDevice")(obj, P(xs), 1, 100, stride, P(g), None, 4, None) == 0 and (g == 3).all()
    fn("free")(obj)
    # streaming: three uneven pieces and random pieces == one call, hop below and above the frame length
    rng = np.random.default_rng(12)
    for r, hop in ((8, 64), (8, 100), (8, 300), (8, 700)):
        N = 1 << r
        x = signal("glide", N + hop * 9 + 31, sr, seed=90) + 0.01 * signal("noise", N + hop * 9 + 31, sr, seed=91)
        st, one = new(lib, kind, sr, 80.0, 2000.0, r, hop)
        assert st == 0
        whole = call(lib, kind, one, x)
        fn("free")(one)
        for cuts in ([len(x) // 5, len(x) // 5 + 2 * N + 3], sorted(rng.integers(1, len(x), 6).tolist())):
            st, obj = new(lib, kind, sr, 80.0, 2000.0, r, hop, cont=1)
            assert st == 0
            parts = [call(lib, kind, obj, p) for p in np.split(x, cuts) if len(p)]
            assert fn("pitchBatchDevice")(obj, P(x), 1, len(x), len(x), P(f), None, 1000, None) == -4
            fn("free")(obj)
            got = np.concatenate(parts)
            assert same_bits(got, whole), (r, hop, len(got), len(whole))
    print(f"pitch_lag {kind}: batches of 3 strided clips bitwise the single calls; streaming in pieces == one call at hops 64 / "
          "100 / 300 / 700 of 256; refusals", flush=True)


def main(argv):
    gold = np.load(os.path.join(pc.GOLDEN, "pitch_lag.npz"))
    names = [a for a in argv if a != "extras"] or (list(pc.SMALL) if not argv else [])
    for kind in pc.KINDS:
        for name in names:
            fixture_case(kind, name, gold)
        if not argv or "extras" in argv:
            extras(kind)
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
