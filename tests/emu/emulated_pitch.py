#!/usr/bin/env python3
"""afx_pitch_yin.hip as emulated device code through the C host object: every case of tests/golden/pitch_yin.npz by the rule
of the GPU tests (tests/pitch_check.py) -- results, candidate lists and, through pitchYINObj_curveBatchDevice, the curve --,
"not found" frames (host call keeps the caller's entries, device call writes 0), a strided batch bitwise equal to single
calls, capped candidate lists, streaming in pieces == one call (hop below and above fftLength), refusals.
AFX_LIB = the library tests/test_pitch_emulated.py builds.  Arguments: case names (default: all) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import pitch_cases as pc  # noqa: E402
from tests import pitch_restate as pr  # noqa: E402
from tests.golden.make_pitch_golden import bind, call, fp, ip, new  # noqa: E402
from tests.pitch_check import check_candidates, check_case  # noqa: E402

lib = C.CDLL(os.environ["AFX_LIB"])
bind(lib)
ll = C.c_longlong
lib.pitchYINObj_pitchBatchDevice.restype = C.c_int
lib.pitchYINObj_pitchBatchDevice.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, ll, fp, fp, fp, ll, C.c_void_p]
lib.pitchYINObj_troughsBatchDevice.restype = C.c_int
lib.pitchYINObj_troughsBatchDevice.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, ll, fp, fp, ip, C.c_int, C.c_void_p]
lib.pitchYINObj_curveBatchDevice.restype = C.c_int
lib.pitchYINObj_curveBatchDevice.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, ll, fp, C.c_void_p]


def P(a, t=fp):
    return a.ctypes.data_as(t)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fixture_case(name, gold):
    sr, lo, hi, r, hop, auto, thresh, kind, n = pc.CASES[name]
    x = pc.case_input(name)
    mi, ma, ylen, mlen = pc.plan(sr, lo, hi, r, hop, auto)
    st, obj = new(lib, sr, lo, hi, r, hop, auto)
    assert st == 0 and obj, (name, st)
    lib.pitchYINObj_setThresh(obj, thresh)
    fre, val, mn, lens, cf, cv = call(lib, obj, x)
    T = len(fre)
    curve = np.full((T, ylen), np.nan, np.float32)
    assert lib.pitchYINObj_curveBatchDevice(obj, P(x), 1, len(x), len(x), P(curve), None) == 0
    # the device call writes every frame: 0 where the host call left the caller's NaN
    dfre, dval, dmn = (np.full(T + 2, 7.0, np.float32) for _ in range(3))
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(x), 1, len(x), len(x), P(dfre), P(dval), P(dmn), T + 2, None) == 0
    lib.pitchYINObj_free(obj)
    unv = np.isnan(fre)
    assert np.array_equal(np.isnan(val), unv), name
    assert not dfre[:T][unv].any() and not dval[:T][unv].any() and (dfre[T:] == 7).all(), name
    assert same_bits(dfre[:T][~unv], fre[~unv]) and same_bits(dval[:T][~unv], val[~unv]) and same_bits(dmn[:T], mn), name
    ref = {k: gold[f"{name}/{k}"] for k in ("fre", "trough", "min", "len")}
    frames = pr.pitch(x, sr, r, hop, auto, mi, ma, thresh)
    w = check_case(name, frames, ref, {"fre": fre, "trough": val, "min": mn, "len": lens}, sr, mi, curve)
    # candidate lists of the frames that agree in count: same lags, values within the curve's bar
    gf, gv = gold[f"{name}/cand_fre"], gold[f"{name}/cand_val"]
    for t in range(T):
        if lens[t] == ref["len"][t] and frames[t]["snap_margin"] >= 1e-4:
            k = int(lens[t])
            eps = max(1e-5, 4 * abs(float(ref["min"][t]) - frames[t]["min"]))
            check_candidates(name, t, frames[t], sr, mi, eps, cf[t, :k], cv[t, :k], gf[t, :k], gv[t, :k])
            assert not cf[t, k:].any() and not cv[t, k:].any(), (name, t)
    print(f"pitch {name}: n_fft {1 << r}, hop {hop}, auto {auto}, {T} frames, {int((~unv).sum())} voiced: min {w['worst_min']:.1e} "
          f"curve {w['worst_curve']:.1e} fre {w['worst_fre']:.1e} explained {w['explained']}", flush=True)


def extras():
    # a strided batch: bitwise the single calls; capped candidate lists; refusals
    sr, r, hop, auto = 16000, 9, 128, 256
    n, clips, stride = 512 + 128 * 9 + 5, 3, 512 + 128 * 9 + 16
    xs = np.zeros((clips, stride), np.float32)
    for c, kind in enumerate(("tone:330", "bursts", "glide")):
        xs[c, :n] = pc.signal(kind, n, sr, seed=70 + c)
    st, obj = new(lib, sr, 60.0, 2000.0, r, hop, auto)
    assert st == 0
    T = lib.pitchYINObj_calTimeLength(obj, n)
    single = [call(lib, obj, xs[c, :n], fill=0.0) for c in range(clips)]
    f, v, m = (np.full((clips, T + 1), 5.0, np.float32) for _ in range(3))
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), clips, n, stride, P(f), P(v), P(m), T + 1, None) == 0
    for c in range(clips):
        assert same_bits(f[c, :T], single[c][0]) and same_bits(v[c, :T], single[c][1]) and same_bits(m[c, :T], single[c][2]), c
    assert (f[:, T] == 5).all() and (m[:, T] == 5).all(), "wrote behind a clip"
    f2 = np.full((clips, T), 5.0, np.float32)
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), clips, n, stride, P(f2), None, None, T, None) == 0
    assert same_bits(f2, f[:, :T])
    for pitch in (1, 2, 0):
        cf, cv = np.full((clips * T, max(pitch, 1)), -1.0, np.float32), np.full((clips * T, max(pitch, 1)), -1.0, np.float32)
        ln = np.full(clips * T, -1, np.int32)
        assert lib.pitchYINObj_troughsBatchDevice(obj, P(xs), clips, n, stride, P(cf) if pitch else None, P(cv) if pitch else None,
                                                  P(ln, ip), pitch, None) == 0
        for c in range(clips):
            lens, sf, sv = single[c][3], single[c][4], single[c][5]
            assert np.array_equal(ln[c * T:(c + 1) * T], lens), (pitch, c)
            for t in range(T):
                k = min(int(lens[t]), pitch)
                assert same_bits(cf[c * T + t, :k], sf[t, :k]) and same_bits(cv[c * T + t, :k], sv[t, :k])
                assert (cf[c * T + t, k:] == -1).all()
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), clips, n, stride, None, None, None, T, None) == -6
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), clips, n, stride, P(f), None, None, T - 1, None) == -6
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), clips, n, n - 1, P(f), None, None, T, None) == -6
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), 0, n, stride, P(f), None, None, T, None) == -6
    assert lib.pitchYINObj_pitchBatchDevice(obj, P(xs), 1, 100, stride, P(f), None, None, T, None) == 0  # no frame: nothing to do
    lib.pitchYINObj_free(obj)
    print("pitch batch of 3 strided clips bitwise the single calls; candidate lists capped at 1 / 2 / 0; refusals", flush=True)
    # streaming: pieces of random length == one call, hop below and above the frame length
    rng = np.random.default_rng(12)
    for r, hop in ((8, 64), (8, 100), (8, 300), (8, 700)):
        N = 1 << r
        x = pc.signal("glide", N + hop * 17 + 31, sr, seed=90)
        st, one = new(lib, sr, 100.0, 2000.0, r, hop, N // 2)
        assert st == 0
        whole = call(lib, one, x, fill=0.0)
        lib.pitchYINObj_free(one)
        st, obj = new(lib, sr, 100.0, 2000.0, r, hop, N // 2, cont=1)
        assert st == 0
        parts, at = [], 0
        while at < len(x):
            k = int(rng.integers(1, 2 * N + hop))
            piece = x[at:at + k]
            assert lib.pitchYINObj_calTimeLength(obj, len(piece)) >= 0
            parts.append(call(lib, obj, piece, fill=0.0))
            at += k
        assert lib.pitchYINObj_pitchBatchDevice(obj, P(x), 1, len(x), len(x), P(f), None, None, 1000, None) == -4
        lib.pitchYINObj_free(obj)
        for i in range(3):
            got = np.concatenate([p[i] for p in parts])
            assert same_bits(got, whole[i]), (r, hop, i, len(got), len(whole[i]))
        assert np.array_equal(np.concatenate([p[3] for p in parts]), whole[3])
    print("pitch streaming in random pieces == one call at hops 64 / 100 / 300 / 700 of 256", flush=True)


def main(argv):
    gold = np.load(os.path.join(pc.GOLDEN, "pitch_yin.npz"))
    names = [a for a in argv if a != "extras"] or (list(pc.CASES) if not argv else [])
    for name in names:
        fixture_case(name, gold)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
