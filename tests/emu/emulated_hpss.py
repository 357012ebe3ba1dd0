#!/usr/bin/env python3
"""afx_hpss.hip as emulated device code: (a) afx_medianFilterDevice BITWISE against the sort-based numpy statement
(tests/hpss_restate.py) for every odd order 1 ... 63 and fallback orders, both axes, planes smaller than the window, tile-edge
shapes (rows / cols = tile +- 1) and clip boundaries; (b) hpssObj_hpss through the C host object against tests/golden/hpss.npz
by the rule of the GPU tests (tests/hpss_check.py), plus order 1 (identity, our deviation) and batches / chunks / the magnitude
planes against single calls and the float64 restatement.  AFX_LIB = the library tests/test_hpss_emulated.py builds.
Arguments: "median", "hpss" (default: both)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import hpss_cases as hc  # noqa: E402
from tests import hpss_restate as hr  # noqa: E402
from tests.golden.make_hpss_golden import bind, fp, run  # noqa: E402
from tests.hpss_check import check_waveform  # noqa: E402

lib = C.CDLL(os.environ["AFX_LIB"])
bind(lib)
lib.afx_medianFilterDevice.restype = C.c_int
lib.afx_medianFilterDevice.argtypes = [fp, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_void_p]
lib.hpssObj_hpssBatchDevice.restype = C.c_int
lib.hpssObj_hpssBatchDevice.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_longlong, fp, fp, C.c_longlong, C.c_void_p]
lib.hpssObj_spectraBatchDevice.restype = C.c_int
lib.hpssObj_spectraBatchDevice.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_longlong, fp, fp, C.c_void_p]


def median(plane, axis, order, fpc=0):
    out = np.full(plane.shape, np.nan, np.float32)
    st = lib.afx_medianFilterDevice(plane.ctypes.data_as(fp), plane.shape[0], plane.shape[1], fpc, axis, order,
                                    out.ctypes.data_as(fp), None)
    assert st == 0, (st, plane.shape, axis, order)
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def median_cases():
    rng = np.random.default_rng(5)
    n = 0
    # every register-path order and two rank-counting ones on a plane that spans tiles in both directions
    plane = rng.standard_normal((70, 131)).astype(np.float32) ** 2
    for order in list(range(1, 64, 2)) + [65, 101]:
        for axis in (0, 1):
            assert same_bits(median(plane, axis, order), hr.median_filter(plane, axis, order)), (order, axis)
            n += 1
    print(f"median: orders 1 ... 63, 65, 101 on [70, 131], both axes: bitwise", flush=True)
    # tile edges (64 frames x 128 columns), planes smaller than the window, negative values and ties
    for rows, cols in ((63, 127), (64, 128), (65, 129), (1, 1), (3, 2), (2, 300), (130, 5)):
        p = rng.standard_normal((rows, cols)).astype(np.float32)
        p[rng.random((rows, cols)) < 0.2] = 0.5  # ties
        for order in (3, 21, 31, 63, 255):
            for axis in (0, 1):
                assert same_bits(median(p, axis, order), hr.median_filter(p, axis, order)), (rows, cols, order, axis)
                n += 1
    print("median: tile-edge and tiny planes, ties, orders 3 / 21 / 31 / 63 / 255: bitwise", flush=True)
    # clips: axis 0 restarts at every clip (the last one shorter), axis 1 does not care
    p = rng.standard_normal((3 * 23 + 7, 40)).astype(np.float32)
    for order in (5, 21, 65):
        assert same_bits(median(p, 0, order, 23), hr.median_filter(p, 0, order, 23)), order
        assert same_bits(median(p, 1, order, 23), hr.median_filter(p, 1, order)), order
        for c in range(3):
            assert same_bits(median(p, 0, order, 23)[c * 23:(c + 1) * 23], median(np.ascontiguousarray(p[c * 23:(c + 1) * 23]), 0, order))
        n += 2
    print("median: clips of 23 frames (+ a short one) equal per-clip calls: bitwise", flush=True)
    # refusals
    q = np.zeros((4, 4), np.float32)
    o = np.zeros_like(q)
    for order in (0, 2, 257, -3):
        assert lib.afx_medianFilterDevice(q.ctypes.data_as(fp), 4, 4, 0, 0, order, o.ctypes.data_as(fp), None) == -4, order
    assert lib.afx_medianFilterDevice(q.ctypes.data_as(fp), 4, 4, 0, 2, 3, o.ctypes.data_as(fp), None) == -6
    assert lib.afx_medianFilterDevice(q.ctypes.data_as(fp), 4, 4, 0, 0, 3, q.ctypes.data_as(fp), None) == -6
    print(f"median cases: {n}", flush=True)


def new(r, w, h, p):
    obj = C.c_void_p()
    st = lib.hpssObj_new(C.byref(obj), r, C.byref(C.c_int(w)), None, C.byref(C.c_int(h)), C.byref(C.c_int(p)))
    assert st == 0, st
    return obj


def hpss_cases():
    gold = np.load(os.path.join(hc.GOLDEN, "hpss.npz"))
    for name, (r, w, h, p, kind, n, outs, init) in hc.CASES.items():
        x = hc.case_input(name)
        ih, ip_ = hc.initial(name, "h"), hc.initial(name, "p")
        ha, pa = run(lib, x, r, w, h, p, outs, ih, ip_)
        worst = 0.0
        for key, got in (("h", ha), ("p", pa)):
            if key in outs:
                worst = max(worst, check_waveform(f"{name}/{key}", got, gold[f"{name}/{key}"], np.abs(x).max(), r, w))
            else:
                assert got is None and f"{name}/{key}" not in gold
        print(f"hpss {name}: n_fft {1 << r}, orders {h} / {p}, {len(x)} samples: worst {worst:.2e} of the input peak", flush=True)
    # order 1 is the identity (the reference masks with stale memory there): against the restatement
    x = hc.signal("mix", 1024 + 256 * 12, seed=99)
    for h, p in ((1, 31), (21, 1), (1, 1)):
        ha, pa = run(lib, x, 10, hc.HAMM, h, p)
        wh, wp = hr.hpss(x, 10, hc.HAMM, h, p)
        check_waveform(f"order {h}/{p} h", ha, wh, np.abs(x).max(), 10, hc.HAMM)
        check_waveform(f"order {h}/{p} p", pa, wp, np.abs(x).max(), 10, hc.HAMM)
    print("hpss orders 1/31, 21/1, 1/1 against the float64 restatement", flush=True)
    # a batch with a clip stride, in one chunk and in chunks of one clip: bitwise the single-clip calls; magnitude planes
    r, n, clips, stride = 9, 512 + 128 * 30 + 5, 3, 512 + 128 * 30 + 16
    m = hc.out_length(r, n)
    xs = np.zeros((clips, stride), np.float32)
    for c in range(clips):
        xs[c, :n] = hc.signal("mix", n, seed=50 + c)
    obj = new(r, hc.HAMM, 21, 31)
    single = [run(lib, xs[c, :n], r, hc.HAMM, 21, 31) for c in range(clips)]
    for chunk_mb in (None, "1"):
        if chunk_mb:
            os.environ["AFX_HPSS_CHUNK_MB"] = chunk_mb
        dh, dp = np.zeros((clips, m + 3), np.float32), np.zeros((clips, m + 3), np.float32)
        st = lib.hpssObj_hpssBatchDevice(obj, xs.ctypes.data_as(fp), clips, n, stride, dh.ctypes.data_as(fp), dp.ctypes.data_as(fp),
                                         m + 3, None)
        assert st == 0, st
        for c in range(clips):
            assert same_bits(dh[c, :m], single[c][0]) and same_bits(dp[c, :m], single[c][1]), (chunk_mb, c)
        assert not dh[:, m:].any() and not dp[:, m:].any(), "wrote behind a clip"
        os.environ.pop("AFX_HPSS_CHUNK_MB", None)
    t, f = (n - 512) // 128 + 1, 257
    hm, pm = np.zeros((clips, t, f), np.float32), np.zeros((clips, t, f), np.float32)
    assert lib.hpssObj_spectraBatchDevice(obj, xs.ctypes.data_as(fp), clips, n, stride, hm.ctypes.data_as(fp), pm.ctypes.data_as(fp),
                                          None) == 0
    for c in range(clips):
        s, mag, wh, wp = hr.spectra(xs[c, :n], r, hc.HAMM, 21, 31)
        # (the soft mask divides by h^2 + p^2: where both medians are rounding noise the float32 mask is free; judged by the plane's peak)
        assert np.abs(hm[c] - wh).max() <= 1e-5 * mag.max() and np.abs(pm[c] - wp).max() <= 1e-5 * mag.max(), c
        assert np.abs(hm[c] + pm[c] - mag).max() <= 1e-5 * mag.max()
    assert lib.hpssObj_hpssBatchDevice(obj, xs.ctypes.data_as(fp), clips, n, stride, None, None, m, None) == -6
    assert lib.hpssObj_hpssBatchDevice(obj, xs.ctypes.data_as(fp), clips, n, stride, dh.ctypes.data_as(fp), None, m - 1, None) == -6
    lib.hpssObj_free(obj)
    print("hpss batch of 3 strided clips: one chunk and chunks of one clip bitwise the single calls; magnitude planes", flush=True)


def main(argv):
    what = argv or ["median", "hpss"]
    if "median" in what:
        median_cases()
    if "hpss" in what:
        hpss_cases()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
