#!/usr/bin/env python3
"""afx_fst.hip as emulated device code through the C host object: the cases r4full, r6full, r9default and the 15 + 8 rows of
r14edge of tests/fst_cases.py, all three inputs, through fstObj_fst and fstObj_fstBatchDevice (matrix + cells) at the bar of
the GPU tests; three chunks with an odd stride bitwise equal to three single calls; outputs pre-filled with NaN come back
finite; 64 guard floats behind each output unchanged; the cells-only and matrix-only forms write nothing else; a plane that is
not 16-byte aligned takes the dword stores and gives the same bits; refusals.
The spectrum comes from the float64 stand-in of tests/emu/fst_emulated.cpp: this run exercises the two FST kernels only.
AFX_LIB = the library tests/test_fst_emulated.py builds.  Arguments: case names (default: the four above) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import audioflux_amd as af  # noqa: E402  (AFX_LIB: the emulated library)
from tests import fst_cases as fc  # noqa: E402

GUARD = 64
DEFAULT = ("r4full", "r6full", "r9default", "r14edge")
lib = af.get_lib()
lib.fstObj_new.restype, lib.fstObj_new.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int]
lib.fstObj_fst.restype, lib.fstObj_fst.argtypes = None, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
lib.fstObj_free.restype, lib.fstObj_free.argtypes = None, [C.c_void_p]
lib.fstObj_fstBatchDevice.restype = C.c_int
lib.fstObj_fstBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 5
lib.afxdev_error_count.restype = C.c_int


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cplx(re, im):
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def guarded(n, shift=0):
    """n NaN floats and GUARD floats of 7.5 behind them, starting `shift` floats behind a 16-byte boundary"""
    raw = np.zeros(n + GUARD + 8, np.float32)
    at = (-(raw.ctypes.data // 4) % 4 + shift) % 4
    a = raw[at:at + n + GUARD]
    assert a.ctypes.data % 16 == 4 * shift
    a[:n], a[n:] = np.nan, 7.5
    return a


def new(r):
    o = C.c_void_p(None)
    st = lib.fstObj_new(C.byref(o), r)
    assert st == 0 and o, (r, st, af.last_error())
    return o


def batch(o, r, x, stride, lo, hi, matrix=True, cells=True, shift=0):
    """x [chunks][N] laid out with `stride`, 4 bytes behind a 16-byte boundary -> rows [chunks][hi-lo+1][N], cells complex64"""
    chunks, N = x.shape
    rows, cl = hi - lo + 1, N // 2 + 1
    buf = guarded(chunks * stride, 1)
    buf[:] = 0
    for q in range(chunks):
        buf[q * stride:q * stride + N] = x[q]
    outs = [guarded(chunks * rows * N, shift), guarded(chunks * rows * N, shift), guarded(chunks * cl), guarded(chunks * cl)]
    ptr = [a.ctypes.data for a in outs]
    st = lib.fstObj_fstBatchDevice(o, buf.ctypes.data, chunks, stride, lo, hi, ptr[0] if matrix else None,
                                   ptr[1] if matrix else None, ptr[2] if cells else None, ptr[3] if cells else None, None)
    assert st == 0, (st, af.last_error())
    for a in outs:
        assert (a[-GUARD:] == 7.5).all(), "wrote behind an output"
    re, im = (a[:-GUARD].reshape(chunks, rows, N) for a in outs[:2])
    cre, cim = (a[:-GUARD].reshape(chunks, cl) for a in outs[2:])
    for want, a, b, what in ((matrix, re, im, "matrix"), (cells, cre, cim, "cells")):
        if want:
            assert np.isfinite(a).all() and np.isfinite(b).all(), f"a {what} element nobody wrote"
        else:
            assert np.isnan(a).all() and np.isnan(b).all(), f"{what} written although not asked for"
    return cplx(re, im), cplx(cre, cim)


def single(o, r, x, lo, hi):
    N = 1 << r
    x = np.ascontiguousarray(x, np.float32)
    re, im = guarded((hi - lo + 1) * N), guarded((hi - lo + 1) * N)
    lib.fstObj_fst(o, x.ctypes.data, lo, hi, re.ctypes.data, im.ctypes.data)
    assert (re[-GUARD:] == 7.5).all() and (im[-GUARD:] == 7.5).all(), "wrote behind an output"
    return cplx(re[:-GUARD].reshape(hi - lo + 1, N), im[:-GUARD].reshape(hi - lo + 1, N))


def case(name):
    c = fc.by_name(name)
    x = fc.inputs(name)[list(c.chunks)]
    o = new(c.r)
    worst = 0.0
    for lo, hi in c.ranges:
        rows, cells = batch(o, c.r, x, (1 << c.r) + 3, lo, hi)
        worst = max(worst, fc.judge_cells(name, c.chunks, cells, tag=" emulated"),
                    fc.judge_rows(name, c.chunks, rows, lo, hi, tag=" emulated fstObj_fstBatchDevice"))
        assert same_bits(rows, np.stack([fc.expand(cl, c.r, lo, hi) for cl in cells])), "matrix != expansion of the cells"
        ones = np.stack([single(o, c.r, xc, lo, hi) for xc in x])
        assert same_bits(rows, ones), "batch != single host calls"
        r2, _ = batch(o, c.r, x, (1 << c.r) + 3, lo, hi, cells=False)
        _, c2 = batch(o, c.r, x, (1 << c.r) + 3, lo, hi, matrix=False)
        r3, _ = batch(o, c.r, x, 1 << c.r, lo, hi, cells=False, shift=1)  # dword stores
        assert same_bits(r2, rows) and same_bits(c2, cells) and same_bits(r3, rows), "the form of the call changes the results"
        if c.matrix:
            ref = fc.reference(name)
            e = max(np.abs(rows[q].astype(np.complex128) - ref.mat_c[k]).max() / ref.peak[k] for q, k in enumerate(c.chunks))
            assert e <= fc.FLOOR, ("stored matrix", e)
    lib.fstObj_free(o)
    print(f"fst {name}: worst error / bar {worst:.2f}; strided batch == singles bitwise, guards intact", flush=True)


def extras():
    r, N = 6, 64
    o = new(r)
    x = guarded(3 * N)
    x[:] = 0.25
    out = guarded(3 * 33 * N)
    xp, op = x.ctypes.data, out.ctypes.data
    f = lib.fstObj_fstBatchDevice
    bad = [(None, xp, 1, N, 0, 32, op, op, None, None), (o, None, 1, N, 0, 32, op, op, None, None),
           (o, xp, 1, N, 0, 32, op, None, None, None), (o, xp, 1, N, 0, 32, None, op, None, None),
           (o, xp, 1, N, 0, 32, op, op, op, None), (o, xp, 1, N, 0, 32, None, None, None, None),
           (o, xp, 0, N, 0, 32, op, op, None, None), (o, xp, 1, N - 1, 0, 32, op, op, None, None),
           (o, xp, 1, N, -1, 32, op, op, None, None), (o, xp, 1, N, 5, 4, op, op, None, None),
           (o, xp, 1, N, 0, 33, op, op, None, None)]
    for a in bad:
        assert f(*a, None) == -6, a
    assert np.isnan(out[:-GUARD]).all(), "a refused call wrote"
    # the host entry clamps like the reference; minIndex > maxIndex writes nothing and counts a failure
    xs = np.ascontiguousarray(fc.inputs("r6full")[0])
    a = single(o, r, xs, 0, 32)
    re, im = guarded(33 * N), guarded(33 * N)
    lib.fstObj_fst(o, xs.ctypes.data, -5, 99, re.ctypes.data, im.ctypes.data)
    assert same_bits(cplx(re[:-GUARD], im[:-GUARD]).reshape(33, N), a)
    before = lib.afxdev_error_count()
    re[:-GUARD] = np.nan
    lib.fstObj_fst(o, xs.ctypes.data, 9, 3, re.ctypes.data, im.ctypes.data)
    assert lib.afxdev_error_count() > before and np.isnan(re[:-GUARD]).all()
    lib.fstObj_free(o)
    lib.fstObj_free(None)
    print("fst refusals leave the outputs untouched; clamping; minIndex > maxIndex writes nothing and is counted", flush=True)


def main(argv):
    for name in [a for a in argv if a != "extras"] or (DEFAULT if not argv else ()):
        case(name)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
