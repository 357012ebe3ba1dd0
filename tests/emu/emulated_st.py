#!/usr/bin/env python3
"""afx_st.hip as emulated device code through the C host object: the cases r4full, r6full, r9list and three rows of r9fn of
tests/st_cases.py, all three inputs, through stObj_st and stObj_stBatchDevice at the bar of the GPU tests; three chunks with an
odd stride bitwise equal to three single calls; outputs pre-filled with NaN come back finite; 64 guard floats behind each
output unchanged; planes that are not 16-byte aligned take the dword stores and give the same bits; the row of bin 0 writes
zeros to the imaginary plane; setValue and back equals a fresh object; refusals.
The spectrum comes from the float64 stand-in of tests/emu/st_emulated.cpp: this run exercises the row kernel only.
AFX_LIB = the library tests/test_st_emulated.py builds.  Arguments: case names (default: the four above) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import audioflux_amd as af  # noqa: E402  (AFX_LIB: the emulated library)
from tests import st_cases as sc  # noqa: E402

GUARD = 64
DEFAULT = ("r4full", "r6full", "r9list", "r9fn")
fp = C.POINTER(C.c_float)
lib = af.get_lib()
lib.stObj_new.restype, lib.stObj_new.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, fp, fp]
lib.stObj_useBinArr.restype, lib.stObj_useBinArr.argtypes = None, [C.c_void_p, C.c_void_p, C.c_int]
lib.stObj_setValue.restype, lib.stObj_setValue.argtypes = None, [C.c_void_p, C.c_float, C.c_float]
lib.stObj_st.restype, lib.stObj_st.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.stObj_free.restype, lib.stObj_free.argtypes = None, [C.c_void_p]
lib.stObj_getBinLength.restype, lib.stObj_getBinLength.argtypes = C.c_int, [C.c_void_p]
lib.stObj_stBatchDevice.restype = C.c_int
lib.stObj_stBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
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


def new(r, lo, hi, factor=None, norm=None, bins=None):
    o = C.c_void_p(None)
    st = lib.stObj_new(C.byref(o), r, lo, hi, C.byref(C.c_float(factor)) if factor is not None else None,
                       C.byref(C.c_float(norm)) if norm is not None else None)
    assert st == 0 and o, (r, st, af.last_error())
    if bins is not None:
        b = np.ascontiguousarray(bins, np.int32)
        lib.stObj_useBinArr(o, b.ctypes.data, len(b))
        assert lib.stObj_getBinLength(o) == len(b)
    return o


def batch(o, x, stride, shift=0):
    """x [chunks][N] laid out with `stride`, 4 bytes behind a 16-byte boundary, NaN in the gaps -> [chunks][rows][N]"""
    chunks, N = x.shape
    rows = lib.stObj_getBinLength(o)
    buf = guarded(chunks * stride, 1)
    for q in range(chunks):
        buf[q * stride:q * stride + N] = x[q]
    outs = [guarded(chunks * rows * N, shift), guarded(chunks * rows * N, shift)]
    st = lib.stObj_stBatchDevice(o, buf.ctypes.data, chunks, stride, outs[0].ctypes.data, outs[1].ctypes.data, None)
    assert st == 0, (st, af.last_error())
    for a in outs:
        assert (a[-GUARD:] == 7.5).all(), "wrote behind an output"
        assert np.isfinite(a[:-GUARD]).all(), "an element nobody wrote (or the gaps of x were read)"
    return cplx(*(a[:-GUARD].reshape(chunks, rows, N) for a in outs))


def single(o, x):
    N = len(x)
    rows = lib.stObj_getBinLength(o)
    x = np.ascontiguousarray(x, np.float32)
    re, im = guarded(rows * N), guarded(rows * N)
    lib.stObj_st(o, x.ctypes.data, re.ctypes.data, im.ctypes.data)
    assert (re[-GUARD:] == 7.5).all() and (im[-GUARD:] == 7.5).all(), "wrote behind an output"
    return cplx(re[:-GUARD].reshape(rows, N), im[:-GUARD].reshape(rows, N))


def case(name):
    c = sc.by_name(name)
    N = 1 << c.r
    x = sc.inputs(name)[list(c.chunks)]
    pos = None
    if name == "r9fn":  # three rows of the 256: the fixture's selection, as a list
        pos = list(c.store)
        o = new(c.r, c.lo, c.hi, c.factor, c.norm, [sc.rows_of(c)[p] for p in pos])
    else:
        o = new(c.r, c.lo, c.hi, c.factor, c.norm, c.bins)
    bins = sc.rows_of(c) if pos is None else [sc.rows_of(c)[p] for p in pos]
    assert lib.stObj_getBinLength(o) == len(bins)
    rows = batch(o, x, N + 3)
    worst = sc.judge(name, c.chunks, rows, tag=" emulated stObj_stBatchDevice", pos=pos)
    ones = np.stack([single(o, xc) for xc in x])
    assert same_bits(rows, ones), "batch != single host calls"
    assert same_bits(batch(o, x, N, shift=1), rows), "unaligned planes (dword stores) change the results"
    for i, k in enumerate(bins):
        if k == 0:
            assert not rows[:, i].imag.any() and (rows[:, i].real == rows[:, i, :1].real).all(), "the row of bin 0"
    if name == "r9fn":  # setValue to 1, 1 equals a fresh object bit for bit, and back again
        lib.stObj_setValue(o, 1.0, 1.0)
        fresh = new(c.r, c.lo, c.hi, None, None, bins)
        a, b = batch(o, x, N + 3), batch(fresh, x, N + 3)
        assert same_bits(a, b) and not same_bits(a, rows), "setValue(1, 1) != a fresh object"
        lib.stObj_setValue(o, c.factor, c.norm)
        assert same_bits(batch(o, x, N + 3), rows), "setValue back"
        lib.stObj_free(fresh)
    lib.stObj_free(o)
    print(f"st {name}: worst error / bar {worst:.2f}; strided batch == singles bitwise, guards intact", flush=True)


def extras():
    r, N = 6, 64
    o = new(r, 5, 5)  # minIndex >= maxIndex: the reference's fall-back to the full range
    assert lib.stObj_getBinLength(o) == N // 2 + 1
    lib.stObj_free(o)
    o = new(r, 3, 9)
    assert lib.stObj_getBinLength(o) == 7 and lib.stObj_getBinLength(None) == 0
    x = guarded(3 * N)
    x[:] = 0.25
    out = guarded(3 * 7 * N)
    xp, op = x.ctypes.data, out.ctypes.data
    f = lib.stObj_stBatchDevice
    for a in ((None, xp, 1, N, op, op), (o, None, 1, N, op, op), (o, xp, 1, N, None, op), (o, xp, 1, N, op, None),
              (o, xp, 0, N, op, op), (o, xp, -2, N, op, op), (o, xp, 1, N - 1, op, op)):
        assert f(*a, None) == -6, a
    assert np.isnan(out[:-GUARD]).all(), "a refused call wrote"
    # useBinArr: an entry out of range is ignored silently; an empty or over-long list is refused and counted
    before = lib.afxdev_error_count()
    for bad in ([3, 33], [-1], [4, 5, 64]):
        b = np.array(bad, np.int32)
        lib.stObj_useBinArr(o, b.ctypes.data, len(b))
        assert lib.stObj_getBinLength(o) == 7
    assert lib.afxdev_error_count() == before
    b = np.zeros(N + 1, np.int32)
    for length in (0, -3, N + 1):
        before = lib.afxdev_error_count()
        lib.stObj_useBinArr(o, b.ctypes.data, length)
        assert lib.afxdev_error_count() > before and lib.stObj_getBinLength(o) == 7
    lib.stObj_useBinArr(o, b.ctypes.data, N)  # N rows of bin 0: the longest list
    assert lib.stObj_getBinLength(o) == N
    xs = np.ascontiguousarray(sc.inputs("r6full")[0])
    m = single(o, xs)
    assert (m.real == m.real[0, 0]).all() and not m.imag.any() and abs(m.real[0, 0] - xs.mean()) < 1e-6
    lib.stObj_free(o)
    lib.stObj_free(None)
    for rr in (3, 15, 0, -1):
        o = C.c_void_p(1)
        assert lib.stObj_new(C.byref(o), rr, 0, 4, None, None) == -4 and not o
    print("st refusals leave the outputs untouched; useBinArr rules; the full-range fall-back", flush=True)


def main(argv):
    for name in [a for a in argv if a != "extras"] or (DEFAULT if not argv else ()):
        case(name)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
