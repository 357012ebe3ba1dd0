#!/usr/bin/env python3
"""afx_nsgt.hip as emulated device code through the C host object: every case of tests/nsgt_cases.py but oct84, all three
inputs, through nsgtObj_nsgt (+ nsgtObj_getCellData) and nsgtObj_nsgtBatchDevice at the bar of the GPU tests; three chunks
with an odd stride bitwise equal to three single calls; outputs pre-filled with NaN come back finite; 64 guard floats behind
each output unchanged; cells off gives the same matrix; nsgtObj_setMinLength equals a fresh object.
The spectrum comes from the float64 stand-in of tests/emu/nsgt_emulated.cpp: this run exercises the band kernel only.
AFX_LIB = the library tests/test_nsgt_emulated.py builds.  Arguments: case names (default: all but oct84) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import audioflux_amd as af  # noqa: E402  (AFX_LIB: the emulated library)
from tests import nsgt_cases as nc  # noqa: E402

GUARD = 64
lib = af.get_lib()
lib.nsgtObj_nsgtBatchDevice.restype = C.c_int
lib.nsgtObj_nsgtBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 5


def make(c, min_len=None):
    return af.NSGT(num=c.num, radix2_exp=c.r, samplate=c.sr, low_fre=c.low, high_fre=c.high, bin_per_octave=c.bpo,
                   min_len=c.min_len if min_len is None else min_len, nsgt_filter_bank_type=af.NSGTFilterBankType(c.bank),
                   scale_type=af.SpectralFilterBankScaleType(nc.SCALE[c.scale]),
                   style_type=af.SpectralFilterBankStyleType(nc.STYLE[c.style]),
                   normal_type=af.SpectralFilterBankNormalType(nc.NORMAL[c.normal]))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def guarded(n):
    a = np.full(n + GUARD, np.nan, np.float32)
    a[n:] = 7.5
    return a


def batch(o, x, stride, cells=True):
    """x [chunks][N] laid out with `stride`; -> re, im [chunks][num][max], cre, cim [chunks][total] (float32)"""
    chunks, N = x.shape
    mx, tot = o.get_max_time_length(), o.get_total_time_length()
    buf = np.zeros(chunks * stride + 1, np.float32)
    for q in range(chunks):
        buf[1 + q * stride:1 + q * stride + N] = x[q]
    outs = [guarded(chunks * o.num * mx), guarded(chunks * o.num * mx), guarded(chunks * tot), guarded(chunks * tot)]
    ptr = [a.ctypes.data for a in outs]
    st = lib.nsgtObj_nsgtBatchDevice(o._obj, buf.ctypes.data + 4, chunks, stride, ptr[0], ptr[1], ptr[2] if cells else None,
                                     ptr[3] if cells else None, None)
    assert st == 0, (st, af.last_error())
    for a in outs:
        assert (a[-GUARD:] == 7.5).all(), "wrote behind an output"
    re, im = (a[:-GUARD].reshape(chunks, o.num, mx) for a in outs[:2])
    cre, cim = (a[:-GUARD].reshape(chunks, tot) for a in outs[2:])
    assert np.isfinite(re).all() and np.isfinite(im).all(), "a matrix element nobody wrote"
    if cells:
        assert np.isfinite(cre).all() and np.isfinite(cim).all(), "a cell nobody wrote"
    else:
        assert np.isnan(cre).all() and np.isnan(cim).all(), "cells written although not asked for"
    return re, im, cre, cim


def singles(o, x):
    mats, cells = [], []
    for xc in x:
        m = o.nsgt(xc)
        mats.append(m)
        cells.append(np.concatenate(o.get_cell_data()))
    return np.stack(mats), np.stack(cells)


def case(name):
    c = nc.by_name(name)
    x = nc.inputs(name)
    o = make(c)
    p = nc.product_plan(name)
    assert o.get_max_time_length() == p.max and o.get_total_time_length() == p.total
    assert np.array_equal(o.get_time_length_arr(), p.len) and same_bits(o.get_fre_band_arr(), p.fre)
    assert np.array_equal(o.get_bin_band_arr(), p.bin)
    mats, cells = singles(o, x)
    w1 = nc.judge(name, range(3), cells, mats, tag=" emulated nsgtObj_nsgt")
    re, im, cre, cim = batch(o, x, (1 << c.r) + 3)
    w2 = nc.judge(name, range(3), cre + 1j * cim, re + 1j * im, tag=" emulated nsgtObj_nsgtBatchDevice")
    assert same_bits(re, np.ascontiguousarray(mats.real)) and same_bits(im, np.ascontiguousarray(mats.imag)), "batch != singles"
    assert same_bits(cre, np.ascontiguousarray(cells.real)) and same_bits(cim, np.ascontiguousarray(cells.imag)), "batch cells != singles"
    re2, im2, _, _ = batch(o, x, (1 << c.r) + 3, cells=False)
    assert same_bits(re2, re) and same_bits(im2, im), "cells off changes the matrix"
    print(f"nsgt {name}: lengths {p.len.min()} ... {p.len.max()}, worst error / bar {max(w1, w2):.2f}; strided batch of 3 == singles "
          f"bitwise, guards intact", flush=True)


def extras():
    # nsgtObj_setMinLength rebuilds the WHOLE plan: getters, cells and matrix of a fresh object
    c = nc.by_name("mel12")
    x = nc.inputs("mel12")
    o = make(c)
    for m in (40, 1, 3):
        o.set_min_length(m)
        fresh = make(c, m)
        assert o.get_max_time_length() == fresh.get_max_time_length() and o.get_total_time_length() == fresh.get_total_time_length()
        assert np.array_equal(o.get_time_length_arr(), fresh.get_time_length_arr())
        a, b = singles(o, x), singles(fresh, x)
        assert same_bits(np.ascontiguousarray(a[0].real), np.ascontiguousarray(b[0].real)) and same_bits(a[1].view(np.float32), b[1].view(np.float32)), m
    before = singles(o, x)
    try:
        o.set_min_length(1000)  # longer than the 512 samples of a chunk: refused, the object stays
        raise SystemExit("a band longer than the chunk was accepted")
    except RuntimeError:
        pass
    after = singles(o, x)
    assert same_bits(before[0].view(np.float32), after[0].view(np.float32)) and o.get_max_time_length() == p_max(o)
    # refusals
    buf = np.zeros(3 * 600, np.float32)
    out = np.zeros(3 * o.num * o.get_max_time_length(), np.float32)
    f = lib.nsgtObj_nsgtBatchDevice
    assert f(o._obj, buf.ctypes.data, 1, 512, None, out.ctypes.data, None, None, None) == -6
    assert f(o._obj, buf.ctypes.data, 0, 512, out.ctypes.data, out.ctypes.data, None, None, None) == -6
    assert f(o._obj, buf.ctypes.data, 1, 511, out.ctypes.data, out.ctypes.data, None, None, None) == -6
    assert f(o._obj, buf.ctypes.data, 1, 512, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, None) == -6
    print("nsgt set_min_length 40 / 1 / 3 == fresh objects bitwise; 1000 refused, object unchanged; refusals", flush=True)


def p_max(o):
    return int(o.get_time_length_arr().max())


def main(argv):
    names = [a for a in argv if a != "extras"] or ([c.name for c in nc.CASES if c.name != "oct84"] if not argv else [])
    for name in names:
        case(name)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
