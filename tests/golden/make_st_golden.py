#!/usr/bin/env python3
"""Writes tests/golden/st.npz: what the compiled reference gives for every case of tests/st_cases.py, by raw ctypes through
the reference driver's lib().  Per case and input of the case: the reference's rows, complex64 -- the whole matrix for r4full,
r6full and r9list, the case's selection of rows (and of columns at 2^14) elsewhere.  Per case: the reference-vs-float64
error of its inputs over ALL its rows on the metric of tests/st_cases.py (the bar of the GPU tests is max(1e-5, 2 x that)).

    python tests/golden/make_st_golden.py        (needs the compiled reference; 2^14 takes its 537 MB window table)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import st_cases as sc  # noqa: E402

fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)


def bind(L):
    L.stObj_new.restype, L.stObj_new.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, fp, fp]
    L.stObj_useBinArr.restype, L.stObj_useBinArr.argtypes = None, [C.c_void_p, ip, C.c_int]
    L.stObj_setValue.restype, L.stObj_setValue.argtypes = None, [C.c_void_p, C.c_float, C.c_float]
    L.stObj_st.restype, L.stObj_st.argtypes = None, [C.c_void_p, fp, fp, fp]
    L.stObj_free.restype, L.stObj_free.argtypes = None, [C.c_void_p]
    return L


def ref_new(L, r, lo, hi, factor=None, norm=None, bins=None):
    obj = C.c_void_p(None)
    f = C.byref(C.c_float(factor)) if factor is not None else None
    n = C.byref(C.c_float(norm)) if norm is not None else None
    st = L.stObj_new(C.byref(obj), r, lo, hi, f, n)
    assert st == 0 and obj, (r, st)
    if bins is not None:
        b = np.ascontiguousarray(bins, np.int32)
        L.stObj_useBinArr(obj, b.ctypes.data_as(ip), len(b))
    return obj


def ref_rows(L, obj, x, r, rows):
    """-> complex64 [rows][N]; the planes start as zeros, as the reference's wrapper hands them over"""
    N = 1 << r
    x = np.ascontiguousarray(x, np.float32)
    re, im = np.zeros((rows, N), np.float32), np.zeros((rows, N), np.float32)
    L.stObj_st(obj, x.ctypes.data_as(fp), re.ctypes.data_as(fp), im.ctypes.data_as(fp))
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def case_data(L, c):
    """{key: array} of one case"""
    bins = sc.rows_of(c)
    obj = ref_new(L, c.r, c.lo, c.hi, c.factor, c.norm, c.bins)
    out, r_ref = {}, []
    for k in c.chunks:
        x = sc.inputs(c.name)[k]
        rows = ref_rows(L, obj, x, c.r, len(bins))
        out[f"{c.name}/{sc.INPUTS[k]}/rows"] = sc.select(c, rows)
        w = sc.f64_st(x, c.r, bins, c.factor, c.norm)
        r_ref.append(np.abs(rows.astype(np.complex128) - w).max() / np.abs(w).max())
    out[f"{c.name}/ref_vs_f64"] = np.array(r_ref, np.float64)
    L.stObj_free(obj)
    return out


def main():
    from oracle import ref
    L = bind(ref.lib())
    out = {}
    for c in sc.CASES:
        d = case_data(L, c)
        out.update(d)
        print(f"{c.name}: reference vs float64 {d[c.name + '/ref_vs_f64']}", flush=True)
    np.savez_compressed(sc.GOLDEN, **out)
    print(f"{sc.GOLDEN}: {os.path.getsize(sc.GOLDEN)} bytes")
    assert os.path.getsize(sc.GOLDEN) < 600000


if __name__ == "__main__":
    main()
