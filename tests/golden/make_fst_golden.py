#!/usr/bin/env python3
"""Writes tests/golden/fst.npz: what the compiled reference gives for every row of tests/fst_cases.py, by raw ctypes through
the reference driver's lib().  Per case and input: the reference's cells -- one row per band (index 0, 1, 2 and n + 1 for
n = 2 ... N/4), decimated to its distinct columns, complex64 [N/2 + 1] in the library's cell order -- and, for the cases
marked `matrix`, the whole matrix of the case's range.  Per case: the reference-vs-float64 error of the three inputs on the
metric of tests/fst_cases.py (the bar of the GPU tests is max(1e-5, 2 x that)).

    python tests/golden/make_fst_golden.py        (needs the compiled reference; 2^14 takes its 537 MB table)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import fst_cases as fc  # noqa: E402

fp = C.POINTER(C.c_float)


def bind(L):
    L.fstObj_new.restype, L.fstObj_new.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int]
    L.fstObj_fst.restype, L.fstObj_fst.argtypes = None, [C.c_void_p, fp, C.c_int, C.c_int, fp, fp]
    L.fstObj_free.restype, L.fstObj_free.argtypes = None, [C.c_void_p]
    return L


def ref_rows(L, obj, x, r, lo, hi):
    """-> complex64 [hi - lo + 1][N]; 0 <= lo <= hi <= N/2 (anything else makes the reference write N/2 + 1 rows)"""
    N = 1 << r
    assert 0 <= lo <= hi <= N // 2
    x = np.ascontiguousarray(x, np.float32)
    re, im = np.zeros((hi - lo + 1, N), np.float32), np.zeros((hi - lo + 1, N), np.float32)
    L.fstObj_fst(obj, x.ctypes.data_as(fp), lo, hi, re.ctypes.data_as(fp), im.ctypes.data_as(fp))
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def ref_cells(L, obj, x, r):
    """one row per band, decimated to its distinct columns"""
    N = 1 << r
    out = [ref_rows(L, obj, x, r, f, f)[0, :1] for f in range(3)]
    n = 2
    while n <= N // 4:
        out.append(ref_rows(L, obj, x, r, n + 1, n + 1)[0, ::N // n])
        n *= 2
    return np.concatenate(out)


def case_data(L, c):
    """{key: array} of one case"""
    obj = C.c_void_p(None)
    st = L.fstObj_new(C.byref(obj), c.r)
    assert st == 0 and obj, (c.name, st)
    out, r_ref = {}, []
    for k, x in zip(fc.INPUTS, fc.inputs(c.name)):
        cells = ref_cells(L, obj, x, c.r)
        out[f"{c.name}/{k}/cells"] = cells
        if c.matrix:
            (lo, hi), = c.ranges
            out[f"{c.name}/{k}/matrix"] = ref_rows(L, obj, x, c.r, lo, hi)
        w = fc.cells64(x, c.r)
        r_ref.append(np.abs(cells.astype(np.complex128) - w).max() / np.abs(w).max())
    out[f"{c.name}/ref_vs_f64"] = np.array(r_ref, np.float64)
    L.fstObj_free(obj)
    return out


def main():
    from oracle import ref
    L = bind(ref.lib())
    out = {}
    for c in fc.CASES:
        d = case_data(L, c)
        out.update(d)
        print(f"{c.name}: reference vs float64 {d[c.name + '/ref_vs_f64']}", flush=True)
    np.savez_compressed(fc.GOLDEN, **out)
    print(f"{fc.GOLDEN}: {os.path.getsize(fc.GOLDEN)} bytes")
    assert os.path.getsize(fc.GOLDEN) < 600000


if __name__ == "__main__":
    main()
