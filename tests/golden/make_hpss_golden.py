#!/usr/bin/env python3
"""Writes tests/golden/hpss.npz: hArr / pArr of the compiled reference's hpssObj_hpss (oracle.ref.lib()) for the cases of
tests/hpss_cases.py.  Inputs are regenerated from seeds; only the outputs are stored.
Key: <case>/h, <case>/p.

    python tests/golden/make_hpss_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref  # noqa: E402
from tests import hpss_cases as hc  # noqa: E402

fp = C.POINTER(C.c_float)


def bind(lib):
    lib.hpssObj_new.restype = C.c_int
    lib.hpssObj_new.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_int)]
    lib.hpssObj_calDataLength.restype = C.c_int
    lib.hpssObj_calDataLength.argtypes = [C.c_void_p, C.c_int]
    lib.hpssObj_hpss.restype = None
    lib.hpssObj_hpss.argtypes = [C.c_void_p, fp, C.c_int, fp, fp]
    lib.hpssObj_free.restype = None
    lib.hpssObj_free.argtypes = [C.c_void_p]


def run(lib, x, r, w, h, p, outs="hp", init_h=None, init_p=None):
    """one hpssObj_hpss call of `lib` (the reference or the product: same prototypes) -> (h or None, p or None)"""
    obj = C.c_void_p()
    st = lib.hpssObj_new(C.byref(obj), r, C.byref(C.c_int(w)), C.byref(C.c_int(1 << r)), C.byref(C.c_int(h)), C.byref(C.c_int(p)))
    assert st == 0 and obj, st
    n = lib.hpssObj_calDataLength(obj, len(x))
    ha = np.zeros(n, np.float32) if init_h is None else np.array(init_h, np.float32)
    pa = np.zeros(n, np.float32) if init_p is None else np.array(init_p, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    lib.hpssObj_hpss(obj, x.ctypes.data_as(fp), len(x), ha.ctypes.data_as(fp) if "h" in outs else None,
                     pa.ctypes.data_as(fp) if "p" in outs else None)
    lib.hpssObj_free(obj)
    return (ha if "h" in outs else None), (pa if "p" in outs else None)


def main():
    lib = ref.lib()
    bind(lib)
    out = {}
    for name, (r, w, h, p, kind, n, outs, init) in hc.CASES.items():
        x = hc.case_input(name)
        ha, pa = run(lib, x, r, w, h, p, outs, hc.initial(name, "h"), hc.initial(name, "p"))
        if ha is not None:
            out[name + "/h"] = ha
        if pa is not None:
            out[name + "/p"] = pa
    path = os.path.join(ROOT, "tests", "golden", "hpss.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} vectors -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
