#!/usr/bin/env python3
"""Writes tests/golden/nsgt.npz: what the compiled reference gives for every row of tests/nsgt_cases.py, by raw ctypes
through the reference driver's lib().  Per case: the plan getters (lengths, fre, bin, max, total), nsgt_filterBank's windows
and offsets; per case and input: the cell data, and the matrix where num * maxLength <= 20000.

A plan with a band longer than the chunk makes the reference write past its scratch (it aborts in glibc): before the
reference sees a configuration, the library's device-free plan (afx_nsgt_plan_host) must have accepted it.

    python tests/golden/make_nsgt_golden.py        (needs the compiled reference)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import nsgt_cases as nc  # noqa: E402

ip, fp = nc.ip, nc.fp


def bind(L):
    L.nsgtObj_new.restype = C.c_int
    L.nsgtObj_new.argtypes = [C.POINTER(C.c_void_p)] + nc.NEW_ARGTYPES
    for name, res in (("nsgtObj_getMaxTimeLength", C.c_int), ("nsgtObj_getTotalTimeLength", C.c_int),
                      ("nsgtObj_getTimeLengthArr", ip), ("nsgtObj_getFreBandArr", fp), ("nsgtObj_getBinBandArr", ip)):
        f = getattr(L, name)
        f.restype, f.argtypes = res, [C.c_void_p]
    L.nsgtObj_setMinLength.restype, L.nsgtObj_setMinLength.argtypes = None, [C.c_void_p, C.c_int]
    L.nsgtObj_nsgt.restype, L.nsgtObj_nsgt.argtypes = None, [C.c_void_p, fp, fp, fp]
    L.nsgtObj_getCellData.restype, L.nsgtObj_getCellData.argtypes = None, [C.c_void_p, C.POINTER(fp), C.POINTER(fp)]
    L.nsgtObj_free.restype, L.nsgtObj_free.argtypes = None, [C.c_void_p]
    return L


def safe(c, min_len=None):
    """the library's own plan accepts the configuration: no band longer than the chunk"""
    import audioflux_amd as af
    st, _ = nc.plan_host(af.get_lib(), c, min_len)
    return st == 0


def getters(L, obj, num):
    return dict(len=np.ctypeslib.as_array(L.nsgtObj_getTimeLengthArr(obj), (num,)).copy(),
                fre=np.ctypeslib.as_array(L.nsgtObj_getFreBandArr(obj), (num,)).copy(),
                bin=np.ctypeslib.as_array(L.nsgtObj_getBinBandArr(obj), (num,)).copy(),
                max=L.nsgtObj_getMaxTimeLength(obj), total=L.nsgtObj_getTotalTimeLength(obj))


def ref_new(L, c, min_len=None):
    assert safe(c, min_len), f"{c.name}: a band longer than the chunk -- the reference must not see this plan"
    obj = C.c_void_p(None)
    st = L.nsgtObj_new(C.byref(obj), c.num, c.r, *nc.new_args(c, min_len))
    return st, obj


def ref_transform(L, obj, x, num, mx, total):
    """-> (cells complex64 [total], matrix complex64 [num][max])"""
    x = np.ascontiguousarray(x, np.float32)
    re, im = np.zeros((num, mx), np.float32), np.zeros((num, mx), np.float32)
    L.nsgtObj_nsgt(obj, x.ctypes.data_as(fp), re.ctypes.data_as(fp), im.ctypes.data_as(fp))
    cr, ci = fp(), fp()
    L.nsgtObj_getCellData(obj, C.byref(cr), C.byref(ci))
    cells = np.ctypeslib.as_array(cr, (total,)) + 1j * np.ctypeslib.as_array(ci, (total,))
    return cells.astype(np.complex64), (re + 1j * im).astype(np.complex64)


def ref_filter_bank(L, c, min_len=None):
    """nsgt_filterBank with the parameters nsgtObj_new resolves (tests/nsgt_cases.py: resolve; style / normal substitutions of
    nsgt_algorithm.c:137-149) -> dict(len, fre, bin, offset, window, max, total)"""
    assert safe(c, min_len), f"{c.name}: a band longer than the chunk -- the reference must not see this plan"
    low, high = nc.resolve(c)
    style = nc.STYLE["Hann"] if c.style == "Gammatone" else nc.STYLE[c.style]
    normal = nc.NORMAL["BandWidth"] if c.normal == "Area" else nc.NORMAL[c.normal]
    fn = L.nsgt_filterBank
    fn.restype = None
    fn.argtypes = [C.c_int] * 8 + [C.c_float, C.c_float, C.c_int, C.POINTER(fp), ip, fp, ip, ip, ip, ip]
    ln, bn, off = (np.zeros(c.num, np.int32) for _ in range(3))
    fre = np.zeros(c.num, np.float32)
    win, mx, tot = fp(), C.c_int(0), C.c_int(0)
    fn(c.num, 1 << c.r, c.sr, c.min_len if min_len is None else min_len, c.bank, nc.SCALE[c.scale], style, normal, float(low),
       float(high), c.bpo, C.byref(win), ln.ctypes.data_as(ip), fre.ctypes.data_as(fp), bn.ctypes.data_as(ip),
       off.ctypes.data_as(ip), C.byref(mx), C.byref(tot))
    window = np.ctypeslib.as_array(win, (tot.value,)).copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(win)
    return dict(len=ln, fre=fre, bin=bn, offset=off, window=window, max=mx.value, total=tot.value)


def main():
    from oracle import ref
    L = bind(ref.lib())
    out = {}
    for c in nc.CASES:
        st, obj = ref_new(L, c)
        assert st == 0 and obj, (c.name, st)
        g = getters(L, obj, c.num)
        fb = ref_filter_bank(L, c)
        for k in ("len", "fre", "bin"):  # the resolution of tests/nsgt_cases.py is the constructor's
            assert np.array_equal(fb[k].view(np.int32), g[k].view(np.int32)), (c.name, k)
        assert fb["max"] == g["max"] and fb["total"] == g["total"], c.name
        for k in ("len", "fre", "bin"):
            out[f"{c.name}/{k}"] = g[k]
        out[f"{c.name}/max_total"] = np.array([g["max"], g["total"]], np.int32)
        out[f"{c.name}/offset"] = fb["offset"]
        out[f"{c.name}/window"] = fb["window"]
        x = nc.inputs(c.name)
        for k, name in enumerate(nc.INPUTS):
            cells, mat = ref_transform(L, obj, x[k], c.num, g["max"], g["total"])
            out[f"{c.name}/{name}/cells"] = cells
            if c.num * g["max"] <= nc.MATRIX_LIMIT:
                out[f"{c.name}/{name}/matrix"] = mat
        L.nsgtObj_free(obj)
        print(f"{c.name}: lengths {g['len'].min()} ... {g['len'].max()}, {len(set(g['len'].tolist()))} distinct, total {g['total']}, "
              f"offsets {fb['offset'].min()} ... {fb['offset'].max()}", flush=True)
    np.savez_compressed(nc.GOLDEN, **out)
    print(f"{nc.GOLDEN}: {os.path.getsize(nc.GOLDEN)} bytes")
    assert os.path.getsize(nc.GOLDEN) < 1000000


if __name__ == "__main__":
    main()
