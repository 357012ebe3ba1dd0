#!/usr/bin/env python3
"""Writes tests/golden/pitch_yin.npz: the outputs of the compiled reference's pitchYINObj_pitch / pitchYINObj_getTroughData
(oracle.ref.lib()) for the cases of tests/pitch_cases.py, plus the float64 curve of tests/pitch_restate.py.  Inputs are
regenerated from seeds; only outputs are stored.
Keys: <case>/fre, /trough (NaN where the reference left the entry alone), /min, /len, /cand_fre, /cand_val [T, mLen], /yin64.

    python tests/golden/make_pitch_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import pitch_cases as pc  # noqa: E402
from tests import pitch_restate as pr  # noqa: E402

fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


def bind(lib):
    lib.pitchYINObj_new.restype = C.c_int
    lib.pitchYINObj_new.argtypes = [C.POINTER(C.c_void_p), ip, fp, fp, ip, ip, ip, ip]
    lib.pitchYINObj_setThresh.restype = None
    lib.pitchYINObj_setThresh.argtypes = [C.c_void_p, C.c_float]
    lib.pitchYINObj_calTimeLength.restype = C.c_int
    lib.pitchYINObj_calTimeLength.argtypes = [C.c_void_p, C.c_int]
    lib.pitchYINObj_pitch.restype = None
    lib.pitchYINObj_pitch.argtypes = [C.c_void_p, fp, C.c_int, fp, fp, fp]
    lib.pitchYINObj_getTroughData.restype = C.c_int
    lib.pitchYINObj_getTroughData.argtypes = [C.c_void_p, C.POINTER(fp), C.POINTER(fp), C.POINTER(ip)]
    lib.pitchYINObj_free.restype = None
    lib.pitchYINObj_free.argtypes = [C.c_void_p]


def new(lib, sr, lo, hi, r, hop, auto, cont=0):
    obj = C.c_void_p()
    st = lib.pitchYINObj_new(C.byref(obj), C.byref(C.c_int(sr)), C.byref(C.c_float(lo)), C.byref(C.c_float(hi)), C.byref(C.c_int(r)),
                             C.byref(C.c_int(hop)), C.byref(C.c_int(auto)), C.byref(C.c_int(cont)))
    return st, obj


def call(lib, obj, x, fill=np.nan):
    """one pitchYINObj_pitch call on an existing object -> fre, trough (entries the call left alone keep `fill`), min, and the
    candidate lists (len, fre [T, mLen], val [T, mLen]; entries behind a frame's count zeroed)"""
    x = np.ascontiguousarray(x, np.float32)
    T = lib.pitchYINObj_calTimeLength(obj, len(x))
    fre, val, mn = (np.full(T, fill, np.float32) for _ in range(3))
    lib.pitchYINObj_pitch(obj, x.ctypes.data_as(fp), len(x), fre.ctypes.data_as(fp), val.ctypes.data_as(fp), mn.ctypes.data_as(fp))
    f, v, ln = fp(), fp(), ip()
    mlen = lib.pitchYINObj_getTroughData(obj, C.byref(f), C.byref(v), C.byref(ln))
    if T == 0:
        return fre, val, mn, np.zeros(0, np.int32), np.zeros((0, mlen), np.float32), np.zeros((0, mlen), np.float32)
    lens = np.ctypeslib.as_array(ln, (T,)).copy()
    cf = np.ctypeslib.as_array(f, (T, mlen)).copy()
    cv = np.ctypeslib.as_array(v, (T, mlen)).copy()
    for t in range(T):
        cf[t, lens[t]:] = 0
        cv[t, lens[t]:] = 0
    return fre, val, mn, lens, cf, cv


def run(lib, x, sr, lo, hi, r, hop, auto, thresh):
    st, obj = new(lib, sr, lo, hi, r, hop, auto)
    assert st == 0 and obj, st
    lib.pitchYINObj_setThresh(obj, thresh)
    out = call(lib, obj, x)
    lib.pitchYINObj_free(obj)
    return out


def main():
    from oracle import ref
    lib = ref.lib()
    bind(lib)
    out = {}
    for name, (sr, lo, hi, r, hop, auto, thresh, kind, n) in pc.CASES.items():
        x = pc.case_input(name)
        fre, val, mn, lens, cf, cv = run(lib, x, sr, lo, hi, r, hop, auto, thresh)
        mi, ma, ylen, mlen = pc.plan(sr, lo, hi, r, hop, auto)
        frames = pr.pitch(x, sr, r, hop, auto, mi, ma, thresh)
        width = max(int(lens.max()) if len(lens) else 0, 1)
        out[name + "/fre"], out[name + "/trough"], out[name + "/min"] = fre, val, mn
        out[name + "/len"], out[name + "/cand_fre"], out[name + "/cand_val"] = lens.astype(np.int32), cf[:, :width], cv[:, :width]
        out[name + "/yin64"] = np.array([f["yin"] for f in frames], np.float32)
        print(f"{name}: {len(fre)} frames, {int(np.isfinite(fre).sum())} voiced, most candidates {width}")
    path = os.path.join(ROOT, "tests", "golden", "pitch_yin.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
