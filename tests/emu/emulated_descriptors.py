#!/usr/bin/env python3
"""The descriptor kernels (afx_descriptors.hip: k_desc_rows / _wide / _long, k_desc_frames) as emulated device code, through
the C host object (spectralObj_new / setEdge / setEdgeArr / computeDevice and the legacy calls), against
tests/golden/spectral.npz by the acceptance rule of the GPU tests (tests/spectral_check.py).  Also: a
full request list equals the single requests bitwise, clips of a batch equal per-clip calls bitwise.
AFX_LIB = the library tests/test_spectral_emulated.py builds.  Arguments: input names (default: all)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import spectral_cases as sc  # noqa: E402
from tests.spectral_check import check_output  # noqa: E402
from tests.spectral_ref import bind, calloc_ints, fp  # noqa: E402

lib = C.CDLL(os.environ["AFX_LIB"])
bind(lib)


class Req(C.Structure):  # AfxSpectralRequest, include/afx_batch.h
    _fields_ = [("kind", C.c_int), ("iarg", C.c_int * 4), ("farg", C.c_float * 2)]


lib.spectralObj_computeDevice.restype = C.c_int
lib.spectralObj_computeDevice.argtypes = [C.c_void_p, fp, fp, C.c_longlong, C.c_int, C.POINTER(Req), C.c_int, fp, C.c_longlong,
                                          C.c_void_p]
lib.afx_spectralSlots.restype = C.c_int
lib.afx_spectralSlots.argtypes = [C.POINTER(Req), C.c_int]


def requests(names):
    arr = (Req * len(names))()
    for r, n in zip(arr, names):
        k, i, f = sc.request_tuple(n)
        r.kind, r.iarg[:], r.farg[:] = k, i, f
    return arr


def new_object(num, fre, edge):
    obj = C.c_void_p()
    assert lib.spectralObj_new(C.byref(obj), num, fre.ctypes.data_as(fp)) == 0
    if isinstance(edge, tuple):
        lib.spectralObj_setEdge(obj, *edge)
    elif edge is not None:
        lib.spectralObj_setEdgeArr(obj, calloc_ints(edge), len(edge))
    return obj


def compute(obj, spec, phase, names, frames_per_clip=0):
    req = requests(names)
    slots = lib.afx_spectralSlots(req, len(names))
    rows = spec.shape[0]
    out = np.full((slots, rows), np.nan, np.float32)
    st = lib.spectralObj_computeDevice(obj, spec.ctypes.data_as(fp), phase.ctypes.data_as(fp) if phase is not None else None, rows,
                                       frames_per_clip, req, len(names), out.ctypes.data_as(fp), rows, None)
    assert st == 0, st
    return out


def check(what, kind, case, got, want, spec, phase, fre, idx, num, second):
    """one output vector against the fixture by the rule of the GPU tests; returns the peak-relative error"""
    check_output(what, case, got, want, spec, phase, fre, idx, num, second=second)
    ok = ~np.isnan(want)
    peak = np.abs(want[ok]).max() if ok.any() else 0.0
    if peak == 0 or kind == "max" or kind in sc.DISCRETE or (kind == "novelty" and sc.PARAMS[case][1][2] == 1):
        return 0.0
    return float(np.abs(got[ok].astype(np.float64) - want[ok]).max() / peak)


def main(argv):
    gold = np.load(os.path.join(sc.GOLDEN, "spectral.npz"))
    ins = sc.inputs()
    checked = 0
    for iname in (argv or list(ins)):
        spec, phase, fre = ins[iname]
        num = spec.shape[1]
        for ename, edge in sc.edges(num).items():
            idx = sc.edge_indices(num, edge)
            names = sc.names_for(phase)
            obj = new_object(num, fre, edge)
            # one request per kind and pass: the cases in two lists (defaults, then the non-default parameter sets)
            first = [n for n in names if n == sc.PARAMS[n][0]]
            rest = [n for n in names if n not in first]
            worst, worst_at = 0.0, ""
            for group in (first, rest):
                out = compute(obj, spec, phase, group)
                slot = 0
                for case in group:
                    kind = sc.PARAMS[case][0]
                    key = f"{iname}/{ename}/{case}"
                    e = check(key, kind, case, out[slot], gold[key], spec, phase, fre, idx, num, False)
                    if kind in sc.TWO_SLOT:
                        e = max(e, check(key + "/fre", kind, case, out[slot + 1], gold[key + "/fre"], spec, phase, fre, idx, num, True))
                    slot += 2 if kind in sc.TWO_SLOT else 1
                    checked += 1
                    if e > worst:
                        worst, worst_at = e, case
                assert slot == out.shape[0]
            # the whole list in one call (kinds repeat: extra passes) == single requests, bitwise
            if iname in ("bark64_mag", "linear257"):
                whole = compute(obj, spec, phase, names)
                slot = 0
                for case in names:
                    n = 2 if sc.PARAMS[case][0] in sc.TWO_SLOT else 1
                    single = compute(obj, spec, phase, [case])
                    assert np.array_equal(whole[slot:slot + n].view(np.uint32), single.view(np.uint32)), f"{iname}/{ename}/{case}: list != single"
                    slot += n
            lib.spectralObj_free(obj)
            print(f"descriptors {iname} [{spec.shape[0]}, {num}] edge {ename}: {len(names)} cases, worst {worst:.2e} of the peak ({worst_at})", flush=True)
    # the legacy host-pointer call and clips
    spec, phase, fre = ins["bark64_mag"]
    num = spec.shape[1]
    obj = new_object(num, fre, None)
    lib.spectralObj_setTimeLength(obj, spec.shape[0])
    got = np.zeros(spec.shape[0], np.float32)
    lib.spectralObj_centroid(obj, spec.ctypes.data_as(fp), got.ctypes.data_as(fp))
    assert np.abs(got - gold["bark64_mag/full/centroid"]).max() <= 1e-5 * np.abs(gold["bark64_mag/full/centroid"]).max()
    clips, frames = 3, 14
    batch = np.ascontiguousarray(spec[:clips * frames])
    frame_cases = ["flux_s2_p2_pos_exp_mean", "sd", "sf_s5_pos", "mkl", "broadband", "novelty"]
    whole = compute(obj, batch, None, frame_cases, frames_per_clip=frames)
    for c in range(clips):
        one = compute(obj, np.ascontiguousarray(batch[c * frames:(c + 1) * frames]), None, frame_cases)
        assert np.array_equal(whole[:, c * frames:(c + 1) * frames].view(np.uint32), one.view(np.uint32)), f"clip {c}"
    lib.spectralObj_free(obj)
    print(f"legacy call and {clips} clips x {frames} frames: bitwise equal to per-clip calls", flush=True)
    print(f"{checked} cases")
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
