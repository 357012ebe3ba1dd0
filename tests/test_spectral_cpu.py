"""CPU-only: the C ABI of the spectral-descriptor family -- every function the new / extended headers declare is exported and
callable with the argument list of its header, no object without a device, slot counting and argument validation -- and the
float64 restatement pinned to the fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audioflux_amd as af
from audioflux_amd.spectral import KINDS, SpectralRequest, request
from tests import spectral_cases as sc
from tests import spectral_restate as sr
from tests.conftest import ROOT

AFX_ERR_ARG = -6
C_TYPES = {"int": C.c_int, "float": C.c_float, "long long": C.c_longlong}


def prototypes(header, prefix):
    """name -> list of C parameter declarations, from the header text"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*(int|void)\s+(" + prefix + r"_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S):
        out[name] = (ret, [" ".join(a.split()) for a in args.split(",")])
    return out


def ctype_of(decl):
    if "*" in decl:
        return C.c_void_p
    for k, v in C_TYPES.items():
        if decl.startswith(k + " ") or decl.startswith("const " + k + " "):
            return v
    return C.c_int  # enums, by value


def test_every_declared_descriptor_function_is_exported_with_its_header_arity():
    lib = af.get_lib()
    spectral = prototypes("feature/spectral_algorithm.h", "spectralObj")
    assert len(spectral) == 35, sorted(spectral)
    gram = {n: p for n, p in prototypes("spectrogram_algorithm.h", "spectrogramObj").items()
            if n.split("_", 1)[1] in {"setEdge", "setEdgeArr", "preprocess"} | {n2.split("_", 1)[1] for n2 in spectral}}
    gram = {n: p for n, p in gram.items() if n not in ("spectrogramObj_new", "spectrogramObj_free", "spectrogramObj_setTimeLength")}
    assert len(gram) == 33, sorted(gram)
    for name, (ret, args) in {**spectral, **gram}.items():
        assert hasattr(lib, name), name
        # the spectrogram object's descriptor takes what the descriptor object's takes behind the object pointer
        twin = "spectralObj_" + name.split("_", 1)[1]
        if name.startswith("spectrogramObj_") and twin in spectral:
            assert [ctype_of(a) for a in args[1:]] == [ctype_of(a) for a in spectral[twin][1][1:]], name
    # NULL-object calls through ctypes with the header's argument list: they return (void entry points record the failure)
    before = lib.afx_error_count()
    for name, (ret, args) in {**spectral, **gram}.items():
        if name in ("spectralObj_new", "spectralObj_setEdgeArr", "spectrogramObj_setEdgeArr"):
            continue
        fn = getattr(lib, name)
        fn.restype = None if ret == "void" else C.c_int
        fn.argtypes = [ctype_of(a) for a in args]
        fn(*[None if t is C.c_void_p else t(0) for t in fn.argtypes])
    assert lib.afx_error_count() > before
    hdr = open(os.path.join(ROOT, "include", "flux_base.h")).read()
    for name, val in (("SpectralNoveltyMethod_Sub", 0), ("SpectralNoveltyMethod_Entroy", 1), ("SpectralNoveltyMethod_KL", 2),
                      ("SpectralNoveltyMethod_IS", 3), ("SpectralNoveltyData_Value", 0), ("SpectralNoveltyData_Number", 1)):
        assert re.search(rf"{name}\s*=\s*{val}\b", hdr), name
    assert af.SpectralNoveltyMethodType.IS == 3 and af.SpectralNoveltyDataType.NUMBER == 1


def test_kind_numbers_are_the_header_enum():
    src = open(os.path.join(ROOT, "include", "afx_batch.h")).read()
    body = re.search(r"typedef enum \{ (AFX_SD_FLATNESS.*?) \} AfxSpectralKind;", src, flags=re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.replace("\n", " ").split(",")]
    assert names == ["AFX_SD_" + k.upper() for k in KINDS] + ["AFX_SD_COUNT"]
    assert list(KINDS) == sc.KINDS


def test_no_descriptor_object_without_a_device():
    if af.runtime_status() == 0:
        pytest.skip("a device is present")
    lib = af.get_lib()
    obj = C.c_void_p()
    fre = (C.c_float * 4)(1, 2, 3, 4)
    lib.spectralObj_new.restype = C.c_int
    lib.spectralObj_new.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_float)]
    assert lib.spectralObj_new(C.byref(obj), 4, fre) <= -2 and not obj
    assert lib.spectralObj_new(C.byref(obj), 1, fre) == -1  # "num is error!!!"
    with pytest.raises(RuntimeError):
        af.Spectral(4, [1, 2, 3, 4])


def test_slots_and_argument_validation():
    lib = af.get_lib()
    lib.afx_spectralSlots.restype = C.c_int
    lib.afx_spectralSlots.argtypes = [C.POINTER(SpectralRequest), C.c_int]
    every = (SpectralRequest * len(KINDS))(*[request(k) for k in KINDS])
    assert lib.afx_spectralSlots(every, len(KINDS)) == 33
    assert lib.afx_spectralSlots(every, 3) == 3
    two = (SpectralRequest * 2)(request("max"), request("var"))
    assert lib.afx_spectralSlots(two, 2) == 4
    assert lib.afx_spectralSlots(every, 0) == AFX_ERR_ARG and lib.afx_spectralSlots(None, 2) == AFX_ERR_ARG
    bad = (SpectralRequest * 1)(request(30))
    assert lib.afx_spectralSlots(bad, 1) == AFX_ERR_ARG
    fn = lib.spectralObj_computeDevice
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.POINTER(SpectralRequest), C.c_int, C.c_void_p,
                   C.c_longlong, C.c_void_p]
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for req, count, what in ((every, 0, "count"), (bad, 1, "kind"), ((SpectralRequest * 1)(request("pd")), 1, "dPhase")):
        assert fn(None, p, None, 4, 0, req, count, p, 4, None) == AFX_ERR_ARG
        assert what in af.last_error(), (what, af.last_error())


def test_float64_restatement_is_pinned_to_the_fixture():
    """the third opinion agrees with the compiled reference's vectors: to 1e-4 of the peak for the float32 sums (the
    reference's own rounding), exactly for the maximum, on all but threshold frames for the discrete outputs"""
    gold = np.load(os.path.join(sc.GOLDEN, "spectral.npz"))
    for iname, (spec, phase, fre) in sc.inputs().items():
        num = spec.shape[1]
        for ename, edge in sc.edges(num).items():
            idx = sc.edge_indices(num, edge)
            for case in sc.names_for(phase):
                kind, iarg, farg = sc.PARAMS[case]
                outs = sr.restate(kind, iarg, farg, spec, phase, fre, idx, num)
                for k, o in enumerate(outs):
                    want = gold[f"{iname}/{ename}/{case}" + ("/fre" if k else "")]
                    what = f"{iname}/{ename}/{case}[{k}]"
                    ok = ~np.isnan(want)
                    assert np.array_equal(np.isnan(o), ~ok), what
                    if kind in sc.DISCRETE or (kind == "novelty" and iarg[2] == 1):
                        bad = o != want
                        if bad.any():
                            assert np.all(sr.margin(kind, iarg, farg, spec, idx)[bad] <= 1e-4), what
                        continue
                    peak = np.abs(want[ok]).max()
                    tol = 2e-3 if kind in sc.CANCELLING or kind in ("kurtosis", "novelty") else 1e-4
                    assert np.abs(o[ok] - want[ok]).max() <= tol * max(peak, 1e-30), (what, np.abs(o[ok] - want[ok]).max() / peak)


def test_wrapper_signatures_are_the_reference_wrappers():
    """names and defaults of the two reference wrappers, which differ: Spectral.flux(is_exp=False) / broadband(threshold=0),
    the spectrogram classes flux(is_no_exp=True) (handed to the C isExp argument) / broadband(threshold)"""
    import inspect
    sig = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]  # noqa: E731
    E = inspect.Parameter.empty
    assert sig(af.Spectral.flux) == [("m_data_arr", E), ("step", 1), ("p", 2), ("is_positive", False), ("is_exp", False), ("tp", 0)]
    assert sig(af.SpectrogramBase.flux) == [("m_data_arr", E), ("step", 1), ("p", 2), ("is_positive", False), ("is_no_exp", True), ("tp", 0)]
    assert sig(af.Spectral.broadband) == [("m_data_arr", E), ("threshold", 0)]
    assert sig(af.SpectrogramBase.broadband) == [("m_data_arr", E), ("threshold", E)]
    for cls in (af.Spectral, af.SpectrogramBase, af.MelSpectrogram):
        assert sig(cls.rolloff) == [("m_data_arr", E), ("threshold", 0.95)]
        assert sig(cls.band_width) == [("m_data_arr", E), ("p", 2)]
        assert sig(cls.energy) == [("m_data_arr", E), ("is_log", False), ("gamma", 10.0)]
        assert sig(cls.eer) == [("m_data_arr", E), ("is_norm", False), ("gamma", 1.0)]
        assert sig(cls.sd) == sig(cls.sf) == [("m_data_arr", E), ("step", 1), ("is_positive", False)]
        assert sig(cls.pd) == sig(cls.rcd) == [("m_data_arr", E), ("m_phase_arr", E)]
        assert [n for n, _ in sig(cls.novelty)] == ["m_data_arr", "step", "threshold", "method_type", "data_type"]
