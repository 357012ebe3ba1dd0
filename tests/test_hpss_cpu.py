"""CPU-only: the HPSS ABI without a device -- exports, prototypes against the reference header, the wrapper's signature, the
constructor's defaults and refusals, the frame / length arithmetic, slideLength ignored."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.conftest import ROOT

import audioflux_amd as af

REF_HEADER = "/root/reference/src/mir/hpss_algorithm.h"
HAMM, HANN = 2, 1


def _prototypes(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(hpssObj_\w+)\s*\(([^)]*)\)\s*;", src):
        out[name] = (ret, [re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", " *", a.strip())) for a in args.split(",")])
    return out


def test_exports_and_header():
    lib = af.get_lib()
    for name in ("hpssObj_new", "hpssObj_calDataLength", "hpssObj_hpss", "hpssObj_free", "hpssObj_debug", "hpssObj_hpssBatchDevice",
                 "hpssObj_spectraBatchDevice", "afx_medianFilterDevice"):
        assert hasattr(lib, name), name
    ours = _prototypes(os.path.join(ROOT, "include", "mir", "hpss_algorithm.h"))
    assert sorted(ours) == ["hpssObj_calDataLength", "hpssObj_debug", "hpssObj_free", "hpssObj_hpss", "hpssObj_new"]
    text = open(os.path.join(ROOT, "include", "mir", "hpss_algorithm.h")).read()
    assert "IGNORED" in text and "fftLength/4" in text  # the header says what happens to slideLength


@pytest.mark.skipif(not os.path.exists(REF_HEADER), reason="the reference tree is not on this machine")
def test_prototypes_equal_the_reference_header_argument_for_argument():
    assert _prototypes(os.path.join(ROOT, "include", "mir", "hpss_algorithm.h")) == _prototypes(REF_HEADER)


def test_wrapper_signature_and_defaults_are_the_reference_wrappers():
    # python/audioflux/mir/hpss.py: HPSS.__init__(self, radix2_exp=12, window_type=WindowType.HAMM, slide_length=1024, h_order=21,
    # p_order=31); cal_data_length(self, data_length); hpss(self, data_arr)
    sig = inspect.signature(af.HPSS.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("radix2_exp", 12), ("window_type", af.WindowType.HAMM), ("slide_length", 1024), ("h_order", 21), ("p_order", 31)]
    assert list(inspect.signature(af.HPSS.cal_data_length).parameters) == ["self", "data_length"]
    assert list(inspect.signature(af.HPSS.hpss).parameters) == ["self", "data_arr"]
    assert "HPSS" in af.__all__ and int(af.WindowType.HAMM) == HAMM
    for extra in ("hpss_device", "spectra_device"):
        assert list(inspect.signature(getattr(af.HPSS, extra)).parameters)[:3] == ["self", "x", "stream"]


def _plan(radix2_exp, window=None, slide=None, h=None, p=None, n=0):
    fn = af.get_lib().afx_test_hpss_plan
    fn.restype = C.c_int
    ip = C.POINTER(C.c_int)
    fn.argtypes = [C.c_int, ip, ip, ip, ip, C.c_int, ip]
    out = (C.c_int * 7)()
    opt = lambda v: None if v is None else C.byref(C.c_int(v))  # noqa: E731
    st = fn(radix2_exp, opt(window), opt(slide), opt(h), opt(p), n, out)
    assert st == out[0]
    return dict(zip(("status", "window", "hop", "h", "p", "frames", "length"), out))


def test_constructor_defaults():
    d = _plan(11)
    assert (d["status"], d["window"], d["hop"], d["h"], d["p"]) == (0, HAMM, 512, 21, 31)  # Hamm, not stftObj_new's Rect
    assert _plan(10, window=HANN)["window"] == HANN
    for bad in (0, -5, 20, 64 - 2):  # <= 0 or even: the defaults
        d = _plan(10, h=bad, p=bad)
        assert (d["h"], d["p"]) == (21, 31), bad
    d = _plan(10, h=1, p=63)
    assert (d["status"], d["h"], d["p"]) == (0, 1, 63)


@pytest.mark.parametrize("slide", [None, 1, 100, 512, 4096, -7])
def test_slide_length_is_ignored(slide):
    for r in (8, 11, 12):
        d = _plan(r, slide=slide, n=5 << r)
        assert d["hop"] == (1 << r) // 4 and d["frames"] == 17 and d["length"] == 5 << r


def test_refusals_need_no_device():
    lib = af.get_lib()
    fn = lib.hpssObj_new
    fn.restype = C.c_int
    ip = C.POINTER(C.c_int)
    fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, ip, ip, ip, ip]
    for r in (-1, 0, 1, 15, 31):
        obj = C.c_void_p(0x1234)
        assert fn(C.byref(obj), r, None, None, None, None) == -100 and not obj, r
    for h, p in ((65, 31), (21, 255), (1001, 1001)):
        obj = C.c_void_p(0x1234)
        assert fn(C.byref(obj), 11, None, None, C.byref(C.c_int(h)), C.byref(C.c_int(p))) == -4 and not obj
        assert "odd orders up to 63" in af.last_error()
    assert fn(None, 11, None, None, None, None) == -1
    # NULL object: the void call is counted, the int calls answer
    lib.hpssObj_calDataLength.restype = C.c_int
    lib.hpssObj_calDataLength.argtypes = [C.c_void_p, C.c_int]
    assert lib.hpssObj_calDataLength(None, 4096) == 0
    before = lib.afx_error_count()
    lib.hpssObj_hpss.restype = None
    lib.hpssObj_hpss.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2
    lib.hpssObj_hpss(None, None, 0, None, None)
    assert lib.afx_error_count() == before + 1 and "NULL object" in af.last_error()
    lib.hpssObj_free.restype = None
    lib.hpssObj_free.argtypes = [C.c_void_p]
    lib.hpssObj_free(None)
    lib.hpssObj_hpssBatchDevice.restype = C.c_int
    lib.hpssObj_hpssBatchDevice.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 2 + [C.c_longlong, C.c_void_p]
    assert lib.hpssObj_hpssBatchDevice(None, None, 1, 1, 1, None, None, 1, None) == -6
    lib.afx_medianFilterDevice.restype = C.c_int
    lib.afx_medianFilterDevice.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.afx_medianFilterDevice(None, 4, 4, 0, 0, 3, None, None) == -6
    for order in (2, 0, 257):
        assert lib.afx_medianFilterDevice(0x1000, 4, 4, 0, 0, order, 0x2000, None) == -4


@pytest.mark.parametrize("r,n,frames,length", [
    (10, 1023, 0, 768), (10, 1024, 1, 1024), (10, 1279, 1, 1024), (10, 1280, 2, 1280), (10, 1024 + 256 * 33 + 77, 34, 1024 + 256 * 33),
    (11, 480000, 934, 2048 + 512 * 933), (12, 480000, 465, 4096 + 1024 * 464), (2, 4, 1, 4), (2, 9, 6, 9), (14, 16384 * 3, 9, 16384 * 3)])
def test_frame_and_length_table(r, n, frames, length):
    # T = (n - N) / hop + 1, 0 below N; calDataLength = (T - 1) hop + N by the reference's arithmetic (3 N / 4 at T = 0)
    d = _plan(r, n=n)
    assert (d["status"], d["frames"], d["length"]) == (0, frames, length)


def test_restatement_median_is_the_sorted_window():
    """the float64 statement the other tests lean on, against a loop that sorts every zero-padded window"""
    import numpy as np
    from tests.hpss_restate import median_filter
    rng = np.random.default_rng(3)
    a = rng.standard_normal((9, 7)).astype(np.float32)
    for order in (1, 3, 5, 11):
        h = order // 2
        for axis in (0, 1):
            want = np.zeros_like(a)
            for i in range(9):
                for j in range(7):
                    idx = [(i + d, j) if axis == 0 else (i, j + d) for d in range(-h, h + 1)]
                    win = sorted(float(a[p]) if 0 <= p[0] < 9 and 0 <= p[1] < 7 else 0.0 for p in idx)
                    want[i, j] = win[h]
            assert np.array_equal(median_filter(a, axis, order), want), (order, axis)
    two = median_filter(np.concatenate([a, a]), 0, 5, frames_per_clip=9)
    assert np.array_equal(two[:9], median_filter(a, 0, 5)) and np.array_equal(two[9:], two[:9])
