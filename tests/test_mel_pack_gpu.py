"""GPU: the packed band plan of k_stft_mel_v2 (afx_bandplan.c: afx_bandpack_build; afx_melparts.h: band_stage3) against the plan as
it came, built in the same process with AFX_MEL_NOPACK=1 (read at plan creation), through the plan layer itself
(afxk_melfused_create / _run): afxk_melfused_pack says which of the two a plan is.

The packed plan runs 48 tap slots per lane where the (48, 16) variant runs 64; a row's multiply-adds and their order do not
change with the partitions that hold it, so every comparison is for equality of bits.  3 clips x 301 frames with AFX_MEL_CUS=1
(read per launch): one workgroup's waves claim 32- and 16-frame runs, then 4-frame runs and a clamped last one, across clip
boundaries.  Routes: mel-128 + MFCC-13 in one launch, complex results, the temporal instantiation; hops 256 / 512 / 1024."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from oracle import restate
from tests import cases
from tests.test_bandplan import Band

pytestmark = pytest.mark.gpu
HOPS = [256, 512, 1024]
FRAMES, CLIPS, NUM, CC = 301, 3, 128, 13
vp, fp = C.c_void_p, C.POINTER(C.c_float)


class Args(C.Structure):  # AfxMelFusedArgs, audioflux_amd/csrc/hip/afx_device.h
    _fields_ = [("x", vp), ("clipStride", C.c_longlong), ("batch", C.c_int), ("dataLength", C.c_int), ("timeLength", C.c_int),
                ("hop", C.c_int), ("specMap", C.c_int), ("postPow", C.c_int), ("normValue", C.c_float), ("out", vp), ("outIm", vp),
                ("dct", vp), ("ccNum", C.c_int), ("ccRectify", C.c_int), ("cc", vp), ("energy", vp), ("rms", vp), ("zcr", vp)]


def library():
    lib = af.get_lib()
    lib.afxk_melfused_create.argtypes = [C.POINTER(vp), C.c_int, fp, C.POINTER(Band), vp]
    lib.afxk_melfused_run.argtypes = [vp, C.POINTER(Args), vp]
    lib.afxk_melfused_destroy.argtypes = [vp]
    lib.afxk_melfused_destroy.restype = None
    lib.afxk_melfused_pack.argtypes = [vp]
    lib.afxk_melfused_kind.argtypes = [vp]
    return lib


@pytest.fixture(scope="module")
def plans():
    """(packed plan, plan as it came) of mel-128 at 16 kHz, n_fft 2048, with the DCT-II operand on the device"""
    import os
    import torch
    lib = library()
    assert lib.afxdev_ensure() == 0, af.last_error()
    bank, _, _ = restate.mel_bank(NUM, 2048, 16000, 0.0, 8000.0)
    band = Band()
    assert lib.afx_bandplan_build(bank.ctypes.data_as(fp), NUM, 1025, C.byref(band)) == 0
    window = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2048) / 2048)).astype(np.float32)
    made = []
    saved = os.environ.pop("AFX_MEL_NOPACK", None)
    try:
        for nopack in (False, True):
            if nopack:
                os.environ["AFX_MEL_NOPACK"] = "1"
            plan = vp()
            st = lib.afxk_melfused_create(C.byref(plan), 11, window.ctypes.data_as(fp), C.byref(band), None)
            assert st == 0, (st, af.last_error())
            made.append(plan)
    finally:
        os.environ.pop("AFX_MEL_NOPACK", None)
        if saved is not None:
            os.environ["AFX_MEL_NOPACK"] = saved
    packed, plain = made
    assert lib.afxk_melfused_pack(packed) == 1 and lib.afxk_melfused_pack(plain) == 0, "mel-128 at n_fft 2048 was not re-packed"
    assert lib.afxk_melfused_kind(packed) == 1 and lib.afxk_melfused_kind(plain) == 1
    k = np.arange(NUM)
    dct = np.sqrt(2.0 / NUM) * np.cos(np.pi * np.outer(k, k + 0.5) / NUM)
    dct[0] /= np.sqrt(2.0)
    dct = torch.from_numpy(np.ascontiguousarray(dct.astype(np.float32))).cuda()
    yield lib, packed, plain, dct
    torch.cuda.synchronize()
    lib.afxk_melfused_destroy(packed)
    lib.afxk_melfused_destroy(plain)
    lib.afx_bandplan_free(C.byref(band))


_clips = {}


def clips(hop):
    """the three clips on the device, made once per hop"""
    import torch
    if hop not in _clips:
        xs = np.stack([cases.noise(900 + hop + i, 2048 + (FRAMES - 1) * hop) for i in range(CLIPS)])
        _clips[hop] = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    return _clips[hop]


def run(lib, plan, route, hop, dct):
    """every output of the route, NaN-filled first; every value must have been written"""
    import torch
    xd = clips(hop)
    n = xd.shape[1]
    a = Args()
    a.x, a.clipStride, a.batch, a.dataLength, a.timeLength, a.hop = xd.data_ptr(), n, CLIPS, n, FRAMES, hop
    a.normValue = 1.0
    rows = lambda *shape: torch.full((CLIPS * FRAMES,) + shape, float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    out = {"mel": rows(NUM)}
    a.out = out["mel"].data_ptr()
    if route == "mfcc":
        out["cc"] = rows(CC)
        a.dct, a.ccNum, a.cc = dct.data_ptr(), CC, out["cc"].data_ptr()
    elif route == "complex":
        out["im"] = rows(NUM)
        a.specMap, a.outIm = 3, out["im"].data_ptr()
    elif route == "temporal":
        for name in ("energy", "rms", "zcr"):
            out[name] = rows()
        a.energy, a.rms, a.zcr = (out[name].data_ptr() for name in ("energy", "rms", "zcr"))
    torch.cuda.synchronize()
    st = lib.afxk_melfused_run(plan, C.byref(a), None)
    assert st == 0, (route, st, af.last_error())
    torch.cuda.synchronize()
    out = {name: v.cpu().numpy() for name, v in out.items()}
    for name, v in out.items():
        assert np.isfinite(v).all(), f"{route}: {name} has values that no wave wrote"
    return out


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("route", ["mfcc", "complex", "temporal"])
def test_packed_plan_equals_the_plan_as_it_came(route, hop, plans, monkeypatch):
    lib, packed, plain, dct = plans
    monkeypatch.setenv("AFX_MEL_CUS", "1")
    got, want = run(lib, packed, route, hop, dct), run(lib, plain, route, hop, dct)
    assert got["mel"].shape == (CLIPS * FRAMES, NUM) and np.abs(got["mel"]).max() > 0
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{route} at hop {hop}: {name} differs from the unpacked plan's bits"


def test_objects_get_the_packed_plan_and_their_results_do_not_depend_on_it(monkeypatch):
    """through bftObj_new (the same afxk_melfused_create): mel + MFCC-13 of a BFT object made with and without AFX_MEL_NOPACK"""
    import torch
    monkeypatch.setenv("AFX_MEL_CUS", "1")
    xd = clips(512)
    res = []
    for nopack in (False, True):
        if nopack:
            monkeypatch.setenv("AFX_MEL_NOPACK", "1")
        else:
            monkeypatch.delenv("AFX_MEL_NOPACK", raising=False)
        o = af.BFT(NUM, radix2_exp=11, samplate=16000, low_fre=0.0, high_fre=8000.0, slide_length=512,
                   scale_type=af.SpectralFilterBankScaleType.MEL, data_type=af.SpectralDataType.POWER)
        assert o.fused_plan_kind() == 1
        mel, cc = af.mel_mfcc_device(o, af.XXCC(NUM), xd, CC)
        torch.cuda.synchronize()
        res.append((mel.cpu().numpy(), cc.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
