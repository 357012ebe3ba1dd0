"""GPU: every route through k_stft_mel_v2's frame loop (afx_melfused2.hip) gives the bits it gave before the loop's address
arithmetic moved to scalar bases and immediates (round 8: the hand-issued next-frame fetch, the scalar-base row stores, the
five-instruction pair power, the cepstrum block's row pointers).

None of those changes may move a result by a bit, so the check is exact: tests/golden/mel_v2_bits.npz holds what the library of
the commit before the change wrote for these seeded inputs on an MI355X, and every array must come back equal.  The shapes are
small on purpose -- 3 clips x 37 frames: with AFX_MEL_CUS=1 one workgroup's waves claim short runs that start inside a clip and
cross clip boundaries (whole-frame fetches between shifted ones), unset every wave has a frame or none -- and cover every
instantiation family: hops 512 / 256 / 1024 (SHIFT 4 / 2 / 8), hop 300 (SHIFT 0) on 8-byte aligned frame starts and, with clips
an odd number of floats apart, on unaligned ones; mel-128 + MFCC-13 in one launch (CC == 1), mel-40 (split plan, CC == 2),
complex results, the STFT rows (16-byte stores on rows of 1028 floats, and the bin slice) and the temporal instantiation.

Every output is NaN-filled first and every row must be written; the 1e-5 bar against the compiled reference (or the float64
restatement where oracle/_ref is not built) is the suite's own (tests/test_bft_gpu.py)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref, restate
from tests import cases
from tests.conftest import assert_parity

pytestmark = pytest.mark.gpu
TOL = 1e-5
FRAMES = 37
HOOK = "AFX_MEL_CUS"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mel_v2_bits.npz")
# (hop, extra samples per clip): an odd clip length puts the clips an odd number of floats apart -> the unaligned fetch path
MEL_CASES = [(512, 0), (256, 0), (1024, 0), (300, 0), (300, 1)]


def clips(hop, extra=0):
    return np.stack([cases.noise(4100 + hop + i, 2048 + (FRAMES - 1) * hop + extra) for i in range(3)])


def mel_bft(num=128, hop=512, **kw):
    return af.BFT(num, radix2_exp=11, samplate=16000, low_fre=0.0, high_fre=8000.0, slide_length=hop,
                  scale_type=af.SpectralFilterBankScaleType.MEL, data_type=af.SpectralDataType.POWER, **kw)


def nan_like(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def all_written(*arrays):
    for a in arrays:
        assert np.isfinite(a).all(), "values that no wave wrote"


def mel_mfcc(num, hop, extra=0):
    """mel + MFCC-13 of the three clips in ONE launch into NaN-filled outputs"""
    import torch
    o, xx = mel_bft(num=num, hop=hop), af.XXCC(num)
    assert o.fused_plan_kind() == (1 if num == 128 else 2)
    xs = clips(hop, extra)
    xd = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    assert o.cal_time_length(xs.shape[1]) == FRAMES
    mel, cc = nan_like(torch, (3, FRAMES, num)), nan_like(torch, (3, FRAMES, 13))
    af.mel_mfcc_device(o, xx, xd, 13, out_mel=mel, out_cc=cc)
    torch.cuda.synchronize()
    mel, cc = mel.cpu().numpy(), cc.cpu().numpy()
    all_written(mel, cc)
    return mel, cc


def bft_device(o, xs):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    shape = (xs.shape[0], o.cal_time_length(xs.shape[1]), o.num)
    re = nan_like(torch, shape)
    im = nan_like(torch, shape) if o.result_type == 0 else None
    o.bft_device(xd, out_real=re, out_imag=im)
    torch.cuda.synchronize()
    out = (re.cpu().numpy(),) + ((im.cpu().numpy(),) if im is not None else ())
    all_written(*out)
    return out


def complex_rows():
    o = mel_bft()
    o.set_result_type(0)
    return bft_device(o, clips(512))


def slice_rows(hop):
    """a linear-scale bin slice is the mapped spectrum row itself: afxk_stft2k's dword stores"""
    o = af.BFT(100, radix2_exp=11, samplate=16000, low_fre=1000.0, high_fre=8000.0, slide_length=hop,
               scale_type=af.SpectralFilterBankScaleType.LINEAR, data_type=af.SpectralDataType.POWER)
    o.set_result_type(1)
    return bft_device(o, clips(hop))[0]


class AfxStftArgs(C.Structure):  # audioflux_amd/csrc/hip/afx_device.h
    _fp, _ip = C.c_void_p, C.c_void_p
    _fields_ = [("x", _fp), ("clipStride", C.c_longlong), ("batch", C.c_int), ("dataLength", C.c_int), ("timeLength", C.c_int),
                ("radix2Exp", C.c_int), ("hop", C.c_int), ("window", _fp), ("twiddle", _fp), ("mode", C.c_int),
                ("normValue", C.c_float), ("binLo", C.c_int), ("binCount", C.c_int), ("outPitch", C.c_longlong),
                ("outRe", _fp), ("outIm", _fp), ("energy", _fp), ("rms", _fp), ("zcr", _fp), ("padLeft", C.c_int),
                ("bandStart", _ip), ("bandLen", _ip), ("bandOff", _ip), ("bandW", _fp), ("bandNum", C.c_int),
                ("bandPost", C.c_int), ("bandPostArg", C.c_float), ("fullSpectrum", C.c_int), ("padMode", C.c_int),
                ("padValueL", C.c_float), ("padValueR", C.c_float)]


def hann():
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2048) / 2048)).astype(np.float32)


def vec_rows(hop):
    """the dense-bank route's rows: all 1025 power bins on 16-byte aligned rows of 1028 floats (16-byte stores, zero pad)"""
    import torch
    lib = af.get_lib()
    lib.afxk_stft2k.restype = C.c_int
    lib.afxk_stft2k.argtypes = [C.POINTER(AfxStftArgs), C.c_void_p]
    xs = clips(hop)
    xd = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    wd = torch.from_numpy(hann()).cuda()
    out = nan_like(torch, (3 * FRAMES, 1028))
    assert xd.data_ptr() % 8 == 0 and wd.data_ptr() % 8 == 0 and out.data_ptr() % 16 == 0
    a = AfxStftArgs()
    a.x, a.clipStride, a.batch, a.dataLength, a.timeLength, a.radix2Exp, a.hop = xd.data_ptr(), xs.shape[1], 3, xs.shape[1], FRAMES, 11, hop
    a.window, a.mode, a.normValue, a.binLo, a.binCount, a.outPitch, a.outRe = wd.data_ptr(), 1, 1.0, 0, 1025, 1028, out.data_ptr()
    torch.cuda.synchronize()
    st = lib.afxk_stft2k(C.byref(a), None)
    assert st == 0, (st, af.last_error())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    all_written(out)
    return out


def temporal(clip):
    """TEMPORAL: energy / rms / zero-crossing rate beside the rows, through the reference entry point (one clip per call)"""
    o = mel_bft(is_temporal=True)
    rows = o.bft(clips(512)[clip], result_type=1)
    e, r, z = o.get_temporal_data()
    assert rows.shape == (128, FRAMES) and e.shape == r.shape == z.shape == (FRAMES,)
    all_written(rows, e, r, z)
    return rows, e, r, z


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def all_outputs():
    """name -> array of every route (what tests/golden/mel_v2_bits.npz holds, made by this very function)"""
    out = {}
    for hop, extra in MEL_CASES:
        out[f"mel128_h{hop}_x{extra}"], out[f"mfcc128_h{hop}_x{extra}"] = mel_mfcc(128, hop, extra)
    out["mel40_h512"], out["mfcc40_h512"] = mel_mfcc(40, 512)
    out["cplx_re_h512"], out["cplx_im_h512"] = complex_rows()
    for hop in (512, 300):
        out[f"slice_h{hop}"] = slice_rows(hop)
    for hop in (512, 1024):
        # 456 KB a piece: the fixture keeps a digest of all the rows and, at hop 512, the middle clip (its first frame follows a clip boundary)
        v = vec_rows(hop)
        if hop == 512:
            out[f"vec_h{hop}_clip1"] = v[FRAMES:2 * FRAMES]
        out[f"vec_h{hop}_sha256"] = np.frombuffer(bytes.fromhex(digest(v)), np.uint8)
    for clip in (0, 1):
        for name, a in zip(("rows", "energy", "rms", "zcr"), temporal(clip)):
            out[f"temporal_{name}_clip{clip}"] = a
    return out


_golden = {}


def golden(name):
    if not _golden:
        with np.load(GOLDEN) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden[name]


def assert_bits(name, got):
    want = golden(name)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    same = np.array_equal(got, want)
    if not same:
        d = got.view(np.uint32 if got.dtype == np.float32 else got.dtype) != want.view(np.uint32 if want.dtype == np.float32 else want.dtype)
        raise AssertionError(f"{name}: {int(d.sum())} of {d.size} values differ from the parent commit's bits, first at {tuple(np.argwhere(d)[0])}")


@pytest.fixture(params=["1", None], ids=["one_cu", "whole_device"])
def cus(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, request.param)
    return request.param


_reference = {}


def reference_clip0(hop, extra, num):
    """mel + MFCC-13 of clip 0 by the compiled reference (the float64 restatement where it is not built), once per case"""
    key = (hop, extra, num)
    if key not in _reference:
        x = clips(hop, extra)[0]
        if ref.available():
            m, c = ref.mel_mfcc(x[None], num=num, hop=hop)
            _reference[key] = m[0], c[0]
        else:
            bank, _, _ = restate.mel_bank(num, 2048, 16000, 0.0, 8000.0)
            m = restate.bft(x, bank, 2048, hop)
            _reference[key] = m, restate.xxcc(m)
    return _reference[key]


def power_rows(x, hop):
    w = hann().astype(np.float64)
    return np.stack([np.abs(np.fft.rfft(x[i * hop:i * hop + 2048].astype(np.float64) * w)) ** 2 for i in range(FRAMES)])


@pytest.mark.parametrize("hop,extra", MEL_CASES)
def test_mel128_mfcc13_one_launch(hop, extra, cus):
    """the headline instantiation family (CC == 1): SHIFT 4 / 2 / 8 / 0, aligned and unaligned fetches"""
    mel, cc = mel_mfcc(128, hop, extra)
    assert_bits(f"mel128_h{hop}_x{extra}", mel)
    assert_bits(f"mfcc128_h{hop}_x{extra}", cc)
    rmel, rcc = reference_clip0(hop, extra, 128)
    assert_parity(mel[0], rmel, TOL, f"mel hop {hop}+{extra}")
    assert_parity(cc[0], rcc, TOL, f"mfcc hop {hop}+{extra}")


def test_mel40_split_plan_general_cepstrum_block(cus):
    """SPLIT + CC == 2 (afx_ccblock.h)"""
    mel, cc = mel_mfcc(40, 512)
    assert_bits("mel40_h512", mel)
    assert_bits("mfcc40_h512", cc)
    rmel, rcc = reference_clip0(512, 0, 40)
    assert_parity(mel[0], rmel, TOL, "mel-40")
    assert_parity(cc[0], rcc, TOL, "mfcc of mel-40")


def test_complex_results(cus):
    """CPLX: two passes of the bank per frame, two output planes"""
    re, im = complex_rows()
    assert_bits("cplx_re_h512", re)
    assert_bits("cplx_im_h512", im)
    if ref.available():
        r = ref.RefBFT(128, 11, samplate=16000, low_fre=0.0, high_fre=8000.0, window_type=1, slide_length=512,
                       scale_type=2, style_type=0, normal_type=0, data_type=0)
        r.set_result_type(0)
        rre, rim = r.bft(clips(512)[0])
        assert_parity(re[0] + 1j * im[0], np.asarray(rre) + 1j * np.asarray(rim), TOL, "complex mel rows")


@pytest.mark.parametrize("hop", [512, 300])
def test_spectrum_rows_bin_slice(hop, cus):
    got = slice_rows(hop)
    assert_bits(f"slice_h{hop}", got)
    if ref.available():
        r = ref.RefBFT(100, 11, samplate=16000, low_fre=1000.0, high_fre=8000.0, window_type=1, slide_length=hop,
                       scale_type=0, style_type=0, normal_type=0, data_type=0)
        r.set_result_type(1)
        assert_parity(got[0], r.bft(clips(hop)[0])[0], TOL, f"spectrum slice hop {hop}")


@pytest.mark.parametrize("hop", [512, 1024])
def test_spectrum_rows_16_byte_stores(hop, cus):
    got = vec_rows(hop)
    if hop == 512:
        assert_bits(f"vec_h{hop}_clip1", got[FRAMES:2 * FRAMES])
    assert digest(got) == golden(f"vec_h{hop}_sha256").tobytes().hex(), "rows differ from the parent commit's bits"
    assert (got[:, 1025:] == 0).all()
    xs = clips(hop)
    for c in range(3):
        assert_parity(got[c * FRAMES:(c + 1) * FRAMES, :1025], power_rows(xs[c], hop), TOL, f"power rows hop {hop} clip {c}")


@pytest.mark.parametrize("clip", [0, 1])
def test_temporal_instantiation(clip, cus):
    rows, e, r, z = temporal(clip)
    for name, a in zip(("rows", "energy", "rms", "zcr"), (rows, e, r, z)):
        assert_bits(f"temporal_{name}_clip{clip}", a)
    if clip == 0:
        assert_parity(rows.T, reference_clip0(512, 0, 128)[0], TOL, "temporal rows")
    assert (e > 0).all()
