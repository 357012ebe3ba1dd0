"""GPU: the waves of a k_stft_mel_v2 workgroup claim runs of frames from their workgroup's range (afx_melfused2.hip).

A workgroup's waves only come back for a second run when the workgroup owns more frames than its first twelve runs, which
on a 256-CU device takes hundreds of thousands of frames.  AFX_MEL_CUS=N makes the launcher size its grid as if the device
had N CUs (read per launch), so a few hundred frames go through every part of the claim path: 16-frame runs, the
4-frame tail, the clamped last run, runs that start inside a clip and runs that cross a clip boundary.

A frame's values do not depend on the wave that computes it nor on the run it belongs to, so every comparison between two
partitions of the same frames is for equality of bits; the 1e-5 bar against the reference is the suite's own
(tests/test_bft_gpu.py)."""
import warnings

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref, restate
from tests import cases
from tests.conftest import assert_parity

pytestmark = pytest.mark.gpu
TOL = 1e-5
FRAMES = 301  # per clip: 3 x 301 = 903 frames, a multiple of neither 4 nor 16
HOOK = "AFX_MEL_CUS"


def clips(hop):
    return np.stack([cases.noise(900 + hop + i, 2048 + (FRAMES - 1) * hop) for i in range(3)])


def mel_bft(num=128, hop=512, **kw):
    return af.BFT(num, radix2_exp=11, samplate=16000, low_fre=0.0, high_fre=8000.0, slide_length=hop,
                  scale_type=af.SpectralFilterBankScaleType.MEL, data_type=af.SpectralDataType.POWER, **kw)


def nan_like(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def mel_mfcc(o, xx, xs, cc_num=13):
    """mel + MFCC of xs[clips, n] in ONE launch into NaN-filled outputs; every row must have been written"""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    t = o.cal_time_length(xs.shape[1])
    mel, cc = nan_like(torch, (xs.shape[0], t, o.num)), nan_like(torch, (xs.shape[0], t, cc_num))
    af.mel_mfcc_device(o, xx, xd, cc_num, out_mel=mel, out_cc=cc)
    torch.cuda.synchronize()
    mel, cc = mel.cpu().numpy(), cc.cpu().numpy()
    assert np.isfinite(mel).all(axis=2).all() and np.isfinite(cc).all(axis=2).all(), "rows that no wave wrote"
    return mel, cc


def per_clip(fn, xs):
    """the same clips one per call: other workgroup ranges, other runs"""
    parts = [fn(xs[i:i + 1]) for i in range(xs.shape[0])]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))


_reference = {}


def compiled_reference():
    """whether the compiled reference is built; where it is not, the checks against it fall back to the float64 numpy
    restatement (as __graft_entry__.smoke does) or are left out, and say so"""
    if not ref.available():
        warnings.warn("oracle/_ref is not built: checked against the numpy restatement, not the compiled reference")
    return ref.available()


def reference_clip0(hop, num=128):
    """mel + MFCC-13 of clip 0 by the compiled reference, computed once per (hop, num)"""
    if (hop, num) not in _reference:
        x = clips(hop)[0]
        if compiled_reference():
            m, c = ref.mel_mfcc(x[None], num=num, hop=hop)
            _reference[hop, num] = m[0], c[0]
        else:
            bank, _, _ = restate.mel_bank(num, 2048, 16000, 0.0, 8000.0)
            m = restate.bft(x, bank, 2048, hop)
            _reference[hop, num] = m, restate.xxcc(m)
    return _reference[hop, num]


@pytest.mark.parametrize("hop", [512, 256, 300])  # SHIFT 4, SHIFT 2, SHIFT 0 with unaligned fetches
@pytest.mark.parametrize("cus", [1, 2])
def test_claimed_runs_equal_per_clip_calls_and_the_reference(cus, hop, monkeypatch):
    """3 clips x 301 frames, mel-128 + MFCC-13 in one launch (the headline instantiation at hop 512)"""
    monkeypatch.setenv(HOOK, str(cus))
    o, xx = mel_bft(hop=hop), af.XXCC(128)
    assert o.fused_plan_kind() == 1
    xs = clips(hop)
    mel, cc = mel_mfcc(o, xx, xs)
    assert mel.shape == (3, FRAMES, 128) and cc.shape == (3, FRAMES, 13)
    mel1, cc1 = per_clip(lambda x: mel_mfcc(o, xx, x), xs)
    assert np.array_equal(mel, mel1) and np.array_equal(cc, cc1)
    rmel, rcc = reference_clip0(hop)
    assert_parity(mel[0], rmel, TOL, f"mel hop {hop} at {cus} CU")
    assert_parity(cc[0], rcc, TOL, f"mfcc hop {hop} at {cus} CU")


def test_unset_hook_gives_the_same_bits(monkeypatch):
    """the main case on the whole device (every wave claims at most one short run) against one workgroup's claimed runs"""
    o, xx = mel_bft(), af.XXCC(128)
    xs = clips(512)
    monkeypatch.delenv(HOOK, raising=False)
    mel, cc = mel_mfcc(o, xx, xs)
    monkeypatch.setenv(HOOK, "1")
    mel1, cc1 = mel_mfcc(o, xx, xs)
    assert np.array_equal(mel, mel1) and np.array_equal(cc, cc1)


@pytest.mark.parametrize("cus", [1, 2])
def test_split_plan_with_the_general_cepstrum_block(cus, monkeypatch):
    """mel-40: row segments (SPLIT) and the cepstrum block of afx_ccblock.h (CC == 2), one call site at the end of a run"""
    monkeypatch.setenv(HOOK, str(cus))
    o, xx = mel_bft(num=40), af.XXCC(40)
    assert o.fused_plan_kind() == 2
    xs = clips(512)
    mel, cc = mel_mfcc(o, xx, xs)
    mel1, cc1 = per_clip(lambda x: mel_mfcc(o, xx, x), xs)
    assert np.array_equal(mel, mel1) and np.array_equal(cc, cc1)
    rmel, rcc = reference_clip0(512, 40)
    assert_parity(mel[0], rmel, TOL, f"mel-40 at {cus} CU")
    assert_parity(cc[0], rcc, TOL, f"mfcc of mel-40 at {cus} CU")


def bft_device(o, xs):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    shape = (xs.shape[0], o.cal_time_length(xs.shape[1]), o.num)
    re = nan_like(torch, shape)
    im = nan_like(torch, shape) if o.result_type == 0 else None
    o.bft_device(xd, out_real=re, out_imag=im)
    torch.cuda.synchronize()
    out = (re.cpu().numpy(),) + ((im.cpu().numpy(),) if im is not None else ())
    for a in out:
        assert np.isfinite(a).all(axis=2).all(), "rows that no wave wrote"
    return out


@pytest.mark.parametrize("cus", [1, 2])
def test_complex_results(cus, monkeypatch):
    """CPLX: real and imaginary planes, two passes of the bank per frame"""
    monkeypatch.setenv(HOOK, str(cus))
    o = mel_bft()
    o.set_result_type(0)
    xs = clips(512)
    got = bft_device(o, xs)
    one = per_clip(lambda x: bft_device(o, x), xs)
    assert len(got) == 2 and np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])
    monkeypatch.delenv(HOOK)
    whole = bft_device(o, xs)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


@pytest.mark.parametrize("cus", [1, 2])
def test_spectrum_rows(cus, monkeypatch):
    """STFT: afxk_stft2k's rows (a linear-scale bin slice is the mapped spectrum row itself), hop 512 and an odd hop"""
    for hop in (512, 300):
        o = af.BFT(100, radix2_exp=11, samplate=16000, low_fre=1000.0, high_fre=8000.0, slide_length=hop,
                   scale_type=af.SpectralFilterBankScaleType.LINEAR, data_type=af.SpectralDataType.POWER)
        o.set_result_type(1)
        xs = clips(hop)
        monkeypatch.setenv(HOOK, str(cus))
        got, = bft_device(o, xs)
        one, = per_clip(lambda x: bft_device(o, x), xs)
        assert np.array_equal(got, one)
        monkeypatch.delenv(HOOK)
        whole, = bft_device(o, xs)
        assert np.array_equal(got, whole)
        if compiled_reference():
            r = ref.RefBFT(100, 11, samplate=16000, low_fre=1000.0, high_fre=8000.0, window_type=1, slide_length=hop,
                           scale_type=0, style_type=0, normal_type=0, data_type=0)
            r.set_result_type(1)
            assert_parity(got[0], r.bft(xs[0])[0], TOL, f"spectrum rows hop {hop} at {cus} CU")


@pytest.mark.parametrize("cus", [1, 2])
def test_temporal_features(cus, monkeypatch):
    """TEMPORAL: energy / rms / zero-crossing rate beside the rows, one clip of 301 frames through the reference entry point"""
    o = mel_bft(is_temporal=True)
    x = clips(512)[0]
    monkeypatch.delenv(HOOK, raising=False)
    want = o.bft(x, result_type=1)
    want_t = o.get_temporal_data()
    monkeypatch.setenv(HOOK, str(cus))
    got = o.bft(x, result_type=1)
    got_t = o.get_temporal_data()
    assert got.shape == (128, FRAMES) and np.isfinite(got).all() and np.array_equal(got, want)
    for g, w in zip(got_t, want_t):
        assert g.shape == (FRAMES,) and np.isfinite(g).all() and np.array_equal(g, w)
    assert_parity(got.T, reference_clip0(512)[0], TOL, f"temporal rows at {cus} CU")
    assert (got_t[0] > 0).all()


@pytest.mark.parametrize("frames", [5, 192])
@pytest.mark.parametrize("cus", [1, 2])
def test_edge_sizes(cus, frames, monkeypatch):
    """5 frames: one workgroup of one-frame runs with or without the hook, most waves claim nothing.  192 frames at 1 CU: 16
    frames per wave remain only for the first claim (one 16-frame run), every later run has 4 frames; at 2 CUs two ranges of 96
    frames in 4-frame runs; without the hook one frame per wave over 16 workgroups"""
    o, xx = mel_bft(), af.XXCC(128)
    xs = clips(512)[:1, :2048 + (frames - 1) * 512]  # the start of clip 0 of the main case
    monkeypatch.setenv(HOOK, str(cus))
    mel, cc = mel_mfcc(o, xx, xs)
    assert mel.shape == (1, frames, 128)
    monkeypatch.delenv(HOOK)
    mel1, cc1 = mel_mfcc(o, xx, xs)
    assert np.array_equal(mel, mel1) and np.array_equal(cc, cc1)
    rmel, rcc = reference_clip0(512)
    assert_parity(mel[0], rmel[:frames], TOL, f"{frames} frames at {cus} CU")
    assert_parity(cc[0], rcc[:frames], TOL, f"mfcc of {frames} frames at {cus} CU")
