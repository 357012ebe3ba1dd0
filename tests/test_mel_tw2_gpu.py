"""GPU: the headline kernel with the W_64 twiddles on the reader side of exchange 2 (afx_melfused2.hip, round 10) on the
inputs where a twiddle by (1, -0) that moved from one element class to another could show: silence (signed zeros), single
impulses (every bin the same magnitude, most butterfly inputs exact zeros) and a full-scale sine on a bin centre.

3 clips x 37 frames at hop 512, mel-128 + MFCC-13 in one launch into NaN-filled outputs, with AFX_MEL_CUS=1 (one workgroup
claims every run: 16-frame runs, 4-frame tails, runs across clip boundaries) and unset.  Clip 1 is silence in both batches.
The 1e-5 bar against the reference is the suite's own (tests/conftest.py: assert_parity)."""
import warnings

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref, restate
from tests.conftest import assert_parity

pytestmark = pytest.mark.gpu
TOL = 1e-5
FRAMES, HOP, N = 37, 512, 2048
LEN = N + (FRAMES - 1) * HOP
HOOK = "AFX_MEL_CUS"


def _clip(kind):
    x = np.zeros(LEN, np.float32)
    if kind == "impulse0":
        x[0] = 1.0   # (frame 0 sees it under the window's zero; the point is the frames that see nothing)
        x[1024] = 1.0  # the window's peak of frame 0, sample 0 of frame 2
    elif kind == "impulse_odd":
        x[4097 + 777] = 1.0
        x[15001] = -0.5
    elif kind == "sine":
        x[:] = np.sin(2 * np.pi * 200 * np.arange(LEN) / N)  # full scale, centre of bin 200 in every frame
    return x


BATCHES = {"impulses": ("impulse0", "silence", "impulse_odd"), "sine": ("sine", "silence", "impulse0")}
_reference = {}


def reference(kind):
    """mel + MFCC-13 of one clip by the compiled reference (the float64 restatement where oracle/_ref is absent), once"""
    if kind not in _reference:
        x = _clip(kind)
        if ref.available():
            m, c = ref.mel_mfcc(x[None], num=128, hop=HOP)
            _reference[kind] = m[0], c[0]
        else:
            warnings.warn("oracle/_ref is not built: checked against the numpy restatement, not the compiled reference")
            bank, _, _ = restate.mel_bank(128, N, 16000, 0.0, 8000.0)
            m = restate.bft(x, bank, N, HOP)
            _reference[kind] = m, restate.xxcc(m)
    return _reference[kind]


def floor_row_f32(cc_num=13):
    """the cepstrum row of a mel row of 1e-8 floors, in float32 and in the kernel's order: log10 as log2(x) * log10(2); band
    16 u + 4 g + c goes to chain c, every chain adds its MFMAs' k-slots g = 0 .. 3 in order, (c0 + c1) + (c2 + c3) at the end"""
    f32 = np.float32
    k = np.arange(128)
    d = np.sqrt(2.0 / 128) * np.cos(np.pi * (k[None, :] + 0.5) * k[:cc_num, None] / 128)
    d[0] = np.sqrt(1.0 / 128)
    d = d.astype(f32)
    lg = f32(np.log2(np.float64(f32(1e-8)))) * f32(0.30102999566398120)
    acc = np.zeros((4, cc_num), f32)
    for u in range(8):
        for c in range(4):
            for g in range(4):
                acc[c] = (acc[c] + lg * d[:, 16 * u + 4 * g + c]).astype(f32)
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(f32)


def run(batch):
    import torch
    xs = np.stack([_clip(k) for k in batch])
    o = af.BFT(128, radix2_exp=11, samplate=16000, low_fre=0.0, high_fre=8000.0, slide_length=HOP,
               scale_type=af.SpectralFilterBankScaleType.MEL, data_type=af.SpectralDataType.POWER)
    xx = af.XXCC(128)
    assert o.fused_plan_kind() == 1
    xd = torch.from_numpy(xs).cuda()
    assert o.cal_time_length(LEN) == FRAMES
    mel = torch.full((3, FRAMES, 128), float("nan"), dtype=torch.float32, device="cuda")
    cc = torch.full((3, FRAMES, 13), float("nan"), dtype=torch.float32, device="cuda")
    af.mel_mfcc_device(o, xx, xd, 13, out_mel=mel, out_cc=cc)
    torch.cuda.synchronize()
    mel, cc = mel.cpu().numpy(), cc.cpu().numpy()
    assert np.isfinite(mel).all(axis=2).all() and np.isfinite(cc).all(axis=2).all(), "rows that no wave wrote"
    return mel, cc


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("cus", ["1", None])
def test_silence_impulses_and_sine(cus, name, monkeypatch):
    if cus is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, cus)
    batch = BATCHES[name]
    mel, cc = run(batch)
    # silence: every bin is an exact zero whatever the zeros' signs, so every mel value is 0.0 and every cepstrum row is the
    # row of 128 floors.  All 37 rows have the same inputs: the same bits.  Against the host's float32 restatement the bar is
    # the rounding of a 128-term float32 sum whose partial sums stay below 128 |lg| / sqrt(128) = 90.6 (half an ulp of 2^-17
    # each: 128 x 2^-18 = 4.9e-4) plus v_log_f32's one ulp of lg carried to the sum (90.6 x 2^-23 = 1.1e-5): 5.0e-4 absolute
    # -- the MFMA's own order of its four k-slots and the last bit of v_log_f32 are not the host's to restate (measured on an
    # MI355X: 1.5e-5, two ulp of the row's peak)
    assert batch[1] == "silence"
    assert np.all(mel[1] == 0.0), np.abs(mel[1]).max()
    assert all(cc[1, t].tobytes() == cc[1, 0].tobytes() for t in range(FRAMES))
    want = floor_row_f32()
    diff = float(np.abs(cc[1, 0] - want).max())
    print(f"silence cepstrum row against the float32 restatement: max abs difference {diff:.3e} (row peak {np.abs(want).max():.4f})")
    assert diff <= 5.0e-4
    for i in (0, 2):
        rmel, rcc = reference(batch[i])
        assert_parity(mel[i], rmel, TOL, f"mel of the {batch[i]} clip, {HOOK}={cus}")
        assert_parity(cc[i], rcc, TOL, f"mfcc of the {batch[i]} clip, {HOOK}={cus}")
