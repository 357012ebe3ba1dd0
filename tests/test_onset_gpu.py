"""GPU parity of onset detection (af.Onset, mir/onset_algorithm.h, the device calls of afx_batch.h): the fixture of the compiled
reference's outputs by the rule of tests/onset_check.py through the host-pointer call and as a batch of one (live against the
compiled reference too when oracle/_ref is present); the checks of tests/onset_suite.py that the emulated kernels run as well --
the max filter and the picker against their restatements exactly, ties, T = 1 / step / step + 1, index tables, an unknown kind,
batches from a misaligned base, both sides of the picker's LDS bound, the envelope against the descriptor call bit for bit, the
dB map, every refusal --; the Python classes; the resident chain mel power -> dB -> onset."""
import ctypes as C
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import onset_cases as oc
from tests import onset_restate as rs
from tests import onset_suite as suite
from tests.onset_check import FACTOR, FLOOR, check_case

pytestmark = pytest.mark.gpu


class TorchDev:
    """device memory: torch tensors on the current device, the default stream"""

    @staticmethod
    def put(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def ptr(buf, first=0):
        return C.c_void_p(buf.data_ptr() + first * buf.element_size())

    @staticmethod
    def get(buf):
        import torch
        torch.cuda.synchronize()
        return buf.cpu().numpy()


D = TorchDev


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "onset.npz"))


@pytest.fixture(scope="module")
def lib():
    return oc.bind_device(af.get_lib())


@pytest.fixture(scope="module")
def ref_lib():
    return oc.bind(ref.lib()) if ref.available() else None


@pytest.mark.parametrize("name", list(oc.CASES))
def test_fixture_case(name, gold, lib, ref_lib):
    """the five fixture shapes and each of the eleven kinds once at (96, 24), phase rows for the five phase kinds"""
    suite.fixture_case(lib, D, name, gold, ref_lib)


def test_max_filter_is_exact(lib):
    suite.max_filter(lib, D)


def test_peak_pick_is_the_float32_rule(lib):
    suite.peak_pick(lib, D)


def test_bit_equal_ties(lib, ref_lib):
    suite.ties(lib, D, ref_lib)


def test_edge_lengths(lib, ref_lib):
    suite.edge_lengths(lib, D, ref_lib)


def test_index_tables(lib, ref_lib):
    suite.index_tables(lib, D, ref_lib)


def test_unknown_kind_equals_flux(lib):
    suite.unknown_kind(lib, D)


def test_batches_are_the_single_calls(lib):
    suite.batches(lib, D)


def test_both_sides_of_the_pickers_lds_bound(lib):
    suite.lds_bound(lib, D)


def test_envelope_is_the_normalised_descriptor(lib):
    suite.envelope_is_normalised_descriptor(lib, D)


def test_power_to_db(lib, gold, ref_lib):
    suite.power_to_db(lib, D, gold, ref_lib)


def test_refusals(lib):
    suite.refusals(lib, D)


def test_chunked_batches_equal_one_pass(lib, monkeypatch):
    """the filtered copy in chunks of one clip (AFX_ONSET_CHUNK_MB below two clips) == one pass, bitwise"""
    T, M, B = 300, 512, 3  # 600 KB per clip
    spec = np.stack([oc.burst_db(T, M, 20 + b) for b in range(B)])
    outs = []
    for mb in (None, "1"):
        if mb:
            monkeypatch.setenv("AFX_ONSET_CHUNK_MB", mb)
        st, obj = oc.new(lib, T, M, 512, 32000, 3)
        assert st == 0
        outs.append(suite.batch_call(lib, D, obj, spec))
        lib.onsetObj_free(obj)
    (s0, e0, p0, c0), (s1, e1, p1, c1) = outs
    assert s0 == 0 and s1 == 0 and suite.same_bits(e0, e1) and np.array_equal(p0, p1) and np.array_equal(c0, c1) and c0.min() > 0


def test_python_classes(lib, gold):
    """af.Onset mirrors the reference wrapper: (fre, time) input, its default NoveltyParam (the mean), four return values,
    leading axes as one batched call; onset_device, power_to_db, max_filter_device, peak_pick_device"""
    import torch
    name = "flux_o3_p2_abs_exp"
    c = oc.CASES[name]
    spec, _ = oc.case_input(name)
    o = af.Onset(c["T"], c["M"], c["hop"], samplate=c["sr"], filter_order=c["order"], novelty_type=af.NoveltyType.FLUX)
    par = af.NoveltyParam(*c["param"])
    pts, evn, tim, val = o.onset(spec.T, novelty_param=par)
    assert np.array_equal(pts, gold[name + "/points"]) and evn.shape == (c["T"],)
    assert np.array_equal(val, evn[pts]) and np.allclose(tim, pts * c["hop"] / c["sr"])
    two = np.stack([spec.T, spec.T[:, ::-1]])[None]  # (1, 2, fre, time)
    p2, e2, t2, v2 = o.onset(two, novelty_param=par)
    assert e2.shape == (1, 2, c["T"]) and p2.shape[:2] == (1, 2) and suite.same_bits(e2[0, 0], evn)
    assert np.array_equal(p2[0, 0, :len(pts)], pts) and (p2[0, 0, len(pts):] == 0).all() and np.array_equal(v2[0, 0, :len(pts)], val)
    # the wrapper's default parameters are not the C default: type 1, the mean
    d_pts, d_evn, _, _ = o.onset(spec.T)
    want = rs.envelope64(spec, None, oc.FLUX, c["order"], (1, 1.0, 1, 0, 1, 0.0, 1, 1.0))
    assert np.abs(d_evn - want).max() <= FLOOR
    e3, p3, c3 = o.onset_device(torch.from_numpy(spec[None]).cuda(), novelty_param=par, max_points=4)
    assert suite.same_bits(e3[0].cpu().numpy(), evn) and int(c3[0]) == len(pts) and np.array_equal(p3[0].cpu().numpy(), pts[:4])
    with pytest.raises(RuntimeError, match="status -6"):
        o.onset(spec.T, index_arr=np.array([c["M"]]))
    with pytest.raises(RuntimeError, match="status -6"):
        af.Onset(c["T"], c["M"], 512, novelty_type=af.NoveltyType.PD).onset(spec.T)
    with pytest.raises(ValueError):
        o.onset(spec)  # (time, fre) instead of (fre, time)
    p = oc.burst_power(60, 16, 7).astype(np.float32)
    bar = 1e-5 * np.abs(gold["db/out"]).max()
    assert np.abs(af.power_to_db(p) - gold["db/out"]).max() <= bar
    stack = np.stack([p, 3 * p])
    assert np.abs(af.power_to_db(stack) - gold["db/out"][None]).max() <= bar
    assert np.abs(af.power_to_db(torch.from_numpy(stack).cuda()).cpu().numpy() - gold["db/out"][None]).max() <= bar
    x = torch.from_numpy(spec).cuda()
    assert np.array_equal(af.max_filter_device(x, 4).cpu().numpy(), rs.max_filter(spec, 4))
    pk, cnt = af.peak_pick_device(torch.from_numpy(evn[None]).cuda(), 1, 1, 6, 7, 1, 0.07)
    assert int(cnt[0]) == len(pts) and np.array_equal(pk[0, :len(pts)].cpu().numpy(), pts)


def test_resident_chain_mel_power_db_onset(lib, ref_lib):
    """samples -> mel power (BFT, resident) -> power_to_db_device -> onset_device against the same mel rows through the
    reference's util_powerToDB and onsetObj_onset (through a float32 numpy dB when there is no compiled reference), by the
    rule: e64 is the float64 chain dB -> envelope from the float32 mel rows, the yardstick FACTOR x the reference chain's
    own distance from it"""
    import torch
    sr, hop, num = 16000, 256, 64
    rng = np.random.default_rng(4)
    n = 16000 * 2
    x = 0.01 * rng.standard_normal(n)
    for t0 in rng.integers(2000, n - 4000, 9):
        x[t0:t0 + 3000] += np.sin(2 * np.pi * rng.uniform(200, 3000) * np.arange(3000) / sr) * np.exp(-np.arange(3000) / 700.0)
    bft = af.BFT(num, radix2_exp=10, samplate=sr, low_fre=0.0, high_fre=8000.0, slide_length=hop,
                 scale_type=af.SpectralFilterBankScaleType.MEL, data_type=af.SpectralDataType.POWER)
    bft.set_result_type(1)
    mel = bft.bft_device(torch.from_numpy(x.astype(np.float32)[None]).cuda())  # (1, T, num): rows of frames
    mel = mel[0] if isinstance(mel, (tuple, list)) else mel
    T = mel.shape[1]
    db = af.power_to_db(mel.reshape(1, 1, T * num)).reshape(1, T, num)
    o = af.Onset(T, num, hop, samplate=sr, filter_order=3)
    evn, pts, cnt = o.onset_device(db)
    torch.cuda.synchronize()
    mel_h = mel[0].cpu().numpy()
    evn, pts = evn[0].cpu().numpy(), pts[0, :int(cnt[0])].cpu().numpy()
    pick, delta = rs.pick_params(sr, hop)
    e64 = rs.envelope64(oc.power_to_db64(mel_h), None, oc.FLUX, 3)
    if ref_lib is not None:
        ref_db = np.zeros(mel_h.size, np.float32)
        ref_lib.util_powerToDB(mel_h.reshape(-1).ctypes.data_as(oc.fp), mel_h.size, -80.0, ref_db.ctypes.data_as(oc.fp))
        st, robj = oc.new(ref_lib, T, num, hop, sr, 3)
        _, ref_evn, ref_pts = oc.call(ref_lib, robj, ref_db.reshape(T, num))
        ref_lib.onsetObj_free(robj)
    else:
        m = mel_h.astype(np.float32)
        ref_db = np.maximum(np.float32(10) * np.log10(m / m.max(), dtype=np.float32), np.float32(-80))
        ref_evn = rs.envelope64(ref_db, None, oc.FLUX, 3)
        ref_pts = rs.pick(ref_evn.astype(np.float32), pick, delta, np.float32)
    eps = max(FLOOR, FACTOR * float(np.abs(ref_evn - e64).max()))
    assert len(ref_pts) >= 5 and eps <= 1e-4, (len(ref_pts), eps)
    check_case("resident chain", e64, eps, ref_pts, evn, pts, pick, delta)
