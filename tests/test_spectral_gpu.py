"""GPU parity of the spectral-descriptor object (af.Spectral): the fixture cases, fresh inputs against the compiled reference,
silent frames, request lists against single requests, clips against per-clip calls, and the headline size."""
import os

import numpy as np
import pytest

import audioflux_amd as af
from audioflux_amd.spectral import KINDS, request
from oracle import ref
from tests import spectral_cases as sc
from tests import spectral_restate as sr
from tests.conftest import HOSTSTUB, parity_log
from tests.spectral_check import check_output

pytestmark = pytest.mark.gpu

INPUTS = sc.inputs()


def py_call(obj, case, spec, phase):
    """the wrapper method of a case, (fre, time) orientation in, list of [T] vectors out"""
    kind, i, f = sc.PARAMS[case]
    i, f = list(i) + [0] * 4, list(f) + [0.0] * 2
    m = spec.T
    if kind in sc.PHASE_KINDS:
        return [getattr(obj, kind)(m, phase.T)]
    if kind in sc.TWO_SLOT:
        return list(getattr(obj, kind)(m))
    # (the C isExp argument: `is_exp` of the Spectral wrapper, `is_no_exp` of the spectrogram wrapper, as in the reference)
    exp_key = "is_no_exp" if isinstance(obj, af.SpectrogramBase) else "is_exp"
    args = {"flux": {"step": i[0], "is_positive": i[1], exp_key: i[2], "tp": i[3], "p": f[0]}, "rolloff": dict(threshold=f[0]),
            "entropy": dict(is_norm=i[0]), "bandwidth": dict(p=f[0]), "energy": dict(is_log=i[0], gamma=f[0]),
            "sd": dict(step=i[0], is_positive=i[1]), "sf": dict(step=i[0], is_positive=i[1]), "mkl": dict(tp=i[0]),
            "broadband": dict(threshold=f[0]), "eef": dict(is_norm=i[0]), "eer": dict(is_norm=i[0], gamma=f[0]),
            "novelty": dict(step=i[0], threshold=f[0], method_type=af.SpectralNoveltyMethodType(i[1]),
                            data_type=af.SpectralNoveltyDataType(i[2]))}.get(kind, {})
    return [getattr(obj, "band_width" if kind == "bandwidth" else kind)(m, **args)]


def set_edge(obj, edge):
    if isinstance(edge, tuple):
        obj.set_edge(*edge)
    elif edge is not None:
        obj.set_edge_arr(edge)


@pytest.mark.parametrize("ename", ["full", "edge", "list"])
@pytest.mark.parametrize("iname", list(INPUTS))
def test_fixture_cases_through_the_wrapper(iname, ename, golden_dir):
    gold = np.load(os.path.join(golden_dir, "spectral.npz"))
    spec, phase, fre = INPUTS[iname]
    num = spec.shape[1]
    edge = sc.edges(num)[ename]
    o = af.Spectral(num, fre)
    set_edge(o, edge)
    idx = sc.edge_indices(num, edge)
    for case in sc.names_for(phase):
        outs = py_call(o, case, spec, phase)
        for k, got in enumerate(outs):
            key = f"{iname}/{ename}/{case}" + ("/fre" if k else "")
            check_output(key, case, got, gold[key], spec, phase, fre, idx, num, second=bool(k))


@pytest.mark.parametrize("power", [False, True])
@pytest.mark.parametrize("num", [2, 13, 40, 128, 129, 1025, 4097])
def test_fresh_inputs_against_the_compiled_reference(num, power):
    if not ref.available():
        pytest.skip("the compiled reference is not here")
    from tests.spectral_ref import RefSpectral
    rng = np.random.default_rng(num + power)
    T = 1000
    mag = np.abs(rng.standard_normal((T, num))) * np.exp(rng.uniform(-3, 3, (T, 1))) * np.exp(-np.arange(num) / (0.3 * num + 1))[None]
    spec = (mag ** 2 if power else mag).astype(np.float32)
    phase = rng.uniform(-np.pi, np.pi, (T, num)).astype(np.float32)
    fre = (np.arange(num) * 15.625 + 20.0).astype(np.float32)
    o = af.Spectral(num, fre)
    r = RefSpectral(ref.lib(), num, fre, None)
    idx = np.arange(num)
    for case in sc.PARAMS:
        kind, iarg, farg = sc.PARAMS[case]
        want = r.run(kind, iarg, farg, spec, phase)
        got = py_call(o, case, spec, phase)
        for k in range(len(want)):
            check_output(f"fresh {num} {'power' if power else 'mag'} {case}[{k}]", case, got[k], want[k], spec, phase, fre, idx, num,
                         second=bool(k))


def test_a_silent_frame_between_loud_ones():
    """the guarded descriptors return the reference's 0, entropy / eef / eer its NaN, on exactly the silent frame"""
    rng = np.random.default_rng(5)
    spec = np.abs(rng.standard_normal((9, 40))).astype(np.float32)
    spec[4] = 0
    fre = np.linspace(50, 4000, 40).astype(np.float32)
    o = af.Spectral(40, fre)
    m = spec.T
    if HOSTSTUB:
        o.entropy(m)
        return
    for name in ("flatness", "centroid", "spread", "skewness", "kurtosis", "crest", "slope", "decrease"):
        v = getattr(o, name)(m)
        assert np.all(np.isfinite(v)) and v[4] == 0, name
    for v in (o.entropy(m), o.eef(m), o.eer(m)):
        assert np.isnan(v[4]) and np.all(np.isfinite(np.delete(v, 4)))


def full_list(with_phase=True):
    names = [n for n in sc.PARAMS if n == sc.PARAMS[n][0] and (with_phase or n not in sc.PHASE_KINDS)]
    return names, [request(*sc.request_tuple(n)) for n in names]


@pytest.mark.parametrize("ename", ["full", "list"])
def test_a_request_list_equals_single_requests_bitwise(ename):
    import torch
    spec, phase, fre = INPUTS["linear257"]
    num = spec.shape[1]
    o = af.Spectral(num, fre)
    set_edge(o, sc.edges(num)[ename])
    ds, dp = torch.from_numpy(spec).cuda(), torch.from_numpy(phase).cuda()
    names, reqs = full_list()
    assert len(reqs) == 30 and sorted(r.kind for r in reqs) == list(range(30))
    whole = o.compute_device(ds, reqs, phase=dp).cpu().numpy()
    assert whole.shape == (33, spec.shape[0])
    slot = 0
    for n, r in zip(names, reqs):
        one = o.compute_device(ds, [r], phase=dp).cpu().numpy()
        assert np.array_equal(whole[slot:slot + one.shape[0]].view(np.uint32), one.view(np.uint32)), n
        slot += one.shape[0]


@pytest.mark.parametrize("step", [1, 2, 5])
def test_clips_of_a_batch_equal_per_clip_calls_bitwise(step):
    import torch
    clips, frames, num = 7, 131, 128
    g = torch.Generator(device="cuda").manual_seed(step)
    spec = torch.rand((clips * frames, num), generator=g, device="cuda") + 0.01
    phase = (torch.rand((clips * frames, num), generator=g, device="cuda") - 0.5) * 6.0
    o = af.Spectral(num, np.arange(num, dtype=np.float32) * 62.5)
    reqs = [request("flux", (step, 1, 0, 1), (2.0,)), request("sd", (step, 0)), request("sf", (step, 1)), request("mkl"),
            request("broadband", (), (1.0,)), request("novelty", (step, 2, 0), (0.0,)), request("pd"), request("wpd"), request("nwpd"),
            request("cd"), request("rcd")]
    whole = o.compute_device(spec, reqs, phase=phase, frames_per_clip=frames).cpu().numpy()
    for c in range(clips):
        lo, hi = c * frames, (c + 1) * frames
        one = o.compute_device(spec[lo:hi].contiguous(), reqs, phase=phase[lo:hi].contiguous()).cpu().numpy()
        assert np.array_equal(whole[:, lo:hi].view(np.uint32), one.view(np.uint32)), f"clip {c}"
        # flux / sd / sf / novelty: `step` leading zeros; mkl / broadband / cd / rcd: one; pd / wpd / nwpd: two
        assert np.all(one[[0, 1, 2, 5], :step] == 0) and np.all(one[[3, 4, 9, 10], 0] == 0) and np.all(one[6:9, :2] == 0)


def test_the_headline_size_resident_on_the_device():
    """934 000 x 128 rows generated on the device: the 19 row-local descriptors twice (bitwise equal), 2 000 sampled rows
    against float64, the centroid inside the band, no NaN in the guarded descriptors"""
    import torch
    rows, num = 934000, 128
    g = torch.Generator(device="cuda").manual_seed(7)
    spec = torch.rand((rows, num), generator=g, device="cuda") ** 4 * 50.0 + 1e-3
    fre = (700.0 * (10 ** (np.linspace(0, 2840, num) / 2595.0) - 1)).astype(np.float32)
    o = af.Spectral(num, fre)
    names = [n for n in sc.ROW_KINDS]
    reqs = [request(*sc.request_tuple(n)) for n in names]
    a = o.compute_device(spec, reqs)
    b = o.compute_device(spec, reqs)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    out = a.cpu().numpy()
    slot_of, s = {}, 0
    for n in names:
        slot_of[n] = s
        s += 2 if n in sc.TWO_SLOT else 1
    guarded = [n for n in names if n not in ("entropy", "eef", "eer")]
    for n in guarded:
        assert np.all(np.isfinite(out[slot_of[n]])), n
    c = out[slot_of["centroid"]]
    assert c.min() >= fre[0] and c.max() <= fre[-1]
    pick = np.random.default_rng(1).choice(rows, 2000, replace=False)
    sample = spec[torch.from_numpy(pick).cuda()].cpu().numpy()
    idx = np.arange(num)
    for n in names:
        kind, iarg, farg = sc.PARAMS[n]
        want = sr.restate(kind, iarg, farg, sample, None, fre, idx, num)
        for k, w in enumerate(want):
            got = out[slot_of[n] + k][pick]
            if kind == "rolloff":
                bad = got != w.astype(np.float32)
                assert bad.mean() <= 0.002, (n, bad.mean())
                continue
            err = np.abs(got - w).max() / np.abs(w).max()
            bar = 1e-4 if kind in sc.CANCELLING or kind == "kurtosis" else 1e-5
            parity_log(f"headline size {n}[{k}] vs float64", err, bar)
            assert err <= bar, (n, k, err)
