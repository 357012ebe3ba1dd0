"""GPU parity of the harmonic-product and log-harmonic-sum pitch trackers (af.PitchHPS / af.PitchLHS, mir/_pitch_hps.h,
mir/_pitch_lhs.h): the fixture of the compiled reference's outputs by the rule of tests/pitch_hs_check.py through the
host-pointer call and through pitchBatchDevice, fresh inputs against the compiled reference when oracle/_ref is present,
the curve export, batch == per-clip calls bitwise with guards, silent frames, streaming in pieces == one call, refusals,
and the plan whose spectrum slice lives in device scratch."""
import ctypes as C
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import pitch_hs_cases as hc
from tests import pitch_hs_restate as hr
from tests.conftest import HOSTSTUB, parity_log
from tests.pitch_cases import signal
from tests.pitch_hs_check import check_case, check_curve, index_of

pytestmark = pytest.mark.gpu
KINDS = [hc.HPS, hc.LHS]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "pitch_hs.npz"))


@pytest.fixture(scope="module")
def lib():
    return hc.bind_device(af.get_lib())


def same_bits(a, b):
    return HOSTSTUB or np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _cls(kind):
    return af.PitchHPS if kind == hc.HPS else af.PitchLHS


def _obj(kind, sr, lo, hi, r, hop, window, count):
    return _cls(kind)(samplate=sr, low_fre=lo, high_fre=hi, radix2_exp=r, slide_length=hop, window_type=window, harmonic_count=count)


def _restated(name, kind):
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
    M, mn, mx, cnt, wt = hc.plan(kind, sr, lo, hi, r, hop, window, count)
    return hr.pitch(kind, hc.case_input(name), sr, r, hop, wt, M, mn, mx, cnt), M


@pytest.mark.parametrize("name,kind", hc.pairs(), ids=[f"{n}-{hc.KIND_NAME[k]}" for n, k in hc.pairs()])
def test_fixture_case(name, kind, gold, lib):
    """every case through pitch() with host pointers and through pitchBatchDevice: the acceptance rule, both routes bit-equal;
    the curve against the restatement with the weighted bar; dValue == curve[index] exactly"""
    import torch
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
    key = f"{name}/{hc.KIND_NAME[kind]}"
    x = hc.case_input(name)
    fre = hc.run_case(lib, name, kind)
    o = _obj(kind, sr, lo, hi, r, hop, window, count)
    xd = torch.from_numpy(x).cuda()[None]
    dfre, dval = (t[0].cpu().numpy() for t in o.pitch_batch_device(xd))
    curve = o.curve_batch_device(xd)[0].cpu().numpy()
    frames, M = _restated(name, kind)
    assert (o.interp_length, len(fre), curve.shape) == (M, len(frames), (len(frames), o.max_index + 1))
    assert same_bits(fre, dfre), key
    w = check_case(key, frames, gold[key + "/eps"], gold[key + "/fre"], fre, sr, M, curve)
    parity_log(f"pitch_hs/{key}", w["worst_curve"] * 1e-5, 1e-5, "pitch_hs: worst curve error / its bar, scaled to 1e-5",
               {"explained": w["explained"], "frames": w["frames"]})
    for t in range(len(fre)):
        i = index_of(fre[t], sr, M)
        assert same_bits(dval[t:t + 1], curve[t, i:i + 1]), (key, t, i)
    if name in hc.CURVES:  # the stored rows are the restatement's
        c64 = gold[key + "/curve64"]
        for t, f in enumerate(frames):
            fin = np.isfinite(c64[t])
            assert np.allclose(c64[t][fin], f["curve"][fin], rtol=1e-6, atol=0), (key, t)


@pytest.mark.parametrize("kind", KINDS, ids=["HPS", "LHS"])
@pytest.mark.parametrize("name", ["d1_sr8k_r13", "d2_sr16k_r13", "d8_default_r12", "d16_sr16k_r10", "d128_sr8k_r6"])
def test_fresh_input_against_the_compiled_reference(name, kind, lib):
    """one case per D class with a seed the fixture has not seen, noise added so that no bin sits below float32 rounding"""
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    from tests.golden.make_pitch_hs_golden import reference_case
    _, sr, lo, hi, r, hop, window, count, sig, n = hc.CASES[name]
    x = signal(sig, n, sr, seed=977) + 0.01 * signal("noise", n, sr, seed=978)
    ref_fre, eps, frames = reference_case(hc.bind(ref.lib()), name, kind, x)
    st, obj = hc.new(lib, kind, sr, lo, hi, r, hop, window, count)
    assert st == 0
    fre = hc.call(lib, kind, obj, x)
    hc.free(lib, kind, obj)
    w = check_case(f"fresh/{name}", frames, eps, ref_fre, fre, sr, hc.round_pow2(sr))
    parity_log(f"pitch_hs/fresh/{name}/{hc.KIND_NAME[kind]}", float(w["explained"]), max(1, w["frames"] // 100),
               "pitch_hs: explained frames / cap")


@pytest.mark.parametrize("kind", KINDS, ids=["HPS", "LHS"])
def test_batch_equals_single_calls_and_writes_nothing_else(kind, lib):
    """3 clips, clipStride > dataLength, outStride > frames, misaligned base pointer, outputs pre-filled with NaN"""
    import torch
    sr, r, hop = 16000, 9, 128
    n, clips, stride = 512 + 128 * 5 + 5, 3, 512 + 128 * 5 + 17
    buf = np.zeros(clips * stride + 1, np.float32)
    xs = buf[1:].reshape(clips, stride)
    for c, sig in enumerate(("tone:330", "stack:196", "glide")):
        xs[c, :n] = signal(sig, n, sr, seed=70 + c)
    o = _obj(kind, sr, 40.0, 2000.0, r, hop, hc.HAMM, 4)
    T = o.cal_time_length(n)
    single = [o.pitch(xs[c, :n].copy()) for c in range(clips)]
    d = torch.from_numpy(buf).cuda()
    assert (d.data_ptr() + 4) % 16 == 4
    pitch_stride, guard = T + 3, 64
    f = torch.full((clips * pitch_stride + guard,), float("nan"), device="cuda")
    v = torch.full_like(f, float("nan"))
    fn = getattr(lib, f"pitch{hc.KIND_NAME[kind]}Obj_pitchBatchDevice")
    st = fn(o._obj, d.data_ptr() + 4, clips, n, stride, f.data_ptr(), v.data_ptr(), pitch_stride, torch.cuda.current_stream().cuda_stream)
    assert st == 0, af.last_error()
    torch.cuda.synchronize()
    fh, vh = f.cpu().numpy(), v.cpu().numpy()
    rows_f, rows_v = fh[:clips * pitch_stride].reshape(clips, pitch_stride), vh[:clips * pitch_stride].reshape(clips, pitch_stride)
    for c in range(clips):
        assert same_bits(rows_f[c, :T], single[c]), c
    assert not np.isnan(rows_f[:, :T]).any() and not np.isnan(rows_v[:, :T]).any(), "a frame entry was not written"
    assert np.isnan(rows_f[:, T:]).all() and np.isnan(rows_v[:, T:]).all(), "wrote beyond a row's frames"
    assert np.isnan(fh[clips * pitch_stride:]).all() and np.isnan(vh[clips * pitch_stride:]).all(), "wrote into the guard"


@pytest.mark.parametrize("kind", KINDS, ids=["HPS", "LHS"])
@pytest.mark.parametrize("name", ["zero_r10", "step_r10"])
def test_silent_frames_give_min_index(name, kind, lib):
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
    x = hc.case_input(name)
    fre = hc.run_case(lib, name, kind)
    M, mn = hc.round_pow2(sr), int(np.ceil(lo))
    want = np.float32((mn + 1) * (1.0 * sr / M))
    N = 1 << r
    silent = [t for t in range(len(fre)) if not x[t * hop:t * hop + N].any()]
    assert silent, name
    if not HOSTSTUB:
        assert all(fre[t] == want for t in silent), (fre, want)


@pytest.mark.parametrize("kind", KINDS, ids=["HPS", "LHS"])
@pytest.mark.parametrize("r,hop", [(8, 100), (8, 300)])
def test_streaming_in_three_uneven_pieces(kind, r, hop, lib):
    sr, N = 16000, 1 << r
    x = signal("glide", N + hop * 9 + 31, sr, seed=90)
    st, one = hc.new(lib, kind, sr, 60.0, 2000.0, r, hop, hc.HAMM, 3)
    assert st == 0
    whole = hc.call(lib, kind, one, x)
    hc.free(lib, kind, one)
    st, obj = hc.new(lib, kind, sr, 60.0, 2000.0, r, hop, hc.HAMM, 3, cont=1)
    assert st == 0
    parts = [hc.call(lib, kind, obj, p) for p in np.split(x, [len(x) // 5, len(x) // 5 + 2 * N + 3])]
    hc.free(lib, kind, obj)
    got = np.concatenate(parts)
    assert len(got) == len(whole) and same_bits(got, whole)


@pytest.mark.parametrize("kind", KINDS, ids=["HPS", "LHS"])
def test_refusals_on_the_device_path(kind, lib):
    import torch
    sr, r, hop = 16000, 9, 128
    n = 512 + 128 * 3
    x = torch.from_numpy(signal("tone:330", n, sr, seed=3)).cuda()
    out = torch.full((16,), 5.0, device="cuda")
    fn = getattr(lib, f"pitch{hc.KIND_NAME[kind]}Obj_pitchBatchDevice")
    cv = getattr(lib, f"pitch{hc.KIND_NAME[kind]}Obj_curveBatchDevice")
    s = torch.cuda.current_stream().cuda_stream
    st, cont = hc.new(lib, kind, sr, 40.0, 2000.0, r, hop, hc.HAMM, 3, cont=1)
    assert st == 0
    assert fn(cont, x.data_ptr(), 1, n, n, out.data_ptr(), None, 16, s) == -4
    hc.free(lib, kind, cont)
    st, o = hc.new(lib, kind, sr, 40.0, 2000.0, r, hop, hc.HAMM, 3)
    assert st == 0
    assert fn(None, x.data_ptr(), 1, n, n, out.data_ptr(), None, 16, s) == -6
    assert fn(o, None, 1, n, n, out.data_ptr(), None, 16, s) == -6
    assert fn(o, x.data_ptr(), 1, n, n, None, None, 16, s) == -6
    assert fn(o, x.data_ptr(), 0, n, n, out.data_ptr(), None, 16, s) == -6
    assert fn(o, x.data_ptr(), 1, 0, n, out.data_ptr(), None, 16, s) == -6
    assert fn(o, x.data_ptr(), 1, n, n - 1, out.data_ptr(), None, 16, s) == -6  # clipStride below dataLength
    assert fn(o, x.data_ptr(), 1, n, n, out.data_ptr(), None, 3, s) == -6      # outStride below the 4 frames
    assert cv(o, x.data_ptr(), 1, n, n, None, s) == -6
    assert fn(o, x.data_ptr(), 1, 511, n, out.data_ptr(), None, 16, s) == 0    # no frame: nothing to do
    hc.free(lib, kind, o)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5).all(), "a refused / empty call wrote"


@pytest.mark.parametrize("kind", KINDS, ids=["HPS", "LHS"])
def test_scratch_slice_plan(kind, lib):
    """the plan whose spectrum slice does not fit in LDS (the plan says where the slice lives): the decision follows the
    restatement, every frame's curve entry by entry; with more frames than workgroups in the launch, the frames of the later
    passes equal the same frames at the head of a short clip"""
    import torch
    name = "scratch_r12"
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
    plan = hc_plan(lib, kind, sr, lo, hi, r, hop, window, count)
    assert plan.sliceInLds == 0 and plan.lastBin == 30000
    default = hc_plan(lib, kind)
    assert default.sliceInLds == 1 and default.lastBin == 10000 and default.transforms == 5
    frames, M = _restated(name, kind)
    o = _obj(kind, sr, lo, hi, r, hop, window, count)
    xd = torch.from_numpy(hc.case_input(name)).cuda()[None]
    fre = o.pitch_batch_device(xd)[0][0].cpu().numpy()
    curve = o.curve_batch_device(xd)[0].cpu().numpy()
    if HOSTSTUB:
        return
    eps = 1e-5  # the floor of the rule
    worst = max(check_curve(name, t, f, eps, curve[t]) for t, f in enumerate(frames))
    for t, f in enumerate(frames):
        i = index_of(fre[t], sr, M)
        if i != f["index"]:
            gap = abs(f["curve"][i] - f["curve"][f["index"]])
            assert gap <= eps * (f["weight"][i] + f["weight"][f["index"]]), (t, i, f["index"], gap)
    parity_log(f"pitch_hs/scratch/{hc.KIND_NAME[kind]}", worst * 1e-5, 1e-5, "pitch_hs: worst curve error / its bar, scaled to 1e-5")
    # 1100 frames over 1024 workgroups: frames 1024 ... 1099 are second passes
    N, hop2, T2 = 1 << r, 16, 1100
    o2 = _obj(kind, sr, lo, hi, r, hop2, window, count)
    x2 = torch.from_numpy(signal("noise", N + hop2 * (T2 - 1), sr, seed=41)).cuda()[None]
    long_f, long_v = (t[0].cpu().numpy() for t in o2.pitch_batch_device(x2))
    tail_f, tail_v = (t[0].cpu().numpy() for t in o2.pitch_batch_device(x2[:, 1024 * hop2:].contiguous()))
    assert len(long_f) == T2 and len(tail_f) == T2 - 1024
    assert same_bits(long_f[1024:], tail_f) and same_bits(long_v[1024:], tail_v)


class _Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("samplate", "radix2Exp", "fftLength", "slideLength", "isContinue")] + \
               [("lowFre", C.c_float), ("highFre", C.c_float)] + \
               [(n, C.c_int) for n in ("windowType", "interpLength", "minIndex", "maxIndex", "harmonicCount", "lastBin", "transforms",
                                       "sliceInLds")] + [("sliceFloats", C.c_longlong), ("ldsBytes", C.c_longlong)]


def hc_plan(lib, kind, sr=None, lo=None, hi=None, r=None, hop=None, window=None, count=None):
    p = _Plan()
    f = lib.afx_pitch_hs_plan_host
    f.restype = C.c_int
    f.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.POINTER(_Plan)]
    o = lambda v, t: None if v is None else C.cast(C.pointer(t(v)), C.c_void_p)  # noqa: E731
    st = f(kind, o(sr, C.c_int), o(lo, C.c_float), o(hi, C.c_float), o(r, C.c_int), o(hop, C.c_int), o(window, C.c_int),
           o(count, C.c_int), None, C.byref(p))
    assert st == 0, st
    return p
