"""GPU parity of the time-stretch object (af.TimeStretch; mir/timeStretch_algorithm.h) against the compiled reference
(oracle/_ref when present, else tests/golden/timestretch.npz).  The vocoder's float32 phase accumulator is ill-conditioned
by construction, so the bars are per case and per norm, measured from the reference alone
(tests/golden/make_timestretch_golden.py: twice the distance at which the reference sits from itself when only its FFT's
rounding changes) and read from the fixture.  Every case of tests/timestretch_cases.py through the host-pointer call and
through timeStretchBatchDevice (bit-equal), a strided batch in chunks with guards, the vocoder alone on the reference's own
STFT, a rate sequence on a live object, refusals."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import timestretch_cases as tc
from tests.conftest import HOSTSTUB, assert_parity
from tests.resample_cases import signal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    af.get_lib()  # (loads the HIP runtime in the order the package wants)
    return tc.bind(C.CDLL(af.LIB_PATH))  # a handle of its own: the wrapper classes set other argument types on theirs


def same_bits(a, b):
    return HOSTSTUB or tc.same_bits(np.asarray(a), np.asarray(b))


def within_bars(got, want, name, what):
    """peak- and L2-relative error, each under the case's own bar"""
    bp, bl = tc.bar(name)
    assert np.shape(got) == np.shape(want), f"{what}: shape {np.shape(got)} vs {np.shape(want)}"
    if HOSTSTUB:
        return
    p, l2 = tc.errors(got, want)
    print(f"{what}: peak-rel {p:.3e} (bar {bp:.1e}), l2-rel {l2:.3e} (bar {bl:.1e})")
    assert p <= bp and l2 <= bl, f"{what}: peak-rel {p:.3e} > {bp:.1e} or l2-rel {l2:.3e} > {bl:.1e}"
    assert_parity(got, want, tol=max(bp, bl), what=what)


def _wrapper(c):
    return af.TimeStretch(c["exp"], c["hop"], af.WindowType(c.get("win", tc.HANN)))


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_meets_the_reference(name, lib):
    """the host-pointer call into a destination of 3.25 (overwrite semantics): returned length and capacity are the
    reference's, the input is unmodified, nothing behind the inverse transform's samples is touched, the samples are within
    the case's bars; the device call on 16-byte-aligned tensors is bit-equal to it and to itself"""
    import torch
    c = tc.CASES[name]
    x = tc.case_input(name)
    keep = x.copy()
    wret, wcap, want = tc.expected(name)
    L2 = tc.lengths(c, c["rate"])[2]
    ret, cap, got = tc.run_case(lib, name, fill=3.25)
    assert (ret, cap) == (wret, wcap) and np.array_equal(x, keep), (name, ret, cap, af.last_error())
    assert HOSTSTUB or (got[L2:] == np.float32(3.25)).all(), "samples behind the inverse transform's were written"
    within_bars(got[:L2], want, name, f"timestretch/{name}")
    o = _wrapper(c)
    assert o.cal_data_capacity(c["rate"], len(x)) == wcap
    xd = torch.from_numpy(x).cuda()[None]
    dev = o.time_stretch_batch_device(xd, c["rate"])
    again = o.time_stretch_batch_device(xd, c["rate"])
    assert xd.data_ptr() % 16 == 0 and dev.data_ptr() % 16 == 0 and dev.shape == (1, wret)
    dev, again = dev[0].cpu().numpy(), again[0].cpu().numpy()
    m = min(L2, wret)
    assert same_bits(dev[:m], got[:m]) and same_bits(dev, again) and not dev[m:].any(), name
    rows = o.time_stretch(x, c["rate"])
    assert rows.shape == (wcap,) and same_bits(rows[:L2], got[:L2]) and not rows[L2:].any()


def test_strided_batch_in_chunks_is_bitwise_the_single_calls(lib):
    """5 clips, clipStride > n, outStride > the length, NaN in the stride gaps, a scratch limit that makes the batch take
    three chunks: rows bitwise the single-clip calls, padding and guard rows untouched"""
    import torch
    c, n, clips, rate = tc.CASES["256_64_r0.8"], 3000, 5, 0.8
    o = _wrapper(c)
    p = tc.Plan()
    assert lib.afx_timestretch_plan(c["exp"], c["hop"], C.c_float(rate), n, clips, 0, C.byref(p), None, None) == 0
    assert p.clipsPerChunk == clips
    limit = 2 * p.scratchBytes + 100
    assert lib.afx_timestretch_plan(c["exp"], c["hop"], C.c_float(rate), n, clips, limit, C.byref(p), None, None) == 0
    assert p.clipsPerChunk == 2
    xs = torch.full((clips + 1, n + 13), float("nan"), device="cuda")
    for k in range(clips):
        xs[k, :n] = torch.from_numpy(signal(n, seed=40 + k))
    keep = xs.clone()
    single = [o.time_stretch_batch_device(xs[k:k + 1, :n].contiguous(), rate)[0].cpu().numpy() for k in range(clips)]
    m = p.returnLength
    o.set_scratch_limit(limit)
    out = torch.full((clips + 1, m + 7), 7.5, device="cuda")
    got = o.time_stretch_batch_device(xs[:clips, :n], rate, out=out[:clips])
    assert got.shape == (clips, m)
    out = out.cpu().numpy()
    for k in range(clips):
        assert same_bits(out[k, :m], single[k]), k
    assert HOSTSTUB or ((out[:clips, m:] == 7.5).all() and (out[clips] == 7.5).all())
    assert torch.equal(torch.nan_to_num(xs, nan=-1.0), torch.nan_to_num(keep, nan=-1.0))


@pytest.mark.parametrize("name", tc.VOCODER)
def test_vocoder_alone_meets_the_reference(name, lib):
    """afx_phase_vocoder_device on the reference's own STFT against the reference's phase_vocoder: L2-relative over the
    output planes within the case's bar, the mirror bins exact conjugates bit for bit"""
    import torch
    c = tc.CASES[name]
    N = 1 << c["exp"]
    F = N // 2 + 1
    re, im, wr, wi = tc.expected_vocoder(name)
    T1, T2 = re.shape[0], wr.shape[0]
    dre, dim = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    re2, im2 = torch.full((T2 + 1, N), 7.5, device="cuda"), torch.full((T2 + 1, N), 7.5, device="cuda")
    st = lib.afx_phase_vocoder_device(dre.data_ptr(), dim.data_ptr(), 1, T1, c["exp"], F, c["hop"], C.c_float(c["rate"]),
                                      re2.data_ptr(), im2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, af.last_error()
    re2, im2 = re2.cpu().numpy(), im2.cpu().numpy()
    assert HOSTSTUB or ((re2[T2] == 7.5).all() and (im2[T2] == 7.5).all())
    re2, im2 = re2[:T2], im2[:T2]
    j = np.arange(1, N // 2)
    assert same_bits(re2[:, N - j], re2[:, j]) and same_bits(im2[:, N - j], -im2[:, j])
    if not HOSTSTUB:
        got, want = np.concatenate([re2[:, :F], im2[:, :F]]), np.concatenate([wr, wi])
        l2 = tc.errors(got, want)[1]
        print(f"vocoder/{name}: l2-rel {l2:.3e} (bar {tc.bar(name)[1]:.1e})")
        assert l2 <= tc.bar(name)[1], (name, l2)


def test_rate_sequence_on_a_live_object_gives_what_fresh_objects_give(lib):
    """0.5, 1.7, 0.8, 0.5 on one object: bitwise what fresh objects give (scratch is reused, never trusted), each within its
    own bars of the reference"""
    c, x = dict(exp=8, hop=64, n=3000), signal(3000, seed=5)
    st, live = tc.new(lib, c)
    assert st == 0
    want = tc.expected_sequence()
    for k, rate in enumerate(tc.SEQUENCE):
        L2 = tc.lengths(c, rate)[2]
        got = tc.stretch(lib, live, x, rate, fill=3.25)[2][:L2]
        st, fresh = tc.new(lib, c)
        assert st == 0 and same_bits(got, tc.stretch(lib, fresh, x, rate)[2][:L2]), rate
        lib.timeStretchObj_free(fresh)
        within_bars(got, want[k], f"sequence/{k}", f"timestretch/sequence/{k}")
    lib.timeStretchObj_free(live)


def test_refusals(lib):
    """NULL handle and arrays, batch <= 0, short strides, rate 0 / negative / NaN, n < N, radix2Exp 15, slideLength > N: a
    status, nothing written, afx_error_count() advances for the host-pointer ones"""
    import torch
    I, V = C.c_int, C.c_void_p
    obj = V(None)
    assert lib.timeStretchObj_new(C.byref(obj), C.pointer(I(15)), None, None) == -4 and not obj
    assert lib.timeStretchObj_new(C.byref(obj), C.pointer(I(8)), C.pointer(I(257)), None) == -4 and not obj
    assert lib.pitchShiftObj_new(C.byref(obj), C.pointer(I(15)), None, None) == -4 and not obj
    assert lib.timeStretchObj_new(None, None, None, None) == -6
    c = dict(exp=8, hop=64)
    st, obj = tc.new(lib, c)
    assert st == 0
    x, out = signal(3000), np.full(8000, 3.25, np.float32)
    f = lib.timeStretchObj_timeStretch
    for args in ((None, 0.8, tc.ptr(x), 3000, tc.ptr(out)), (obj, 0.8, None, 3000, tc.ptr(out)), (obj, 0.8, tc.ptr(x), 3000, None),
                 (obj, 0.0, tc.ptr(x), 3000, tc.ptr(out)), (obj, -1.0, tc.ptr(x), 3000, tc.ptr(out)),
                 (obj, float("nan"), tc.ptr(x), 3000, tc.ptr(out)), (obj, float("inf"), tc.ptr(x), 3000, tc.ptr(out)),
                 (obj, 0.8, tc.ptr(x), 255, tc.ptr(out)), (obj, 0.8, tc.ptr(x), 0, tc.ptr(out))):
        before = lib.afx_error_count()
        assert f(args[0], C.c_float(args[1]), *args[2:]) == -6, args[1:4:2]
        assert lib.afx_error_count() > before and (out == np.float32(3.25)).all()
    assert lib.timeStretchObj_calDataCapacity(None, C.c_float(0.8), 3000) == 0
    assert lib.timeStretchObj_calDataCapacity(obj, C.c_float(0.0), 3000) == 0
    xd, od = torch.from_numpy(x).cuda(), torch.full((8000,), 7.5, device="cuda")
    g = lib.timeStretchObj_timeStretchBatchDevice
    xp, op = xd.data_ptr(), od.data_ptr()
    for args in ((None, 0.8, xp, 1, 3000, 3000, op, 3750), (obj, 0.8, None, 1, 3000, 3000, op, 3750), (obj, 0.8, xp, 1, 3000, 3000, None, 3750),
                 (obj, 0.8, xp, 0, 3000, 3000, op, 3750), (obj, 0.8, xp, -1, 3000, 3000, op, 3750), (obj, 0.8, xp, 2, 1500, 1499, op, 1875),
                 (obj, 0.8, xp, 2, 1500, 1500, op, 1874), (obj, 0.0, xp, 1, 3000, 3000, op, 3750), (obj, -0.5, xp, 1, 3000, 3000, op, 3750),
                 (obj, float("nan"), xp, 1, 3000, 3000, op, 3750), (obj, 0.8, xp, 1, 255, 255, op, 3750), (obj, 0.8, xp, 1, 0, 0, op, 3750)):
        assert g(args[0], C.c_float(args[1]), *args[2:], None) == -6, args[1:]
    torch.cuda.synchronize()
    assert HOSTSTUB or bool((od == 7.5).all())
    assert g(obj, C.c_float(0.8), xp, 2, 1500, 1500, op, 1875, None) == 1875
    torch.cuda.synchronize()
    lib.timeStretchObj_free(obj)
    lib.timeStretchObj_free(None)
    with pytest.raises(RuntimeError):
        af.TimeStretch(15)
    with pytest.raises(ValueError):
        af.TimeStretch(8, 64).time_stretch(x, 0.0)
