"""GPU parity of the pitch-shift object (af.PitchShift; mir/pitchShift_algorithm.h) against the compiled reference
(oracle/_ref when present, else tests/golden/timestretch.npz) at the per-case bars of the fixture (the perturbed and
unperturbed stretched signals of tests/golden/make_timestretch_golden.py pushed through the reference's resampler): the
cases of timestretch_cases.PITCH through the host-pointer call and pitchShiftBatchDevice (bit-equal), the length rule -- never
more than the input's length, the rest of a shorter result untouched --, a strided batch in chunks, refusals."""
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
    af.get_lib()
    return tc.bind(C.CDLL(af.LIB_PATH))


def same_bits(a, b):
    return HOSTSTUB or tc.same_bits(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("name", list(tc.PITCH))
def test_case_meets_the_reference(name, lib):
    """the host-pointer call into a destination of 3.25: exactly min(n, resampled length) samples are written, the input is
    unmodified, the samples are within the case's bars; the device call is bit-equal to it and to itself"""
    import torch
    c = tc.PITCH[name]
    x = tc.case_input(name)
    keep = x.copy()
    want = tc.expected_pitch(name)
    m = tc.pitch_length(c["n"], c["semi"])
    before = lib.afx_error_count()
    out = tc.run_pitch(lib, name, fill=3.25)
    assert lib.afx_error_count() == before, af.last_error()
    assert np.array_equal(x, keep) and (HOSTSTUB or (out[m:] == np.float32(3.25)).all()), "samples behind the length were written"
    got = out[:m]
    o = af.PitchShift(c["exp"], c["hop"])
    xd = torch.from_numpy(x).cuda()[None]
    dev = o.pitch_shift_batch_device(xd, c["semi"])
    again = o.pitch_shift_batch_device(xd, c["semi"])
    assert dev.shape == (1, m) and same_bits(dev[0].cpu().numpy(), got) and same_bits(again[0].cpu().numpy(), got), name
    rows = o.pitch_shift(np.stack([x, x]), c["semi"], samplate=44100)
    assert rows.shape == (2, len(x)) and same_bits(rows[0, :m], got) and same_bits(rows[1], rows[0]) and not rows[:, m:].any()
    if HOSTSTUB:
        return
    bp, bl = tc.bar(name)
    p, l2 = tc.errors(got, want)
    print(f"pitchshift/{name}: {len(x)} -> {m} samples, peak-rel {p:.3e} (bar {bp:.1e}), l2-rel {l2:.3e} (bar {bl:.1e})")
    assert p <= bp and l2 <= bl, (name, p, bp, l2, bl)
    assert_parity(got, want, tol=max(bp, bl), what=f"pitchshift/{name}")


@pytest.mark.parametrize("n,semi,written", [(3001, -12, 3001), (3000, -5, 2999), (3000, -12, 3000), (3001, 12, 3001)])
def test_length_rule(n, semi, written, lib):
    """n = 3001 at -12 semitones: the resampled length is 3002, exactly 3001 samples are written -- the word behind the
    destination stays; 3000 at -5: 2999, the last sample stays as the caller gave it.  Host-pointer and device call alike."""
    import torch
    st, obj = tc.new(lib, dict(exp=8, hop=64), "pitchShift")
    assert st == 0
    x = signal(n, seed=9)
    out = tc.shift(lib, obj, x, semi, fill=3.25)  # n + 8 words of 3.25
    od = torch.full((2, n + 8), 7.5, device="cuda")
    xd = torch.from_numpy(x).cuda()
    ret = lib.pitchShiftObj_pitchShiftBatchDevice(obj, semi, xd.data_ptr(), 1, n, n, od.data_ptr(), n + 8, None)
    torch.cuda.synchronize()
    lib.pitchShiftObj__free(obj)
    od = od.cpu().numpy()
    assert ret == written == tc.pitch_length(n, semi)
    if HOSTSTUB:
        return
    assert (out[:written] != np.float32(3.25)).any() and (out[written:] == np.float32(3.25)).all()
    assert tc.same_bits(od[0, :written], out[:written]) and (od[0, written:] == 7.5).all() and (od[1] == 7.5).all()


def test_strided_batch_in_chunks_is_bitwise_the_single_calls(lib):
    import torch
    n, clips, semi = 3000, 5, 3
    o = af.PitchShift(8, 64)
    xs = torch.full((clips + 1, n + 13), float("nan"), device="cuda")
    for k in range(clips):
        xs[k, :n] = torch.from_numpy(signal(n, seed=60 + k))
    single = [o.pitch_shift_batch_device(xs[k:k + 1, :n].contiguous(), semi)[0].cpu().numpy() for k in range(clips)]
    m = tc.pitch_length(n, semi)
    p = tc.Plan()
    assert lib.afx_timestretch_plan(8, 64, C.c_float(tc.semitone_rate(semi)), n, clips, 0, C.byref(p), None, None) == 0
    o.set_scratch_limit(2 * p.scratchBytes + 100)  # two clips of the time stretch, many of the resampler's rows
    out = torch.full((clips + 1, n + 7), 7.5, device="cuda")
    got = o.pitch_shift_batch_device(xs[:clips, :n], semi, out=out[:clips])
    assert got.shape == (clips, m)
    o.set_scratch_limit(2 * 4 * (n + 4))  # less than two rows of each kind: one clip per chunk of the object's own scratch
    out2 = torch.full((clips + 1, n + 7), 7.5, device="cuda")
    o.pitch_shift_batch_device(xs[:clips, :n], semi, out=out2[:clips])
    out, out2 = out.cpu().numpy(), out2.cpu().numpy()
    for k in range(clips):
        assert same_bits(out[k, :m], single[k]) and same_bits(out2[k, :m], single[k]), k
    assert HOSTSTUB or ((out[:clips, m:] == 7.5).all() and (out[clips] == 7.5).all() and same_bits(out, out2))


def test_refusals(lib):
    """|nSemitone| = 13 writes nothing; NULL handle and arrays, batch <= 0, short strides, n < N: a status or a recorded
    failure, nothing written"""
    import torch
    st, obj = tc.new(lib, dict(exp=8, hop=64), "pitchShift")
    assert st == 0
    x, out = signal(3000), np.full(3008, 3.25, np.float32)
    f = lib.pitchShiftObj_pitchShift
    before = lib.afx_error_count()
    f(obj, 32000, 13, tc.ptr(x), 3000, tc.ptr(out))
    f(obj, 32000, -13, tc.ptr(x), 3000, tc.ptr(out))
    assert lib.afx_error_count() == before and (out == np.float32(3.25)).all()
    for args in ((None, 32000, 3, tc.ptr(x), 3000, tc.ptr(out)), (obj, 32000, 3, None, 3000, tc.ptr(out)),
                 (obj, 32000, 3, tc.ptr(x), 3000, None), (obj, 32000, 3, tc.ptr(x), 255, tc.ptr(out)), (obj, 32000, 3, tc.ptr(x), 0, tc.ptr(out))):
        before = lib.afx_error_count()
        f(*args)
        assert lib.afx_error_count() > before and (out == np.float32(3.25)).all(), args[2:5:2]
    xd, od = torch.from_numpy(x).cuda(), torch.full((3008,), 7.5, device="cuda")
    g = lib.pitchShiftObj_pitchShiftBatchDevice
    xp, op = xd.data_ptr(), od.data_ptr()
    for args in ((None, 3, xp, 1, 3000, 3000, op, 3000), (obj, 3, None, 1, 3000, 3000, op, 3000), (obj, 3, xp, 1, 3000, 3000, None, 3000),
                 (obj, 3, xp, 0, 3000, 3000, op, 3000), (obj, 3, xp, 2, 1500, 1499, op, 1500), (obj, 3, xp, 2, 1500, 1500, op, 1400),
                 (obj, 3, xp, 1, 255, 255, op, 3000)):
        assert g(*args, None) == -6, args[1:]
    assert g(obj, 13, xp, 1, 3000, 3000, op, 3000, None) == 0
    torch.cuda.synchronize()
    assert HOSTSTUB or bool((od == 7.5).all())
    lib.pitchShiftObj__free(obj)
    lib.pitchShiftObj__free(None)
    with pytest.raises(ValueError):
        af.PitchShift(8, 64).pitch_shift(x, 13)
