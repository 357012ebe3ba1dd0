"""GPU parity of the resampler (af.Resample, af.WindowResample; dsp/resample_algorithm.h) against the compiled reference
(oracle/_ref when present, else tests/golden/resample.npz) at 1e-5 peak- and L2-relative: every case of
tests/resample_cases.py through the host-pointer call and through resampleBatchDevice (bit-equal), isScale, window tables in
LDS and in global memory, a strided batch with guards, streaming in pieces, the ratio sequence on a live object, refusals."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import resample_cases as rc
from tests.conftest import HOSTSTUB, assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    af.get_lib()  # (loads the HIP runtime in the order the package wants)
    return rc.bind(C.CDLL(af.LIB_PATH))  # a handle of its own: the wrapper classes set other argument types on theirs


def same_bits(a, b):
    return HOSTSTUB or (np.shape(a) == np.shape(b) and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)))


def _wrapper(name):
    """the case's object through the Python classes"""
    c = rc.CASES[name]
    if "qual" in c:
        o = af.Resample(af.ResampleQualityType(c["qual"]), is_scale=bool(c.get("scale")))
    else:
        z, nb, wt, val, ro = c["win"]
        o = af.WindowResample(z, nb, af.WindowType(wt), val, ro, is_scale=bool(c.get("scale")))
    if "rates" in c:
        o.set_samplate(*c["rates"])
    else:
        o.set_samplate_ratio(c["ratio"])
    return o


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_meets_the_reference(name, lib):
    """the host-pointer call into a non-zero destination (overwrite semantics; nothing behind the length is written), the
    input unmodified, the device call bit-equal to it, both at 1e-5 of the reference"""
    import torch
    x = rc.case_input(name)
    keep = x.copy()
    want, sel = rc.expected(name)
    st, obj = rc.new(lib, name)
    assert st == 0 and obj, (name, st, af.last_error())
    got = rc.call(lib, obj, x, fill=3.25)
    lib.resampleObj_free(obj)
    assert np.array_equal(x, keep)
    o = _wrapper(name)
    assert o.cal_data_length(len(x)) == len(got)
    dev = o.resample_batch_device(torch.from_numpy(x).cuda()[None])[0].cpu().numpy()
    assert same_bits(dev, got) and same_bits(o.resample(x), got), name
    if sel is not None:
        got = got[sel]
    print(f"resample/{name}: {len(x)} -> {len(dev)} samples", end="")
    if len(want) and not HOSTSTUB:
        d = got.astype(np.float64) - want
        print(f", peak-rel {np.abs(d).max() / np.abs(want).max():.3e}, l2-rel {np.linalg.norm(d) / np.linalg.norm(want):.3e}")
    else:
        print()
    if len(want) == 0:  # (fewer samples than one output)
        assert len(got) == 0
        return
    assert_parity(got, want, what=f"resample/{name}")


def test_batch_of_strided_clips_is_bitwise_the_single_calls(lib):
    """5 clips, clipStride > dataLength, outStride > the output length: rows bitwise the single-clip results, the padding
    between the output rows and the input untouched; groups of 4 + 1 clips and two tiles of outputs"""
    import torch
    name, n, clips = "441_16_mid", 1500, 5
    o = _wrapper(name)
    m = o.cal_data_length(n)
    assert m == 544  # (more than one tile of 512 outputs)
    xs = torch.zeros((clips, n + 17), dtype=torch.float32)
    for c in range(clips):
        xs[c, :n] = torch.from_numpy(rc.signal(n, seed=40 + c))
    xd = xs.cuda()
    out = torch.full((clips + 1, m + 5), 7.5, dtype=torch.float32, device="cuda")
    got = o.resample_batch_device(xd[:, :n], out=out[:clips])
    assert got.shape == (clips, m) and got.data_ptr() == out.data_ptr()
    res = out.cpu().numpy()
    for c in range(clips):
        assert same_bits(res[c, :m], o.resample(xs[c, :n].numpy())), c
    if not HOSTSTUB:
        assert (res[:clips, m:] == 7.5).all() and (res[clips] == 7.5).all()
    assert torch.equal(xd.cpu(), xs)
    # leading axes of a numpy input go through the same batched call
    assert same_bits(o.resample(xs[:, :n].numpy().reshape(5, 1, n)), res[:clips, :m].reshape(5, 1, m))


def test_streaming_in_pieces_is_the_reference_fed_the_same_pieces(lib):
    """isContinue: (dataLength - dataLength % q) p / q outputs per piece; no history and no remainder is carried, so the
    pieces are NOT the one-shot call"""
    got, want = rc.run_pieces(lib), rc.expected_pieces()
    assert [len(g) for g in got] == [len(w) for w in want] == [320, 0, 1600]
    for k, (g, w) in enumerate(zip(got, want)):
        if len(w):
            assert_parity(g, w, what=f"resample/pieces/{k}")
    st, obj = rc.new(lib, "441_16_best")
    x = rc.signal(sum(rc.PIECES), seed=77)
    whole = rc.call(lib, obj, x)
    assert len(whole) == 1976 != sum(len(g) for g in got)
    # enableContinue(1) on a live object: the other length rule and no batch; (0): back
    lib.resampleObj_enableContinue(obj, 1)
    assert lib.resampleObj_calDataLength(obj, 1000) == 320
    assert lib.resampleObj_resampleBatchDevice(obj, 1, 1, 1000, 1000, 1, 1000, None) == -4
    lib.resampleObj_enableContinue(obj, 0)
    assert lib.resampleObj_calDataLength(obj, 1000) == 362
    assert same_bits(rc.call(lib, obj, x), whole)
    # isContinue with q <= 1: nothing is produced
    lib.resampleObj_enableContinue(obj, 1)
    lib.resampleObj_setSamplate(obj, 16000, 32000)
    assert lib.resampleObj_calDataLength(obj, 1000) == 0 and len(rc.call(lib, obj, x[:1000], fill=2.0)) == 0
    lib.resampleObj_setSamplateRatio(obj, 0.4)
    assert lib.resampleObj_calDataLength(obj, 1000) == 0 and len(rc.call(lib, obj, x[:1000], fill=2.0)) == 0
    lib.resampleObj_free(obj)


def test_ratio_sequence_on_a_live_object(lib):
    """0.5 -> 16000 / 44100 -> 2.0 -> 0.7123 on ONE object: the table is divided and multiplied in place and uploaded again;
    the result is the reference's after the same sequence"""
    got, want = rc.run_sequence(lib), rc.expected_sequence()
    assert [len(g) for g in got] == [1500, 1088, 6000, 2136]
    for k, (g, w) in enumerate(zip(got, want)):
        assert_parity(g, w, what=f"resample/sequence/{k}")


def test_refusals(lib):
    f = lib.resampleObj_resampleBatchDevice
    st, obj = rc.new(lib, "441_16_fast")
    assert st == 0
    import torch
    x = torch.zeros((2, 100), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 40), dtype=torch.float32, device="cuda")
    assert f(obj, x.data_ptr(), 2, 100, 100, out.data_ptr(), 40, None) == 36
    assert f(obj, x.data_ptr(), 2, 100, 99, out.data_ptr(), 40, None) == -6
    assert f(obj, x.data_ptr(), 2, 100, 100, out.data_ptr(), 35, None) == -6
    assert f(obj, None, 2, 100, 100, out.data_ptr(), 40, None) == -6
    assert f(obj, x.data_ptr(), 2, 100, 100, None, 40, None) == -6
    assert f(obj, x.data_ptr(), 0, 100, 100, out.data_ptr(), 40, None) == -6
    assert f(obj, x.data_ptr(), 2, 0, 100, out.data_ptr(), 40, None) == -6
    assert f(None, x.data_ptr(), 2, 100, 100, out.data_ptr(), 40, None) == -6
    assert f(obj, x.data_ptr(), 2, 2, 100, out.data_ptr(), 40, None) == 0  # 2 samples: no output
    before = af.get_lib().afx_error_count()
    h = np.zeros(8, np.float32)
    assert lib.resampleObj_resample(obj, None, 8, h.ctypes.data_as(C.c_void_p)) == -6
    assert lib.resampleObj_resample(obj, h.ctypes.data_as(C.c_void_p), 0, h.ctypes.data_as(C.c_void_p)) == -6
    assert lib.resampleObj_resample(None, h.ctypes.data_as(C.c_void_p), 8, h.ctypes.data_as(C.c_void_p)) == -6
    assert af.get_lib().afx_error_count() >= before + 3 and "NULL object" in af.last_error()
    # a ratio below one table entry per tap
    lib.resampleObj_setSamplateRatio(obj, 0.001)
    big, few = np.zeros(100000, np.float32), np.zeros(200, np.float32)
    assert lib.resampleObj_calDataLength(obj, len(big)) == 100
    assert lib.resampleObj_resample(obj, big.ctypes.data_as(C.c_void_p), len(big), few.ctypes.data_as(C.c_void_p)) == -6
    torch.cuda.synchronize()
    lib.resampleObj_free(obj)
    lib.resampleObj_free(None)
    with pytest.raises(RuntimeError, match="status -4"):
        af.WindowResample(zero_num=1 << 16, nbit=9)  # 2^25 entries
