"""GPU parity of the NCF and cepstrum pitch trackers (af.PitchNCF, af.PitchCEP; mir/_pitch_ncf.h, mir/_pitch_cep.h): the
fixture of the compiled reference's outputs by the rule of tests/pitch_lag_check.py through the host-pointer call and
through pitchBatchDevice, fresh inputs against the compiled reference when oracle/_ref is present, the curve export,
batch == per-clip calls bitwise with guards, silent frames, streaming in pieces == one call, refusals, and an NCF and a CEP
object of different sizes interleaved on one stream."""
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import pitch_lag_cases as pc
from tests import pitch_lag_restate as pr
from tests.conftest import HOSTSTUB, parity_log
from tests.pitch_cases import signal
from tests.pitch_lag_check import check_case, index_of

pytestmark = pytest.mark.gpu
CLS = {"NCF": af.PitchNCF, "CEP": af.PitchCEP}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "pitch_lag.npz"))


@pytest.fixture(scope="module")
def lib():
    return pc.bind_device(af.get_lib())


def same_bits(a, b):
    return HOSTSTUB or np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _obj(kind, sr, lo, hi, r, hop, window=None):
    kw = {} if window is None else {"window_type": af.WindowType(window)}
    return CLS[kind](samplate=sr, low_fre=lo, high_fre=hi, radix2_exp=r, slide_length=hop, **kw)


def _noisy(sig, n, sr, seed):
    """a signal with a noise floor: no bin of its spectrum is empty under the cepstrum's log"""
    return signal(sig, n, sr, seed=seed) + 0.01 * signal("noise", n, sr, seed=seed + 1)


@pytest.mark.parametrize("name", list(pc.CASES))
@pytest.mark.parametrize("kind", pc.KINDS)
def test_fixture_case(kind, name, gold, lib):
    """every case through pitch() with host pointers and through pitchBatchDevice: the acceptance rule, both routes bit-equal;
    the curve against the restatement; dValue == curve[index] exactly"""
    import torch
    c = pc.CASES[name]
    sr, r, hop = c[0], c[3], c[4]
    x = pc.case_input(name)
    fre = pc.run_case(lib, kind, name)
    o = _obj(kind, *pc.ctor_args(name))
    xd = torch.from_numpy(x).cuda()[None]
    dfre, dval = (t[0].cpu().numpy() for t in o.pitch_batch_device(xd))
    curve = o.curve_batch_device(xd)[0].cpu().numpy()
    st, p = pc.plan(lib, kind, *pc.ctor_args(name))
    mn, mx = (int(v) for v in gold[f"{kind}/{name}/plan"])
    assert st == 0 and (o.min_index, o.max_index) == (mn, mx)
    frames = pr.pitch(kind, x, pc.restate_window(p), r, hop, mn, mx)
    assert (len(fre), curve.shape) == (len(frames), (len(frames), mx + 1))
    assert same_bits(fre, dfre), name
    if HOSTSTUB:
        return
    w = check_case(f"{kind}/{name}", frames, gold[f"{kind}/{name}/eps"], gold[f"{kind}/{name}/fre"], fre, sr, curve)
    parity_log(f"pitch_lag/{kind}/{name}", w["worst_curve"] * 1e-5, 1e-5, "pitch_lag: worst curve error / its bar, scaled to 1e-5",
               {"explained": w["explained"], "frames": w["frames"]})
    for t in range(len(fre)):
        i = index_of(fre[t], sr)
        assert same_bits(dval[t:t + 1], curve[t, i:i + 1]), (kind, name, t, i)
    if name in pc.CURVES:  # the stored rows are the restatement's
        c64 = gold[f"{kind}/{name}/curve64"]
        for t, f in enumerate(frames):
            assert np.array_equal(c64[t], f["curve"].astype(np.float32), equal_nan=True), (name, t)


@pytest.mark.parametrize("name", ["r6_sr8k", "r8_stack", "r9_oddhop", "r10_bighop", "r11_sr44k", "rect_r8"])
@pytest.mark.parametrize("kind", pc.KINDS)
def test_fresh_input_against_the_compiled_reference(kind, name, lib):
    """inputs with a seed the fixture has not seen, noise added"""
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    from tests.golden.make_pitch_lag_golden import reference_case
    c = pc.CASES[name]
    x = _noisy(c[6], pc.data_length(name), c[0], 977)
    ref_fre, eps, frames, f, window = reference_case(pc.bind(ref.lib()), kind, name, x)
    st, obj = pc.new(lib, kind, *pc.ctor_args(name))
    assert st == 0
    fre = pc.call(lib, kind, obj, x)
    pc.fn(lib, kind, "free")(obj)
    if HOSTSTUB:
        return
    w = check_case(f"fresh/{kind}/{name}", frames, eps, ref_fre, fre, c[0])
    parity_log(f"pitch_lag/fresh/{kind}/{name}", float(w["explained"]), max(1, w["frames"] // 100), "pitch_lag: explained frames / cap")


@pytest.mark.parametrize("kind", pc.KINDS)
def test_batch_equals_single_calls_and_writes_nothing_else(kind, lib):
    """3 clips, clipStride > dataLength, outStride > frames, 4-byte-misaligned base pointers, outputs pre-filled with NaN"""
    import torch
    sr, r, hop = 16000, 9, 128
    n, clips, stride = 512 + 128 * 5 + 5, 3, 512 + 128 * 5 + 17
    buf = np.zeros(clips * stride + 1, np.float32)
    xs = buf[1:].reshape(clips, stride)
    for c, sig in enumerate(("tone:330", "stack:196", "glide")):
        xs[c, :n] = _noisy(sig, n, sr, 70 + 2 * c)
    o = _obj(kind, sr, 40.0, 2000.0, r, hop, pc.HAMM)
    T = o.cal_time_length(n)
    single = [o.pitch(xs[c, :n].copy()) for c in range(clips)]
    d = torch.from_numpy(buf).cuda()
    assert (d.data_ptr() + 4) % 16 == 4
    pitch_stride, guard = T + 3, 64
    f = torch.full((1 + clips * pitch_stride + guard,), float("nan"), device="cuda")
    v = torch.full_like(f, float("nan"))
    st = pc.fn(lib, kind, "pitchBatchDevice")(o._obj, d.data_ptr() + 4, clips, n, stride, f.data_ptr() + 4, v.data_ptr() + 4, pitch_stride,
                                              torch.cuda.current_stream().cuda_stream)
    assert st == 0, af.last_error()
    torch.cuda.synchronize()
    fh, vh = f.cpu().numpy(), v.cpu().numpy()
    assert np.isnan(fh[0]) and np.isnan(vh[0]), "wrote in front of the output"
    fh, vh = fh[1:], vh[1:]
    rows_f, rows_v = fh[:clips * pitch_stride].reshape(clips, pitch_stride), vh[:clips * pitch_stride].reshape(clips, pitch_stride)
    for c in range(clips):
        assert same_bits(rows_f[c, :T], single[c]), c
    assert not np.isnan(rows_f[:, :T]).any() and not np.isnan(rows_v[:, :T]).any(), "a frame entry was not written"
    assert np.isnan(rows_f[:, T:]).all() and np.isnan(rows_v[:, T:]).all(), "wrote beyond a row's frames"
    assert np.isnan(fh[clips * pitch_stride:]).all() and np.isnan(vh[clips * pitch_stride:]).all(), "wrote into the guard"
    # the curve rows of the batch, with a guard behind them
    cv = torch.full((clips * T * (o.max_index + 1) + guard,), float("nan"), device="cuda")
    assert pc.fn(lib, kind, "curveBatchDevice")(o._obj, d.data_ptr() + 4, clips, n, stride, cv.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    ch = cv.cpu().numpy()
    assert not np.isnan(ch[:-guard]).any() and np.isnan(ch[-guard:]).all()
    one = o.curve_batch_device(torch.from_numpy(xs[1, :n].copy()).cuda()[None])[0].cpu().numpy()
    assert same_bits(ch[:-guard].reshape(clips, T, -1)[1], one)


@pytest.mark.parametrize("name", ["zero_r9", "step_r10"])
@pytest.mark.parametrize("kind", pc.KINDS)
def test_silent_frames_give_min_index(kind, name, lib, gold):
    """a silent clip and a clip that is silent in parts: the frames without a sample give samplate / (minIndex + 1)"""
    c = pc.CASES[name]
    x = pc.case_input(name)
    fre = pc.run_case(lib, kind, name)
    N, hop = 1 << c[3], c[4]
    silent = [t for t in range(len(fre)) if not x[t * hop:t * hop + N].any()]
    assert silent, name
    if not HOSTSTUB:
        want = pr.fre_of(int(gold[f"{kind}/{name}/plan"][0]), c[0])
        assert all(fre[t] == want for t in silent), fre


@pytest.mark.parametrize("r,hop", [(8, 100), (8, 300)])
@pytest.mark.parametrize("kind", pc.KINDS)
def test_streaming_in_three_uneven_pieces(kind, r, hop, lib):
    sr, N = 16000, 1 << r
    x = _noisy("glide", N + hop * 9 + 31, sr, 90)
    st, one = pc.new(lib, kind, sr, 80.0, 2000.0, r, hop)
    assert st == 0
    whole = pc.call(lib, kind, one, x)
    pc.fn(lib, kind, "free")(one)
    st, obj = pc.new(lib, kind, sr, 80.0, 2000.0, r, hop, cont=1)
    assert st == 0
    parts = [pc.call(lib, kind, obj, p) for p in np.split(x, [len(x) // 5, len(x) // 5 + 2 * N + 3])]
    pc.fn(lib, kind, "free")(obj)
    got = np.concatenate(parts)
    assert len(got) == len(whole) == 10 and same_bits(got, whole)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_refusals_on_the_device_path(kind, lib):
    import torch
    sr, r, hop = 16000, 9, 128
    n = 512 + 128 * 3
    x = torch.from_numpy(signal("tone:330", n, sr, seed=3)).cuda()
    out = torch.full((16,), 5.0, device="cuda")
    fn, cv = pc.fn(lib, kind, "pitchBatchDevice"), pc.fn(lib, kind, "curveBatchDevice")
    s = torch.cuda.current_stream().cuda_stream
    st, cont = pc.new(lib, kind, sr, 40.0, 2000.0, r, hop, cont=1)
    assert st == 0
    assert fn(cont, x.data_ptr(), 1, n, n, out.data_ptr(), None, 16, s) == -4
    pc.fn(lib, kind, "free")(cont)
    for bad in (5, 13):
        st, o = pc.new(lib, kind, r=bad)
        assert st == -100 and not o
    st, o = pc.new(lib, kind, 8000, 32.0, 2000.0, 6, 16)  # maxIndex 250 of N = 64
    assert st == -6 and not o
    st, o = pc.new(lib, kind, sr, 40.0, 2000.0, r, hop)
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
    pc.fn(lib, kind, "free")(o)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5).all(), "a refused / empty call wrote"


def test_two_objects_interleaved_on_one_stream():
    """an NCF and a CEP object of different N share no state: calls queued alternately on one stream equal the calls made
    alone"""
    import torch
    a, b = _obj("NCF", *pc.ctor_args("r8_stack")), _obj("CEP", *pc.ctor_args("r11_sr44k"))
    xa = torch.from_numpy(pc.case_input("r8_stack")).cuda()[None]
    xb = torch.from_numpy(pc.case_input("r11_sr44k")).cuda()[None]
    alone_a, alone_b = a.pitch_batch_device(xa), b.pitch_batch_device(xb)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = [(a.pitch_batch_device(xa, s), b.pitch_batch_device(xb, s)) for _ in range(3)]
    s.synchronize()
    for ra, rb in outs:
        for got, want in zip(ra + rb, alone_a + alone_b):
            assert same_bits(got.cpu().numpy(), want.cpu().numpy())
