"""GPU parity of the pitch-estimation-filter tracker (af.PitchPEF, mir/_pitch_pef.h): the fixture of the compiled
reference's outputs by the rule of tests/pitch_pef_check.py through the host-pointer call and through pitchBatchDevice,
fresh inputs against the compiled reference when oracle/_ref is present, the curve export, batch == per-clip calls bitwise
with guards, silent frames, streaming in pieces == one call, refusals, set_filter_params, and two objects of different
sizes interleaved on one stream."""
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import pitch_pef_cases as pc
from tests import pitch_pef_restate as pr
from tests.conftest import HOSTSTUB, parity_log
from tests.pitch_cases import signal
from tests.pitch_pef_check import check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "pitch_pef.npz"))


@pytest.fixture(scope="module")
def lib():
    return pc.bind_device(af.get_lib())


def same_bits(a, b):
    return HOSTSTUB or np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _obj(sr, lo, hi, cut, r, hop, window, alpha, beta, gamma):
    return af.PitchPEF(samplate=sr, low_fre=lo, high_fre=hi, cut_fre=cut, radix2_exp=r, slide_length=hop,
                       window_type=af.WindowType(window), alpha=alpha, beta=beta, gamma=gamma)


def _tables(lib, name):
    c = pc.CASES[name]
    st, t = pc.plan(lib, *pc.ctor_args(name))
    assert st == 0
    t["lin"] = pc.lin_table(c[0], 1 << c[4])
    return t


def _index(lg, mn, fre):
    return mn + int(np.flatnonzero(lg[mn:].view(np.uint32) == np.float32(fre).view(np.uint32))[0])


@pytest.mark.parametrize("name", list(pc.CASES))
def test_fixture_case(name, gold, lib):
    """every case through pitch() with host pointers and through pitchBatchDevice: the acceptance rule, both routes bit-equal;
    the curve against the restatement; dValue == curve[index] exactly"""
    import torch
    c = pc.CASES[name]
    x = pc.case_input(name)
    fre = pc.run_case(lib, name)
    o = _obj(*pc.ctor_args(name))
    xd = torch.from_numpy(x).cuda()[None]
    dfre, dval = (t[0].cpu().numpy() for t in o.pitch_batch_device(xd))
    curve = o.curve_batch_device(xd)[0].cpu().numpy()
    tables = _tables(lib, name)
    mn, mx, pad = (int(v) for v in gold[name + "/plan"])
    assert (o.min_index, o.max_index, o.filter_pad_num, o.log_length) == (mn, mx, pad, 2 << c[4])
    frames = pr.pitch(x, tables, c[4], c[5], pad, mn, mx)
    assert (len(fre), curve.shape) == (len(frames), (len(frames), mx + 1))
    assert same_bits(fre, dfre), name
    if HOSTSTUB:
        return
    w = check_case(name, frames, gold[name + "/eps"], gold[name + "/fre"], fre, tables["lg"], mn, curve)
    parity_log(f"pitch_pef/{name}", w["worst_curve"] * 1e-5, 1e-5, "pitch_pef: worst curve error / its bar, scaled to 1e-5",
               {"explained": w["explained"], "frames": w["frames"]})
    for t in range(len(fre)):
        i = _index(tables["lg"], mn, fre[t])
        assert same_bits(dval[t:t + 1], curve[t, i:i + 1]), (name, t, i)
    if name in pc.CURVES:  # the stored rows are the restatement's
        c64 = gold[name + "/curve64"]
        for t, f in enumerate(frames):
            assert np.array_equal(c64[t], f["curve"].astype(np.float32)), (name, t)


@pytest.mark.parametrize("name", ["r6_sr8k", "r8_stack", "r9_oddhop", "r10_bighop", "r11_sr44k", "p0_beta1_r9", "pN_r8"])
def test_fresh_input_against_the_compiled_reference(name, lib):
    """inputs with a seed the fixture has not seen, noise added"""
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    from tests.golden.make_pitch_pef_golden import reference_case
    c = pc.CASES[name]
    x = signal(c[10], c[11], c[0], seed=977) + 0.01 * signal("noise", c[11], c[0], seed=978)
    ref_fre, eps, frames, f, tables = reference_case(pc.bind(ref.lib()), name, x)
    st, obj = pc.new(lib, *pc.ctor_args(name))
    assert st == 0
    fre = pc.call(lib, obj, x)
    lib.pitchPEFObj_free(obj)
    if HOSTSTUB:
        return
    w = check_case(f"fresh/{name}", frames, eps, ref_fre, fre, tables["lg"], f["minIndex"])
    parity_log(f"pitch_pef/fresh/{name}", float(w["explained"]), max(1, w["frames"] // 100), "pitch_pef: explained frames / cap")


def test_batch_equals_single_calls_and_writes_nothing_else(lib):
    """3 clips, clipStride > dataLength, outStride > frames, 4-byte-misaligned base pointers, outputs pre-filled with NaN"""
    import torch
    sr, r, hop = 16000, 9, 128
    n, clips, stride = 512 + 128 * 5 + 5, 3, 512 + 128 * 5 + 17
    buf = np.zeros(clips * stride + 1, np.float32)
    xs = buf[1:].reshape(clips, stride)
    for c, sig in enumerate(("tone:330", "stack:196", "glide")):
        xs[c, :n] = signal(sig, n, sr, seed=70 + c)
    o = _obj(sr, 40.0, 2000.0, 4000.0, r, hop, pc.HAMM, 10.0, 0.5, 1.8)
    T = o.cal_time_length(n)
    single = [o.pitch(xs[c, :n].copy()) for c in range(clips)]
    d = torch.from_numpy(buf).cuda()
    assert (d.data_ptr() + 4) % 16 == 4
    pitch_stride, guard = T + 3, 64
    f = torch.full((1 + clips * pitch_stride + guard,), float("nan"), device="cuda")
    v = torch.full_like(f, float("nan"))
    st = lib.pitchPEFObj_pitchBatchDevice(o._obj, d.data_ptr() + 4, clips, n, stride, f.data_ptr() + 4, v.data_ptr() + 4, pitch_stride,
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
    assert lib.pitchPEFObj_curveBatchDevice(o._obj, d.data_ptr() + 4, clips, n, stride, cv.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    ch = cv.cpu().numpy()
    assert not np.isnan(ch[:-guard]).any() and np.isnan(ch[-guard:]).all()
    one = o.curve_batch_device(torch.from_numpy(xs[1, :n].copy()).cuda()[None])[0].cpu().numpy()
    assert same_bits(ch[:-guard].reshape(clips, T, -1)[1], one)


@pytest.mark.parametrize("name", ["zero_r9", "wide_cut_r10"])
def test_silent_frames_give_min_index(name, lib, gold):
    c = pc.CASES[name]
    x = pc.case_input(name)
    fre = pc.run_case(lib, name)
    lg = _tables(lib, name)["lg"]
    N, hop = 1 << c[4], c[5]
    silent = [t for t in range(len(fre)) if not x[t * hop:t * hop + N].any()]
    assert silent, name
    if not HOSTSTUB:
        assert all(fre[t] == lg[int(gold[name + "/plan"][0])] for t in silent), fre


@pytest.mark.parametrize("r,hop", [(8, 100), (8, 300)])
def test_streaming_in_three_uneven_pieces(r, hop, lib):
    sr, N = 16000, 1 << r
    x = signal("glide", N + hop * 9 + 31, sr, seed=90)
    st, one = pc.new(lib, sr, 60.0, 2000.0, None, r, hop)
    assert st == 0
    whole = pc.call(lib, one, x)
    lib.pitchPEFObj_free(one)
    st, obj = pc.new(lib, sr, 60.0, 2000.0, None, r, hop, cont=1)
    assert st == 0
    parts = [pc.call(lib, obj, p) for p in np.split(x, [len(x) // 5, len(x) // 5 + 2 * N + 3])]
    lib.pitchPEFObj_free(obj)
    got = np.concatenate(parts)
    assert len(got) == len(whole) and same_bits(got, whole)


def test_refusals_on_the_device_path(lib):
    import torch
    sr, r, hop = 16000, 9, 128
    n = 512 + 128 * 3
    x = torch.from_numpy(signal("tone:330", n, sr, seed=3)).cuda()
    out = torch.full((16,), 5.0, device="cuda")
    fn, cv = lib.pitchPEFObj_pitchBatchDevice, lib.pitchPEFObj_curveBatchDevice
    s = torch.cuda.current_stream().cuda_stream
    st, cont = pc.new(lib, sr, 40.0, 2000.0, None, r, hop, cont=1)
    assert st == 0
    assert fn(cont, x.data_ptr(), 1, n, n, out.data_ptr(), None, 16, s) == -4
    lib.pitchPEFObj_free(cont)
    for bad in (5, 13):
        st, o = pc.new(lib, r=bad)
        assert st == -100 and not o
    st, o = pc.new(lib, sr, 100.0, 2000.0, 2000.0, r, hop)  # cutFre == highFre: maxIndex stays 0
    assert st == -6 and not o
    st, o = pc.new(lib, sr, 40.0, 2000.0, None, r, hop)
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
    lib.pitchPEFObj_free(o)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5).all(), "a refused / empty call wrote"


def test_set_filter_params_leaves_results_unchanged():
    x = pc.case_input("r8_stack")
    o = _obj(*pc.ctor_args("r8_stack"))
    before = o.pitch(x)
    o.set_filter_params(5.0, 0.7, 2.5)
    assert (o.alpha, o.beta, o.gamma) == (5.0, 0.7, 2.5)  # the wrapper remembers them, as the reference's does
    assert same_bits(o.pitch(x), before)
    with pytest.raises(ValueError):
        o.set_filter_params(5.0, 0.7, 1.0)


def test_two_objects_interleaved_on_one_stream():
    """objects of different N share no state: calls queued alternately on one stream equal the calls made alone"""
    import torch
    a, b = _obj(*pc.ctor_args("r8_stack")), _obj(*pc.ctor_args("r11_sr44k"))
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
