"""GPU parity of the harmonic ratio (af.HarmonicRatio; mir/harmonicRatio_algorithm.h): the fixture of the compiled reference's
outputs by the rule of tests/harmonic_ratio_check.py through the host-pointer call and through harmonicRatioBatchDevice (bit-
equal), dValue against the exported curve and dLag, batch == per-clip calls bitwise with guards and no minIndex inherited
across a clip boundary, a call split in two against the compiled reference, the optional outputs NULL, refusals, and the
object interleaved with a PitchNCF object of another size on one stream."""
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import harmonic_ratio_cases as hc
from tests import harmonic_ratio_restate as hr
from tests.conftest import HOSTSTUB, parity_log
from tests.harmonic_ratio_check import check_case, reference_eps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "harmonic_ratio.npz"))


@pytest.fixture(scope="module")
def lib():
    return hc.bind_device(af.get_lib())


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return HOSTSTUB or (a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def _obj(name):
    c = hc.CASES[name]
    return af.HarmonicRatio(samplate=c[0], low_fre=c[1], radix2_exp=c[2], slide_length=c[3])


def _consistent(name, value, lag, first, curve, mx):
    """dValue against the exported curve and dLag: zeros at and below first, the first maximum above it, the entry itself at the
    ends of the range and the reference's parabola through the three entries (float32 / float64 as in flux_util.c:771-780)
    elsewhere"""
    f32, f64 = np.float32, np.float64
    for t in range(len(value)):
        f, row = int(first[t]), curve[t]
        assert not row[:f + 1].any(), (name, t)
        if f + 1 >= mx:
            assert lag[t] == -1 and value[t] == 0, (name, t)
            continue
        j = f + 1 + int(np.argmax(row[f + 1:]))  # numpy's argmax is the first maximum
        assert lag[t] == j, (name, t, lag[t], j)
        if j in (f + 1, mx - 1):
            assert same_bits(value[t:t + 1], row[j:j + 1]), (name, t)
        else:
            v1, v2, v3 = (f32(v) for v in row[j - 1:j + 2])
            p = f32(f64(v3 - v1) / (f64(f32(2) * (f32(2) * v2 - v3 - v1)) + 1e-16))
            want = f32(f64(v2) - 0.25 * f64(v1 - v3) * f64(p))
            assert same_bits(value[t:t + 1], np.array([want])), (name, t, value[t], want)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_fixture_case(name, gold, lib):
    """every case through harmonicRatio() with host pointers and through harmonicRatioBatchDevice: both routes bit-equal, the
    acceptance rule, dValue consistent with the exported curve and dLag"""
    import torch
    c = hc.CASES[name]
    x = hc.case_input(name)
    value = hc.run_case(lib, name)
    o = _obj(name)
    xd = torch.from_numpy(x).cuda()[None]
    dval, dlag, dfirst = (t[0].cpu().numpy() for t in o.harmonic_ratio_batch_device(xd))
    curve = o.curve_batch_device(xd)[0].cpu().numpy()
    st, p = hc.plan(lib, *hc.ctor_args(name))
    N, L, slide, mx = (int(v) for v in gold[name + "/plan"])
    assert st == 0 and (o.window_length, o.fft_length, o.max_length) == (N, L, mx)
    assert o.cal_time_length(len(x)) == c[5] == len(value) and curve.shape == (c[5], mx)
    assert same_bits(value, dval), name
    assert same_bits(o.harmonic_ratio(x), value)
    if HOSTSTUB:
        return
    frames = hr.harmonic_ratio(x, p["window"], c[2], c[3], mx)
    w = check_case(name, frames, gold[name + "/eps"], value, mx, dlag, dfirst, curve, hc.cap(name))
    print(f"{name}: curve {w['worst_curve']:.4f}, value {w['worst_value']:.4f} of their bars, explained {w['explained']} of "
          f"{w['frames']}, first {dfirst.tolist()}, value {value.tolist()}")
    parity_log(f"harmonic_ratio/{name}", max(w["worst_curve"], w["worst_value"]) * 1e-5, 1e-5,
               "harmonic_ratio: worst curve / value error over its bar, scaled to 1e-5", {"explained": w["explained"], "frames": w["frames"]})
    _consistent(name, value, dlag, dfirst, curve, mx)
    if c[4] == "zero":
        assert not value.any() and not curve.any()


def test_batch_equals_single_calls_and_no_min_index_crosses_a_clip(lib):
    """3 different clips, dc behind noise, clipStride > dataLength, outStride > frames, a 4-byte-misaligned base, outputs
    pre-filled: bitwise the single calls, guards untouched, dFirst of the dc clip 0 throughout"""
    import torch
    names = ("carry_r8", "noise_r8", "dc_r8")
    n = 256 + 64 * 5 + 5
    xs = [hc.case_input(k)[:n] for k in names]
    clips, stride = 3, n + 12
    buf = np.zeros(clips * stride + 1, np.float32)
    rows = buf[1:].reshape(clips, stride)
    for c in range(clips):
        rows[c, :n] = xs[c]
    o = af.HarmonicRatio(samplate=16000, low_fre=1000.0, radix2_exp=8, slide_length=64)
    T = o.cal_time_length(n)
    single = [o.harmonic_ratio(x) for x in xs]
    d = torch.from_numpy(buf).cuda()
    assert (d.data_ptr() + 4) % 16 == 4
    pitch, guard = T + 3, 64
    v = torch.full((1 + clips * pitch + guard,), float("nan"), device="cuda")
    lag = torch.full((1 + clips * pitch + guard,), 77, dtype=torch.int32, device="cuda")
    first = torch.full_like(lag, 77)
    s = torch.cuda.current_stream().cuda_stream
    st = lib.harmonicRatioObj_harmonicRatioBatchDevice(o._obj, d.data_ptr() + 4, clips, n, stride, v.data_ptr() + 4, lag.data_ptr() + 4,
                                                       first.data_ptr() + 4, pitch, s)
    assert st == 0, af.last_error()
    torch.cuda.synchronize()
    vh, lh, fh = v.cpu().numpy(), lag.cpu().numpy(), first.cpu().numpy()
    assert np.isnan(vh[0]) and lh[0] == 77 and fh[0] == 77, "wrote in front of the output"
    vh, lh, fh = vh[1:], lh[1:], fh[1:]
    rv, rl, rf = (a[:clips * pitch].reshape(clips, pitch) for a in (vh, lh, fh))
    for c in range(clips):
        assert same_bits(rv[c, :T], single[c]), c
    assert not np.isnan(rv[:, :T]).any() and (rl[:, :T] != 77).all() and (rf[:, :T] != 77).all(), "a frame entry was not written"
    assert np.isnan(rv[:, T:]).all() and (rl[:, T:] == 77).all() and (rf[:, T:] == 77).all(), "wrote beyond a row's frames"
    assert np.isnan(vh[clips * pitch:]).all() and (lh[clips * pitch:] == 77).all() and (fh[clips * pitch:] == 77).all(), "wrote into the guard"
    if not HOSTSTUB:
        assert rf[0, :T].tolist() == [1, 1, 2, 2, 2, 2] and rf[1, :T].all() and not rf[2, :T].any(), rf[:, :T]
    # the curve rows of the batch, with a guard behind them
    cv = torch.full((clips * T * o.max_length + guard,), float("nan"), device="cuda")
    assert lib.harmonicRatioObj_curveBatchDevice(o._obj, d.data_ptr() + 4, clips, n, stride, cv.data_ptr(), s) == 0
    torch.cuda.synchronize()
    ch = cv.cpu().numpy()
    assert not np.isnan(ch[:-guard]).any() and np.isnan(ch[-guard:]).all()
    one = o.curve_batch_device(torch.from_numpy(xs[2]).cuda()[None])[0].cpu().numpy()
    assert same_bits(ch[:-guard].reshape(clips, T, -1)[2], one)


def test_a_split_call_restarts_from_zero_as_the_reference_does(lib, gold):
    """carry_r8 in one call and split at a frame boundary: frames 5 ... 9 inherit 2 in one call and 0 after the split"""
    name = "carry_r8"
    c = hc.CASES[name]
    x = hc.case_input(name)
    cut = c[3] * 5
    st, obj = hc.new(lib, *hc.ctor_args(name))
    assert st == 0
    whole = hc.call(lib, obj, x)
    a, b = hc.call(lib, obj, x[:256 + c[3] * 4]), hc.call(lib, obj, x[cut:])
    lib.harmonicRatioObj_free(obj)
    assert len(a) == len(b) == 5 and same_bits(a, whole[:5])
    if HOSTSTUB:
        return
    assert not same_bits(b, whole[5:])
    st, p = hc.plan(lib, *hc.ctor_args(name))
    mx = p["maxLength"]
    tail = hr.harmonic_ratio(x[cut:], p["window"], c[2], c[3], mx)
    assert [f["first"] for f in tail] == [0] * 5
    eps = np.full(5, 1e-5)
    if ref.available():  # the yardstick of the rule, and the reference's own split
        rlib = hc.bind(ref.lib())
        rst, robj = hc.new(rlib, *hc.ctor_args(name))
        assert rst == 0
        rwhole, rb = hc.call(rlib, robj, x), hc.call(rlib, robj, x[cut:])
        rlib.harmonicRatioObj_free(robj)
        assert same_bits(rwhole, gold[name + "/value"]) and not same_bits(rb, rwhole[5:])
        eps = [reference_eps(f, rb[t]) for t, f in enumerate(tail)]
    check_case("split tail", tail, eps, b, mx)


def test_refusals_on_the_device_path(lib):
    import torch
    n = 512 + 128 * 3
    x = torch.from_numpy(hc.signal("tone:330", n, 16000, seed=3)).cuda()
    out = torch.full((16,), 5.0, device="cuda")
    fn, cv = lib.harmonicRatioObj_harmonicRatioBatchDevice, lib.harmonicRatioObj_curveBatchDevice
    s = torch.cuda.current_stream().cuda_stream
    for bad in (5, 13):
        st, o = hc.new(lib, r=bad)
        assert st == -100 and not o
    st, o = hc.new(lib, 16000, 40.0, 9, None, 128)
    assert st == 0
    assert fn(None, x.data_ptr(), 1, n, n, out.data_ptr(), None, None, 16, s) == -6
    assert fn(o, None, 1, n, n, out.data_ptr(), None, None, 16, s) == -6
    assert fn(o, x.data_ptr(), 1, n, n, None, None, None, 16, s) == -6
    assert fn(o, x.data_ptr(), 0, n, n, out.data_ptr(), None, None, 16, s) == -6
    assert fn(o, x.data_ptr(), 1, 0, n, out.data_ptr(), None, None, 16, s) == -6
    assert fn(o, x.data_ptr(), 1, n, n - 1, out.data_ptr(), None, None, 16, s) == -6  # clipStride below dataLength
    assert fn(o, x.data_ptr(), 1, n, n, out.data_ptr(), None, None, 3, s) == -6      # outStride below the 4 frames
    assert cv(o, x.data_ptr(), 1, n, n, None, s) == -6
    assert fn(o, x.data_ptr(), 1, 511, n, out.data_ptr(), None, None, 16, s) == 0    # no frame: nothing to do
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5).all(), "a refused / empty call wrote"
    # the optional outputs NULL: the values alone, the same bits
    assert fn(o, x.data_ptr(), 1, n, n, out.data_ptr(), None, None, 16, s) == 0
    full = torch.empty(4, device="cuda")
    ints = torch.empty((2, 4), dtype=torch.int32, device="cuda")
    assert fn(o, x.data_ptr(), 1, n, n, full.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), 4, s) == 0
    torch.cuda.synchronize()
    lib.harmonicRatioObj_free(o)
    oh = out.cpu().numpy()
    assert same_bits(oh[:4], full.cpu().numpy()) and (oh[4:] == 5).all()


def test_interleaved_with_a_pitch_ncf_object_on_one_stream():
    """a HarmonicRatio and a PitchNCF object of different N share no state: calls queued alternately on one stream equal the
    calls made alone"""
    import torch
    from tests import pitch_lag_cases as pc
    a = _obj("carry_r8")
    b = af.PitchNCF(samplate=44100, low_fre=50.0, high_fre=1500.0, radix2_exp=11, slide_length=512)
    xa = torch.from_numpy(hc.case_input("carry_r8")).cuda()[None]
    xb = torch.from_numpy(pc.case_input("r11_sr44k")).cuda()[None]
    alone_a, alone_b = a.harmonic_ratio_batch_device(xa), b.pitch_batch_device(xb)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = [(a.harmonic_ratio_batch_device(xa, s), b.pitch_batch_device(xb, s)) for _ in range(3)]
    s.synchronize()
    for ra, rb in outs:
        for got, want in zip(ra + rb, alone_a + alone_b):
            assert same_bits(got.cpu().numpy().view(np.float32), want.cpu().numpy().view(np.float32))
