"""GPU parity of harmonic / percussive separation (af.HPSS, mir/hpss_algorithm.h): the fixture of the compiled reference's
outputs, fresh inputs against the compiled reference when oracle/_ref is present, the median primitive bitwise against the
sort-based numpy statement, batch == per-clip calls and chunked == unchunked bitwise, the magnitude planes, stream ordering,
and properties at the headline size (1000 clips of 30 s) where no reference can run."""
import ctypes as C
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import hpss_cases as hc
from tests import hpss_restate as hr
from tests.conftest import HOSTSTUB
from tests.golden.make_hpss_golden import bind, run
from tests.hpss_check import check_waveform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "hpss.npz"))


@pytest.fixture(scope="module")
def lib():
    lib = af.get_lib()
    bind(lib)
    return lib


def same_bits(a, b):
    return HOSTSTUB or np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("name", list(hc.CASES))
def test_fixture_case(name, gold, lib):
    r, w, h, p, kind, n, outs, init = hc.CASES[name]
    x = hc.case_input(name)
    ha, pa = run(lib, x, r, w, h, p, outs, hc.initial(name, "h"), hc.initial(name, "p"))
    for key, got in (("h", ha), ("p", pa)):
        if key in outs:
            check_waveform(f"{name}/{key}", got, gold[f"{name}/{key}"], np.abs(x).max(), r, w)
        else:
            assert got is None


@pytest.mark.parametrize("r,h,p,w", [(9, 21, 31, hc.HAMM), (11, 21, 31, hc.HAMM), (11, 7, 45, hc.HANN), (12, 63, 3, hc.HAMM),
                                     (13, 21, 31, hc.HAMM), (6, 5, 9, hc.RECT)])
def test_fresh_input_against_the_compiled_reference(r, h, p, w, lib):
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    rlib = ref.lib()
    bind(rlib)
    n = (1 << r) + ((1 << r) // 4) * 37 + 11
    x = hc.signal("mix", n, seed=300 + r)
    got = run(lib, x, r, w, h, p)
    want = run(rlib, x, r, w, h, p)
    for key, g, v in zip("hp", got, want):
        check_waveform(f"fresh r{r} {h}/{p} {key}", g, v, np.abs(x).max(), r, w)


def test_wrapper_all_channels_in_one_call_and_order_one():
    x = np.stack([hc.signal("mix", 2048 + 512 * 30, seed=s) for s in range(4)]).reshape(2, 2, -1)
    o = af.HPSS(radix2_exp=11, slide_length=7)  # slide_length is ignored
    h, p = o.hpss(x)
    assert h.shape == p.shape == (2, 2, o.cal_data_length(x.shape[-1]))
    h0, p0 = o.hpss(x[1, 0])
    assert same_bits(h[1, 0], h0) and same_bits(p[1, 0], p0)
    wh, wp = hr.hpss(x[1, 0], 11, hc.HAMM, 21, 31)
    check_waveform("wrapper h", h0, wh, np.abs(x[1, 0]).max(), 11, hc.HAMM)
    check_waveform("wrapper p", p0, wp, np.abs(x[1, 0]).max(), 11, hc.HAMM)
    # order 1: the identity (documented deviation; the reference masks with stale memory)
    o1 = af.HPSS(radix2_exp=10, h_order=1, p_order=31)
    y = hc.signal("mix", 1024 + 256 * 20, seed=9)
    h1, p1 = o1.hpss(y)
    wh, wp = hr.hpss(y, 10, hc.HAMM, 1, 31)
    check_waveform("order 1 h", h1, wh, np.abs(y).max(), 10, hc.HAMM)
    check_waveform("order 1 p", p1, wp, np.abs(y).max(), 10, hc.HAMM)
    # below one frame: nothing is written
    hs, ps = o1.hpss(y[:1000])
    assert hs.shape == (768,) and not hs.any() and not ps.any()


@pytest.mark.parametrize("shape,orders", [((70, 131), list(range(1, 64, 2)) + [65, 255]), ((63, 127), [3, 21, 31, 63]),
                                          ((65, 129), [3, 21, 31, 63]), ((2, 300), [5, 31, 101]), ((934, 1025), [21, 31, 63])])
def test_median_filter_is_bitwise_the_sorted_window(shape, orders):
    import torch
    rng = np.random.default_rng(shape[0])
    a = rng.standard_normal(shape).astype(np.float32)
    a[rng.random(shape) < 0.1] = 0.25  # ties
    d = torch.from_numpy(a).cuda()
    for order in orders:
        for axis in (0, 1):
            got = af.median_filter_device(d, order, axis).cpu().numpy()
            assert same_bits(got, hr.median_filter(a, axis, order)), (shape, order, axis)


def test_median_filter_clips_and_headline_plane():
    import torch
    rng = np.random.default_rng(1)
    a = rng.standard_normal((3 * 23 + 7, 40)).astype(np.float32)
    d = torch.from_numpy(a).cuda()
    for order in (5, 21, 65):
        assert same_bits(af.median_filter_device(d, order, 0, frames_per_clip=23).cpu().numpy(), hr.median_filter(a, 0, order, 23))
    # the plane of the headline batch: 100 clips x 934 frames x 1025 bins on the device against itself clip by clip, and a
    # sample of its cells against the sort
    g = torch.Generator(device="cuda").manual_seed(7)
    big = torch.rand((100 * 934, 1025), device="cuda", generator=g)
    for axis, order in ((0, 21), (1, 31)):
        out = af.median_filter_device(big, order, axis, frames_per_clip=934)
        one = af.median_filter_device(big[934 * 57:934 * 58].contiguous(), order, axis)
        assert HOSTSTUB or torch.equal(out[934 * 57:934 * 58], one)
        rows = slice(934 * 99 + 900, 934 * 100)  # the end of the last clip
        want = hr.median_filter(big[934 * 99:].cpu().numpy(), axis, order)[900:]
        assert same_bits(out[rows].cpu().numpy(), want)


def _device_call(o, x, chunk_mb=None):
    import torch
    if chunk_mb:
        os.environ["AFX_HPSS_CHUNK_MB"] = str(chunk_mb)
    try:
        h, p = o.hpss_device(x)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("AFX_HPSS_CHUNK_MB", None)
    return h, p


def test_batch_equals_single_clips_and_chunked_equals_unchunked_bitwise():
    import torch
    n = 2048 + 512 * 60 + 100
    x = torch.from_numpy(np.stack([hc.signal("mix", n, seed=20 + c) for c in range(7)])).cuda()
    o = af.HPSS(radix2_exp=11)
    h, p = _device_call(o, x)
    for c in (0, 3, 6):
        h1, p1 = _device_call(o, x[c:c + 1])
        assert HOSTSTUB or (torch.equal(h[c], h1[0]) and torch.equal(p[c], p1[0])), c
    hc_, pc_ = _device_call(o, x, chunk_mb=5)  # a clip's scratch is 2.5 MB: chunks of two clips
    assert HOSTSTUB or (torch.equal(h, hc_) and torch.equal(p, pc_))
    # one output alone equals that output of the pair
    h_only, none = o.hpss_device(x, percussive=False)
    assert none is None and (HOSTSTUB or torch.equal(h_only, h))
    # read-modify-write like stftObj_istft: what the buffer held goes through the same division by the window sum,
    # (held + sum of frames) / sum w^2 -- a second call onto the result gives h / sum w^2 + h
    fn = o._lib.hpssObj_hpssBatchDevice
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    st = fn(o._obj, x.data_ptr(), 7, n, x.stride(0), h.data_ptr(), None, h.shape[1], torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    w = hr.window(hc.HAMM, 2048)
    nrm = np.zeros(h.shape[1])
    for i in range(61):
        nrm[i * 512:i * 512 + 2048] += w * w
    want = h_only.cpu().numpy().astype(np.float64) * (1.0 + 1.0 / nrm)
    assert HOSTSTUB or np.abs(h.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


def test_magnitude_planes_are_consistent_with_the_waveforms():
    import torch
    n = 1024 + 256 * 50
    xs = np.stack([hc.signal("mix", n, seed=40 + c) for c in range(3)])
    x = torch.from_numpy(xs).cuda()
    o = af.HPSS(radix2_exp=10)
    hm, pm = o.spectra_device(x)
    h, p = o.hpss_device(x)
    torch.cuda.synchronize()
    for c in range(3):
        s, mag, wh, wp = hr.spectra(xs[c], 10, hc.HAMM, 21, 31)
        assert np.abs(hm[c].cpu().numpy() - wh).max() <= 1e-5 * mag.max() and np.abs(pm[c].cpu().numpy() - wp).max() <= 1e-5 * mag.max()
    # the harmonic waveform is the inverse of (harmonic magnitude x the unit phase of the clip's own STFT)
    st = af.STFT(radix2_exp=10, window_type=af.WindowType.HAMM, slide_length=256)
    re, im = st.stft_device(x)
    mag = torch.sqrt(re * re + im * im).clamp_min(1e-16)
    full = torch.cat([hm, hm[..., 1:-1].flip(-1)], dim=-1) / mag
    back = st.istft_device((re * full).contiguous(), (im * full).contiguous())
    torch.cuda.synchronize()
    assert HOSTSTUB or float((back - h).abs().max()) <= 1e-5 * float(x.abs().max())


def test_stream_ordering():
    """the call is asynchronous on the caller's stream: work enqueued behind a long kernel on a side stream sees that kernel's
    result, and a consumer on the same stream sees the separation's"""
    import torch
    n = 2048 + 512 * 100
    o = af.HPSS(radix2_exp=11)
    base = torch.from_numpy(np.stack([hc.signal("mix", n, seed=60 + c) for c in range(4)])).cuda()
    want_h, want_p = _device_call(o, base)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = torch.zeros_like(base)
        for _ in range(20):  # a queue of work in front of the producer
            x = x * 1.0
        x = x + base
        h, p = o.hpss_device(x, stream=side)
        total = (h + p).sum()
    side.synchronize()
    assert HOSTSTUB or (torch.equal(h, want_h) and torch.equal(p, want_p))
    assert HOSTSTUB or float(total) == float((want_h + want_p).sum())


def test_properties_at_the_headline_size():
    """1000 clips x 30 s @ 16 kHz, n_fft 2048 (934 000 frames, several chunks): h + p is the round trip of the clip through our own
    STFT objects to 1e-5; a stationary chord goes to h, a click train to p (>= 99 % of the energy)"""
    import torch
    clips, n = 1000, 480000
    o = af.HPSS(radix2_exp=11)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / 16000.0
    chord = sum(a * torch.sin(2 * np.pi * f * t + ph) for f, a, ph in ((220.0, 0.3, 0.1), (277.18, 0.25, 1.0), (329.63, 0.2, 2.0)))
    clicks = torch.zeros(n, device="cuda")
    clicks[997::8009] = 0.8   # a click every 15.6 frames: fewer than half of any 21 frames hold one
    clicks[998::8009] = -0.5
    g = torch.Generator(device="cuda").manual_seed(11)
    x = 0.01 * torch.randn((clips, n), device="cuda", generator=g)
    x[0::2] += chord
    x[1::2] += clicks
    x[0] = chord
    x[1] = clicks
    h, p = o.hpss_device(x)
    torch.cuda.synchronize()
    if HOSTSTUB:
        return
    m = h.shape[1]
    assert m == o.cal_data_length(n) == 2048 + 512 * 933
    # round trip of a sample of clips (first, last, chunk interiors) through the STFT object
    st = af.STFT(radix2_exp=11, window_type=af.WindowType.HAMM, slide_length=512)
    pick = [0, 1, 2, 499, 500, 998, 999]
    re, im = st.stft_device(x[pick].contiguous())
    back = st.istft_device(re, im)
    torch.cuda.synchronize()
    err = float((h[pick] + p[pick] - back).abs().max()) / float(x[pick].abs().max())
    assert err <= 1e-5, err
    inner = slice(8192, m - 8192)  # (the first and last hOrder/2 frames see the zeros outside the clip)
    eh, ep = float((h[0, inner] ** 2).sum()), float((p[0, inner] ** 2).sum())
    assert eh >= 0.99 * (eh + ep), (eh, ep)
    eh, ep = float((h[1, inner] ** 2).sum()), float((p[1, inner] ** 2).sum())
    assert ep >= 0.99 * (eh + ep), (eh, ep)
    # every clip of a kind got the same treatment whatever chunk it was in: clips 0 and 1 again as a batch of their own
    h2, p2 = o.hpss_device(x[:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(h2, h[:2]) and torch.equal(p2, p[:2])
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(p).all())
