"""GPU: the NSGT object on the device -- every row of tests/nsgt_cases.py, three inputs, through NSGT.nsgt_device with the
cells, judged per band at the bar of tests/nsgt_cases.py against float64 and the stored compiled-reference results; batches,
the host entry, nsgtObj_setMinLength against fresh objects, refusals."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import nsgt_cases as nc

pytestmark = pytest.mark.gpu
GUARD = 64


def make(c, min_len=None):
    return af.NSGT(num=c.num, radix2_exp=c.r, samplate=c.sr, low_fre=c.low, high_fre=c.high, bin_per_octave=c.bpo,
                   min_len=c.min_len if min_len is None else min_len, nsgt_filter_bank_type=af.NSGTFilterBankType(c.bank),
                   scale_type=af.SpectralFilterBankScaleType(nc.SCALE[c.scale]),
                   style_type=af.SpectralFilterBankStyleType(nc.STYLE[c.style]),
                   normal_type=af.SpectralFilterBankNormalType(nc.NORMAL[c.normal]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def shifted(x):
    """chunk 0 starts 4 bytes behind a 16-byte boundary, odd chunk stride (the `shift` layout of tests/cwt_check.py)"""
    import torch
    chunks, n = x.shape
    stride = n + 3
    base = torch.zeros(chunks * stride + 8, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    xd = torch.as_strided(base, (chunks, n), (stride, 1), 1)
    xd.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert xd.data_ptr() % 16 == 4 and xd.stride(0) % 2 == 1
    return xd


def run_device(o, xd, cells=True):
    """NaN-filled outputs with GUARD floats behind each -> numpy (re, im, cell_re, cell_im); the guards are checked"""
    import torch
    c = xd.shape[0]
    mx, tot = o.get_max_time_length(), o.get_total_time_length()
    flat = [torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
            for n in (c * o.num * mx, c * o.num * mx, c * tot, c * tot)]
    for f in flat:
        f[-GUARD:] = 7.5
    re, im = (f[:-GUARD].view(c, o.num, mx) for f in flat[:2])
    fn = o._lib.nsgtObj_nsgtBatchDevice
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 5
    if cells:  # the wrapper allocates the cell planes itself: guarded planes go through the C entry
        st = fn(o._obj, xd.data_ptr(), c, xd.stride(0), flat[0].data_ptr(), flat[1].data_ptr(), flat[2].data_ptr(),
                flat[3].data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, af.last_error()
    else:
        o.nsgt_device(xd, out_real=re, out_imag=im)
    torch.cuda.synchronize()
    host = [f.cpu().numpy() for f in flat]
    for h in host:
        assert (h[-GUARD:] == 7.5).all(), "wrote behind an output"
    return (host[0][:-GUARD].reshape(c, o.num, mx), host[1][:-GUARD].reshape(c, o.num, mx),
            host[2][:-GUARD].reshape(c, tot), host[3][:-GUARD].reshape(c, tot))


@pytest.fixture(scope="module")
def results():
    """per case: the object and its device results of the three inputs (computed once, shared, read-only)"""
    cache = {}

    def get(name):
        if name not in cache:
            o = make(nc.by_name(name))
            out = run_device(o, shifted(nc.inputs(name)))
            for a in out:
                a.setflags(write=False)
            cache[name] = (o, out)
        return cache[name]
    return get


@pytest.mark.parametrize("name", [c.name for c in nc.CASES])
def test_device_results_meet_both_references(name, results):
    """three chunks, shifted layout, NaN-filled outputs with guards: every band of every chunk, cells and matrix rows"""
    o, (re, im, cre, cim) = results(name)
    p = nc.product_plan(name)
    assert o.get_max_time_length() == p.max and o.get_total_time_length() == p.total
    assert np.array_equal(o.get_time_length_arr(), p.len) and same_bits(o.get_fre_band_arr(), p.fre)
    assert np.array_equal(o.get_bin_band_arr(), p.bin)
    worst = nc.judge(name, range(3), cre + 1j * cim, re + 1j * im, tag=" device")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["mel12", "log20std", "bark2", "oct24min"])
def test_batch_equals_single_chunks_and_the_host_entry_bitwise(name, results):
    import torch
    o, (re, im, cre, cim) = results(name)
    x = nc.inputs(name)
    for q in range(3):
        a = run_device(o, torch.from_numpy(x[q:q + 1].copy()).cuda())
        assert same_bits(a[0][0], re[q]) and same_bits(a[1][0], im[q]), (name, q, "single chunk")
        assert same_bits(a[2][0], cre[q]) and same_bits(a[3][0], cim[q]), (name, q, "single chunk cells")
        m = o.nsgt(x[q])  # host pointers
        assert m.dtype == np.complex64 and same_bits(m.real, re[q]) and same_bits(m.imag, im[q]), (name, q, "host entry")
        cells = np.concatenate(o.get_cell_data())
        assert [len(b) for b in o.get_cell_data()] == list(o.get_time_length_arr())
        assert same_bits(cells.real, cre[q]) and same_bits(cells.imag, cim[q]), (name, q, "get_cell_data")
    # without the cells: the same matrix, nothing else written
    b = run_device(o, shifted(x), cells=False)
    assert same_bits(b[0], re) and same_bits(b[1], im) and np.isnan(b[2]).all() and np.isnan(b[3]).all()
    # the wrapper's own allocation
    r2, i2, c2, d2 = o.nsgt_device(shifted(x), cells=True)
    torch.cuda.synchronize()
    assert same_bits(r2.cpu().numpy(), re) and same_bits(c2.cpu().numpy(), cre) and same_bits(d2.cpu().numpy(), cim)


def test_set_min_length_rebuilds_the_whole_plan():
    """mel12, 3 -> 40 -> 1: getters, cells and matrix equal those of a fresh object; a plan with a band longer than the chunk
    is refused and leaves the object as it was"""
    c = nc.by_name("mel12")
    xd = shifted(nc.inputs("mel12"))
    o = make(c)
    for m in (40, 1):
        o.set_min_length(m)
        fresh = make(c, m)
        assert o.get_max_time_length() == fresh.get_max_time_length()
        assert o.get_total_time_length() == fresh.get_total_time_length()
        for g in ("get_time_length_arr", "get_fre_band_arr", "get_bin_band_arr"):
            assert same_bits(getattr(o, g)(), getattr(fresh, g)()), (m, g)
        a, b = run_device(o, xd), run_device(fresh, xd)
        assert all(same_bits(u, v) for u, v in zip(a, b)), m
    with pytest.raises(RuntimeError, match="band"):
        o.set_min_length(1000)
    assert all(same_bits(u, v) for u, v in zip(run_device(o, xd), a))
    assert o.get_time_length_arr().max() == fresh.get_time_length_arr().max()


def test_batch_device_refuses_bad_arguments(results):
    import torch
    o, _ = results("mel12")
    n = 512
    x = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * o.num * o.get_max_time_length(), dtype=torch.float32, device="cuda")
    fn = o._lib.nsgtObj_nsgtBatchDevice
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 5
    s = torch.cuda.current_stream().cuda_stream
    xp, op = x.data_ptr(), out.data_ptr()
    assert fn(o._obj, xp, 1, n, None, op, None, None, s) == -6
    assert fn(o._obj, xp, 1, n, op, None, None, None, s) == -6
    assert fn(o._obj, None, 1, n, op, op, None, None, s) == -6
    assert fn(o._obj, xp, 0, n, op, op, None, None, s) == -6
    assert fn(o._obj, xp, 1, n - 1, op, op, None, None, s) == -6
    assert fn(o._obj, xp, 1, n, op, op, op, None, s) == -6
    assert fn(None, xp, 1, n, op, op, None, None, s) == -6
    torch.cuda.synchronize()
    assert not out.any()


def test_multi_channel_input_keeps_its_leading_axes(results):
    o, (re, im, _, _) = results("mel12")
    x = nc.inputs("mel12")
    xs = np.stack([x, x[::-1]])  # (2, 3, N)
    m = o.nsgt(xs)
    assert m.shape == (2, 3, o.num, o.get_max_time_length()) and m.dtype == np.complex64
    assert same_bits(m[0].real, re) and same_bits(m[1, 0].imag, im[2])
    assert o.nsgt(x[0][:300]).shape == (o.num, o.get_max_time_length())  # zero-padded like the reference wrapper
    assert len(o.y_coords()) == o.num + 1 and len(o.x_coords(512)) == o.get_max_time_length() + 1
