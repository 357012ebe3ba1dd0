"""GPU: the FST object on the device -- every row of tests/fst_cases.py through fstObj_fstBatchDevice with the shifted input
layout, NaN-filled guarded outputs, judged at the bar of tests/fst_cases.py against float64 and the stored compiled-reference
cells; the matrix against the expansion of the returned cells, batches against single chunks, the host entry and the wrapper,
the forms of the call, refusals."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from audioflux_amd import _lib
from tests import fst_cases as fc

pytestmark = pytest.mark.gpu
GUARD = 64
ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 5


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cplx(re, im):
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def shifted(x):
    """chunk 0 starts 4 bytes behind a 16-byte boundary, odd chunk stride (the `shift` layout of tests/test_nsgt_gpu.py)"""
    import torch
    chunks, n = x.shape
    stride = n + 3
    base = torch.zeros(chunks * stride + 8, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    xd = torch.as_strided(base, (chunks, n), (stride, 1), 1)
    xd.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert xd.data_ptr() % 16 == 4 and xd.stride(0) % 2 == 1
    return xd


def batch_fn(o):
    fn = o._lib.fstObj_fstBatchDevice
    fn.restype, fn.argtypes = C.c_int, ARGTYPES
    return fn


def run_device(o, xd, lo, hi, matrix=True, cells=True, shift=0):
    """NaN-filled outputs (the planes `shift` floats behind a 16-byte boundary) with GUARD floats behind each -> complex64
    rows [chunks][hi - lo + 1][N] and cells [chunks][N/2 + 1]; the guards are checked, and that nothing unasked is written"""
    import torch
    c, n = xd.shape
    rows, cl = hi - lo + 1, n // 2 + 1
    flat = []
    for size, sh in ((c * rows * n, shift), (c * rows * n, shift), (c * cl, 0), (c * cl, 0)):
        f = torch.full((size + GUARD + 4,), float("nan"), dtype=torch.float32, device="cuda")[sh:sh + size + GUARD]
        f[-GUARD:] = 7.5
        assert f.data_ptr() % 16 == 4 * sh
        flat.append(f)
    ptr = [f.data_ptr() for f in flat]
    st = batch_fn(o)(o._obj, xd.data_ptr(), c, xd.stride(0), lo, hi, ptr[0] if matrix else None, ptr[1] if matrix else None,
                     ptr[2] if cells else None, ptr[3] if cells else None, torch.cuda.current_stream().cuda_stream)
    assert st == 0, af.last_error()
    torch.cuda.synchronize()
    host = [f.cpu().numpy() for f in flat]
    for h in host:
        assert (h[-GUARD:] == 7.5).all(), "wrote behind an output"
    re, im = (h[:-GUARD].reshape(c, rows, n) for h in host[:2])
    cre, cim = (h[:-GUARD].reshape(c, cl) for h in host[2:])
    for want, a, b, what in ((matrix, re, im, "matrix"), (cells, cre, cim, "cells")):
        if want:
            assert np.isfinite(a).all() and np.isfinite(b).all(), f"a {what} element nobody wrote"
        else:
            assert np.isnan(a).all() and np.isnan(b).all(), f"{what} written although not asked for"
    return cplx(re, im), cplx(cre, cim)


def host_entry(o, x, lo, hi):
    """fstObj_fst through the checked proxy -> complex64 [hi - lo + 1][N] (NaN where nothing was written)"""
    n = len(x)
    re, im = (np.full((max(hi - lo + 1, 1), n), np.nan, np.float32) for _ in range(2))
    fn = _lib.checked(o._lib.fstObj_fst)
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    x = np.ascontiguousarray(x, np.float32)
    try:
        fn(o._obj, x.ctypes.data, lo, hi, re.ctypes.data, im.ctypes.data)
    finally:
        host_entry.last = cplx(re, im)
    return host_entry.last


@pytest.fixture(scope="module")
def results():
    """per case: an object of the case's size and per range the device results of the case's chunks (computed once, shared,
    read-only)"""
    cache = {}

    def get(name):
        if name not in cache:
            c = fc.by_name(name)
            o = af.FST(radix2_exp=c.r)
            xd = shifted(fc.inputs(name)[list(c.chunks)])
            out = {}
            for lo, hi in c.ranges:
                rows, cells = run_device(o, xd, lo, hi)
                rows.setflags(write=False)
                cells.setflags(write=False)
                out[(lo, hi)] = (rows, cells)
            cache[name] = (o, xd, out)
        return cache[name]
    return get


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_device_results_meet_both_references(name, results):
    """shifted layout, NaN-filled outputs with guards: cells and every requested row at the bar; every row is bitwise the
    sample-and-hold of its band (so the rows of one band are bitwise equal) and the matrix the expansion of the returned cells"""
    c = fc.by_name(name)
    o, _, out = results(name)
    assert o.get_cell_length() == (1 << c.r) // 2 + 1
    worst = 0.0
    for (lo, hi), (rows, cells) in out.items():
        worst = max(worst, fc.judge_cells(name, c.chunks, cells, tag=f" device {lo}...{hi}"),
                    fc.judge_rows(name, c.chunks, rows, lo, hi, tag=" device"))
        for q in range(len(c.chunks)):
            assert same_bits(rows[q], fc.expand(cells[q], c.r, lo, hi)), (name, q, "matrix != expansion of the cells")
        if c.matrix:
            ref = fc.reference(name)
            for q, k in enumerate(c.chunks):
                e = np.abs(rows[q].astype(np.complex128) - ref.mat_c[k]).max() / ref.peak[k]
                assert e <= max(fc.FLOOR, fc.FACTOR * ref.r_ref[k]), (name, fc.INPUTS[k], "stored matrix", e)
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["r4full", "r9default", "r12doc", "r14edge"])
def test_batch_equals_single_chunks_the_host_entry_and_the_forms_bitwise(name, results):
    import torch
    c = fc.by_name(name)
    o, xd, out = results(name)
    x = fc.inputs(name)[list(c.chunks)]
    for (lo, hi), (rows, cells) in out.items():
        for q in range(len(x)):
            if len(x) > 1:
                r1, c1 = run_device(o, torch.from_numpy(x[q:q + 1].copy()).cuda(), lo, hi)
                assert same_bits(r1[0], rows[q]) and same_bits(c1[0], cells[q]), (name, q, "single chunk")
            assert same_bits(host_entry(o, x[q], lo, hi), rows[q]), (name, q, "host entry")  # r12doc: two passes of row blocks
        r2, _ = run_device(o, xd, lo, hi, cells=False)
        _, c2 = run_device(o, xd, lo, hi, matrix=False)
        assert same_bits(r2, rows) and same_bits(c2, cells), (name, "matrix-only / cells-only form")
        if name != "r12doc":
            r3, _ = run_device(o, xd, lo, hi, cells=False, shift=1)  # planes off the 16-byte grid: dword stores
            assert same_bits(r3, rows), (name, "unaligned planes")


@pytest.mark.parametrize("name", ["r9default", "r12doc"])
def test_wrapper_equals_the_device_results_bitwise(name, results):
    import torch
    c = fc.by_name(name)
    (lo, hi), = c.ranges
    _, xd, out = results(name)
    rows, cells = out[(lo, hi)]
    x = fc.inputs(name)[list(c.chunks)]
    w = af.FST(radix2_exp=c.r, min_index=lo, max_index=None if name == "r9default" else hi)
    assert (w.min_index, w.max_index, w.num, w.fft_length) == (lo, hi, hi - lo + 1, 1 << c.r)
    m = w.fst(x[0])
    assert m.dtype == np.complex64 and m.shape == (w.num, w.fft_length) and same_bits(m, rows[0])
    re, im, cre, cim = w.fst_device(xd, cells=True)  # the wrapper's own allocation
    torch.cuda.synchronize()
    assert same_bits(re.cpu().numpy(), rows.real) and same_bits(im.cpu().numpy(), rows.imag)
    assert same_bits(cre.cpu().numpy(), cells.real) and same_bits(cim.cpu().numpy(), cells.imag)
    re2, im2 = w.fst_device(xd, out_real=torch.empty_like(re), out_imag=torch.empty_like(im))
    torch.cuda.synchronize()
    assert same_bits(re2.cpu().numpy(), rows.real) and same_bits(im2.cpu().numpy(), rows.imag)


def test_docstring_call_returns_the_documented_shape():
    x = fc.inputs("r12doc")[1]
    m = af.FST(radix2_exp=12, min_index=1, max_index=1024).fst(x)
    assert m.dtype == np.complex64 and m.shape == (1024, 4096) and np.isfinite(m.view(np.float32)).all()


def test_element_indices_past_2_31_per_plane():
    """2^14 samples, all 8193 rows, 17 chunks: 2.28e9 elements a plane.  Chunks 0, 15 (ends past 2^31) and 16 equal their
    single-chunk calls bit for bit, compared on the device"""
    import torch
    r, n, chunks = 14, 1 << 14, 17
    rows = n // 2 + 1
    per = rows * n
    assert (chunks - 2) * per < 2 ** 31 < (chunks - 1) * per
    o = af.FST(radix2_exp=r)
    x = fc.inputs("r14edge")
    xd = torch.from_numpy(np.ascontiguousarray(x[[q % 3 for q in range(chunks)]])).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fn = batch_fn(o)
    re, im = (torch.empty(chunks * per, dtype=torch.float32, device="cuda") for _ in range(2))
    assert fn(o._obj, xd.data_ptr(), chunks, n, 0, n // 2, re.data_ptr(), im.data_ptr(), None, None, s) == 0, af.last_error()
    r1, i1 = (torch.empty(per, dtype=torch.float32, device="cuda") for _ in range(2))
    for q in (0, chunks - 2, chunks - 1):
        r1.fill_(float("nan"))
        i1.fill_(float("nan"))
        assert fn(o._obj, xd[q].data_ptr(), 1, n, 0, n // 2, r1.data_ptr(), i1.data_ptr(), None, None, s) == 0, af.last_error()
        assert torch.equal(re[q * per:(q + 1) * per].view(torch.int32), r1.view(torch.int32)), q
        assert torch.equal(im[q * per:(q + 1) * per].view(torch.int32), i1.view(torch.int32)), q
        assert torch.isfinite(r1).all() and torch.isfinite(i1).all(), q
    del re, im, r1, i1
    torch.cuda.empty_cache()


def test_batch_device_refuses_bad_arguments(results):
    import torch
    o, _, _ = results("r6full")
    n, half = 64, 32
    x = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * (half + 1) * n, dtype=torch.float32, device="cuda")
    fn = batch_fn(o)
    s = torch.cuda.current_stream().cuda_stream
    xp, op = x.data_ptr(), out.data_ptr()
    for a in ((None, xp, 1, n, 0, half, op, op, None, None), (o._obj, None, 1, n, 0, half, op, op, None, None),
              (o._obj, xp, 1, n, 0, half, op, None, None, None), (o._obj, xp, 1, n, 0, half, None, op, None, None),
              (o._obj, xp, 1, n, 0, half, op, op, op, None), (o._obj, xp, 1, n, 0, half, op, op, None, op),
              (o._obj, xp, 1, n, 0, half, None, None, None, None), (o._obj, xp, 0, n, 0, half, op, op, None, None),
              (o._obj, xp, -1, n, 0, half, op, op, None, None), (o._obj, xp, 1, n - 1, 0, half, op, op, None, None),
              (o._obj, xp, 1, n, -1, half, op, op, None, None), (o._obj, xp, 1, n, 5, 4, op, op, None, None),
              (o._obj, xp, 1, n, 0, half + 1, op, op, None, None)):
        assert fn(*a, s) == -6, a
    torch.cuda.synchronize()
    assert not out.any()


def test_host_entry_clamps_and_refuses_a_reversed_range(results):
    o, _, out = results("r6full")
    rows, _ = out[(0, 32)]
    x = fc.inputs("r6full")[0]
    got = host_entry(o, x, -5, 99)  # clamped to 0 ... N/2 like the reference: 33 of the 105 rows asked for
    assert same_bits(got[:33], rows[0]) and np.isnan(got[33:].view(np.float32)).all()
    with pytest.raises(RuntimeError, match="minIndex"):
        host_entry(o, x, 9, 3)
    assert np.isnan(host_entry.last.view(np.float32)).all(), "a refused call wrote"
    with pytest.raises(RuntimeError, match="minIndex"):
        host_entry(o, x, 40, 45)  # maxIndex is taken as 32
    assert np.isnan(host_entry.last.view(np.float32)).all(), "a refused call wrote"


def test_multi_channel_input_keeps_its_leading_axes(results):
    _, _, out = results("r9default")
    rows, _ = out[(1, 255)]
    x = fc.inputs("r9default")
    w = af.FST(radix2_exp=9)
    xs = np.stack([x, x[::-1]])  # (2, 3, N)
    m = w.fst(xs)
    assert m.shape == (2, 3, 255, 512) and m.dtype == np.complex64
    assert same_bits(m[0], rows) and same_bits(m[1, 0], rows[2])
    assert w.fst(x[0][:300]).shape == (255, 512)  # zero-padded like the reference wrapper
    assert len(w.y_coords()) == w.num + 1 and len(w.x_coords()) == w.fft_length + 1
    assert np.array_equal(w.get_fre_band_arr(), np.arange(1, 256, dtype=np.float32) * 32000 / 512)


def test_constructor_raises_the_reference_wrappers_value_errors():
    for kw in (dict(min_index=0), dict(radix2_exp=6, max_index=32), dict(radix2_exp=6, min_index=7, max_index=7),
               dict(radix2_exp=6, min_index=9, max_index=4)):
        with pytest.raises(ValueError):
            af.FST(**kw)
    with pytest.raises(RuntimeError, match="status -4"):
        af.FST(radix2_exp=15)
