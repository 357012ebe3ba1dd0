"""CPU-only: the FST plan (afx_fst_plan_host, no device) against the partition lengths and the row map of the float64
restatement; the restatement of tests/fst_cases.py in its two forms and against the compiled reference; the stored fixture
against the compiled reference, bit for bit; the condition on the case table; the status codes that need no device."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import fst_cases as fc

ip = C.POINTER(C.c_int)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def compiled():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the compiled reference")
    from tests.golden import make_fst_golden as mk
    return mk, mk.bind(ref.lib())


def plan_host(r):
    fn = af.get_lib().afx_fst_plan_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int, ip, ip]
    half = 1 << (r - 1)
    cell, ln = np.full(half + 1, -7, np.int32), np.full(half + 1, -7, np.int32)
    assert fn(r, cell.ctypes.data_as(ip), ln.ctypes.data_as(ip)) == 0
    return cell, ln


@pytest.mark.parametrize("r", range(3, 15))
def test_plan_host_equals_the_partitions_of_the_restatement(r):
    """index f shows full-matrix row N/2 - f; partition i (length n, cumulative end c_i) owns rows N - c_i ... N - c_i + n - 1;
    the cells are the partitions from bin -1 on, in order"""
    N = 1 << r
    l = fc.lens(r)
    assert sum(l) == N and len(l) == 2 * r
    end = np.cumsum(l)
    owner = np.zeros(N, np.int64)
    for i, n in enumerate(l):
        owner[N - end[i]:N - end[i] + n] = i
    first = {i: int(sum(l[r - 1:i])) for i in range(r - 1, 2 * r)}  # first cell of a visible partition
    cell, ln = plan_host(r)
    for f in range(N // 2 + 1):
        i = int(owner[N // 2 - f])
        assert i >= r - 1, "a negative band is shown"
        assert (cell[f], ln[f]) == (first[i], l[i]), (r, f)
    assert first[2 * r - 1] + l[-1] == N // 2 + 1
    c2, l2 = fc.row_map(r)
    assert np.array_equal(cell, c2) and np.array_equal(ln, l2)
    fn = af.get_lib().afx_fst_plan_host
    assert fn(r, None, None) == 0


def test_plan_host_refuses_what_the_reference_refuses():
    fn = af.get_lib().afx_fst_plan_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int, ip, ip]
    assert fn(2, None, None) == -1 and fn(0, None, None) == -1 and fn(-3, None, None) == -1


@pytest.mark.parametrize("r", [3, 4, 5, 8])
def test_the_two_forms_of_the_restatement_agree(r):
    """cells64 + expand is f64_fst without the N x N matrix: bit for bit"""
    N = 1 << r
    x = (0.1 * np.random.default_rng(r).standard_normal(N)).astype(np.float32)
    for lo, hi in ((0, N // 2), (1, N // 2 - 1), (2, 2)):
        assert np.array_equal(fc.f64_fst(x, r, lo, hi), fc.expand(fc.cells64(x, r), r, lo, hi))


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_every_band_of_the_table_is_visible_above_the_bar(name):
    """noise and impulse: every band's float64 peak is at least 1e-3 of the chunk's, so a wholly wrong band cannot hide under a
    bar of 1e-5 of the chunk's peak"""
    c, ref = fc.by_name(name), fc.reference(name)
    for k in (0, 2):
        peaks = fc.band_peaks(ref.cells64[k], c.r)
        assert len(peaks) == c.r + 1
        assert peaks.min() >= fc.BAND_FLOOR * ref.peak[k], (name, fc.INPUTS[k], peaks / ref.peak[k])
    assert np.all(ref.r_ref <= 0.5 * fc.FLOOR), "the reference itself is near the bar: look at it"


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_restatement_meets_the_stored_reference(name):
    """float64 vs the stored compiled-reference cells on the metric of the GPU tests; the recorded value is that one"""
    ref = fc.reference(name)
    for k in range(3):
        e = np.abs(ref.cells_c[k] - ref.cells64[k]).max() / ref.peak[k]
        assert e == ref.r_ref[k] and e <= 1e-6, (name, fc.INPUTS[k], e)


@pytest.mark.parametrize("r,lo,hi", [(3, 0, 4), (4, 0, 8), (5, 1, 15), (8, 0, 128), (10, 1, 511), (12, 2040, 2048)])
def test_restatement_meets_the_compiled_reference(r, lo, hi, compiled):
    mk, L = compiled
    N = 1 << r
    rng = np.random.default_rng(100 + r)
    obj = C.c_void_p(None)
    assert L.fstObj_new(C.byref(obj), r) == 0
    for x in ((0.1 * rng.standard_normal(N)).astype(np.float32),
              (0.1 * np.sin(2 * np.pi * 0.1037 * np.arange(N)) + 0.01 * rng.standard_normal(N)).astype(np.float32)):
        got = mk.ref_rows(L, obj, x, r, lo, hi)
        cells = fc.cells64(x, r)
        e = np.abs(got - fc.expand(cells, r, lo, hi)).max() / np.abs(cells).max()
        assert e <= 1e-6, (r, e)
    L.fstObj_free(obj)


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_fixture_reproduces_and_the_reference_rows_expand_its_cells(name, compiled):
    """every stored array again from the compiled reference, bit for bit; the reference's rows of the case's ranges are
    bitwise the expansion of the stored cells"""
    mk, L = compiled
    c = fc.by_name(name)
    gold = np.load(fc.GOLDEN)
    fresh = mk.case_data(L, c)
    assert set(fresh) == {k for k in gold.files if k.startswith(name + "/")}
    for k, v in fresh.items():
        g = gold[k]
        assert g.dtype == v.dtype and g.shape == v.shape and g.tobytes() == v.tobytes(), k
    obj = C.c_void_p(None)
    assert L.fstObj_new(C.byref(obj), c.r) == 0
    for k in c.chunks:
        for lo, hi in c.ranges:
            rows = mk.ref_rows(L, obj, fc.inputs(name)[k], c.r, lo, hi)
            assert same_bits(rows, fc.expand(gold[f"{name}/{fc.INPUTS[k]}/cells"], c.r, lo, hi)), (name, k, lo, hi)
    L.fstObj_free(obj)


def test_new_status_codes_without_a_device():
    """-1 below 3 as the reference, -4 for 3 and above 14; a supported size reaches the device layer: 0, or -2 without one"""
    lib = af.get_lib()
    fn = lib.fstObj_new
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int]
    for r, want in ((-1, -1), (0, -1), (2, -1), (3, -4), (15, -4), (16, -4), (30, -4)):
        o = C.c_void_p(1)
        assert fn(C.byref(o), r) == want and not o, r
    o = C.c_void_p(None)
    st = fn(C.byref(o), 10)
    assert st in (0, -2) and bool(o) == (st == 0)
    if st == 0:
        lib.fstObj_free.argtypes, lib.fstObj_free.restype = [C.c_void_p], None
        lib.fstObj_free(o)
    lib.fstObj_getCellLength.argtypes, lib.fstObj_getCellLength.restype = [C.c_void_p], C.c_int
    assert lib.fstObj_getCellLength(None) == 0


def test_wrapper_raises_the_reference_wrappers_value_errors():
    for kw in (dict(min_index=0), dict(radix2_exp=6, max_index=32), dict(radix2_exp=6, min_index=7, max_index=7),
               dict(radix2_exp=6, min_index=9, max_index=4)):
        with pytest.raises(ValueError):
            af.FST(**kw)
