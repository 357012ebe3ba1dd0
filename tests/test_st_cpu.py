"""CPU-only: the restatement of tests/st_cases.py against the stored and the freshly compiled reference; the window
coefficients of afx_st_plan_host (no device) against the restatement's; the stored fixture against the compiled reference,
bit for bit; the status codes that need no device; the wrapper's ValueErrors."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import st_cases as sc

fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def compiled():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the compiled reference")
    from tests.golden import make_st_golden as mk
    return mk, mk.bind(ref.lib())


def plan_host(r, factor, norm):
    fn = af.get_lib().afx_st_plan_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_float, C.c_float, fp]
    coef = np.full((1 << (r - 1)) + 1, 7.0, np.float32)
    assert fn(r, factor, norm, coef.ctypes.data_as(fp)) == 0
    return coef


@pytest.mark.parametrize("factor,norm", [(1.0, 1.0), (2.5, 0.8), (0.5, 1.5), (3.0, 0.3)])
def test_plan_host_meets_the_coefficients_of_the_restatement(factor, norm):
    """The library forms c_k as the reference does: powf(k, 2 norm) rounded to float32 (within 1 ulp of k^(2 norm)), then a
    double quotient rounded to float32 again; the restatement rounds the float64 value once.  A denominator off by one
    float32 ulp moves the quotient by up to one ulp before its own rounding: 2 ulps allowed (1 seen)."""
    for r in range(4, 15):
        got, want = plan_host(r, factor, norm), sc.coef32(r, factor, norm)
        assert got[0] == 0.0 and np.all(got[1:] < 0)
        d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        assert d <= 2, (r, factor, norm, d)


def test_plan_host_refuses_bad_arguments():
    fn = af.get_lib().afx_st_plan_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_float, C.c_float, fp]
    c = np.zeros(4, np.float32)
    assert fn(0, 1.0, 1.0, c.ctypes.data_as(fp)) == -1 and fn(25, 1.0, 1.0, c.ctypes.data_as(fp)) == -1
    assert fn(-2, 1.0, 1.0, c.ctypes.data_as(fp)) == -1 and fn(4, 1.0, 1.0, None) == -1


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_restatement_meets_the_stored_reference(name):
    """float64 vs the stored compiled-reference rows on the metric of the GPU tests: no worse than the value recorded over all
    the case's rows, and that is far below the floor of the bar"""
    c, ref = sc.by_name(name), sc.reference(name)
    for k in c.chunks:
        e = np.abs(sc.select(c, ref.f64[k]) - ref.stored[k]).max() / ref.peak[k]
        assert e <= ref.r_ref[k] <= 0.5 * sc.FLOOR and e <= 1e-6, (name, sc.INPUTS[k], e, ref.r_ref[k])
        if c.store is None:
            assert e == ref.r_ref[k]


@pytest.mark.parametrize("r,lo,hi,factor,norm,bins", [
    (4, 0, 8, None, None, None), (5, 1, 15, 0.7, 1.3, None), (8, 0, 128, None, None, None), (8, 3, 3, 2.0, None, None),
    (10, 1, 511, None, 0.9, None), (10, 1, 2, None, None, (512, 0, 5, 5, 1)), (12, 2040, 2048, None, None, None)])
def test_restatement_meets_the_compiled_reference(r, lo, hi, factor, norm, bins, compiled):
    """fresh inputs; (8, 3, 3): minIndex >= maxIndex is the full range in the reference"""
    mk, L = compiled
    N = 1 << r
    rng = np.random.default_rng(100 + r)
    obj = mk.ref_new(L, r, lo, hi, factor, norm, bins)
    want_bins = list(bins) if bins is not None else list(range(lo, hi + 1)) if lo < hi else list(range(N // 2 + 1))
    for x in ((0.1 * rng.standard_normal(N)).astype(np.float32),
              (0.1 * np.sin(2 * np.pi * 0.1037 * np.arange(N)) + 0.01 * rng.standard_normal(N)).astype(np.float32)):
        got = mk.ref_rows(L, obj, x, r, len(want_bins))
        want = sc.f64_st(x, r, want_bins, factor or 1.0, norm or 1.0)
        e = np.abs(got - want).max() / np.abs(want).max()
        assert e <= 1e-6, (r, e)
    L.stObj_free(obj)


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_fixture_reproduces(name, compiled):
    """every stored array again from the compiled reference, bit for bit"""
    mk, L = compiled
    gold = np.load(sc.GOLDEN)
    fresh = mk.case_data(L, sc.by_name(name))
    assert set(fresh) == {k for k in gold.files if k.startswith(name + "/")}
    for k, v in fresh.items():
        g = gold[k]
        assert g.dtype == v.dtype and g.shape == v.shape and g.tobytes() == v.tobytes(), k


def test_fixture_covers_the_table_and_stays_small():
    import os
    gold = np.load(sc.GOLDEN)
    want = {f"{c.name}/ref_vs_f64" for c in sc.CASES} | {f"{c.name}/{sc.INPUTS[k]}/rows" for c in sc.CASES for k in c.chunks}
    assert set(gold.files) == want
    assert os.path.getsize(sc.GOLDEN) < 600000


def test_new_status_codes_without_a_device():
    """-4 below 4 and above 14; a supported size reaches the device layer: 0, or -2 without one"""
    lib = af.get_lib()
    fn = lib.stObj_new
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, fp, fp]
    for r in (-1, 0, 2, 3, 15, 16, 30):
        o = C.c_void_p(1)
        assert fn(C.byref(o), r, 0, 4, None, None) == -4 and not o, r
    assert "not supported" in af.last_error()
    o = C.c_void_p(None)
    st = fn(C.byref(o), 10, 1, 100, None, None)
    assert st in (0, -2) and bool(o) == (st == 0)
    lib.stObj_getBinLength.argtypes, lib.stObj_getBinLength.restype = [C.c_void_p], C.c_int
    if st == 0:
        assert lib.stObj_getBinLength(o) == 100
        lib.stObj_free.argtypes, lib.stObj_free.restype = [C.c_void_p], None
        lib.stObj_free(o)
    assert lib.stObj_getBinLength(None) == 0
    lib.stObj_stBatchDevice.restype = C.c_int
    lib.stObj_stBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.stObj_stBatchDevice(None, None, 1, 16, None, None, None) == -6


def test_wrapper_raises_the_reference_wrappers_value_errors():
    for kw in (dict(min_index=0), dict(radix2_exp=6, max_index=32), dict(radix2_exp=6, min_index=7, max_index=7),
               dict(radix2_exp=6, min_index=9, max_index=4)):
        with pytest.raises(ValueError):
            af.ST(**kw)
    assert "ST" in af.__all__
