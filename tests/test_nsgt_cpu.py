"""CPU-only: the NSGT plan (afx_nsgt_plan_host, no device) against the compiled reference -- bitwise, the bar
tests/test_host_setup.py sets for windows and band arrays --, the column map against its float32 restatement, the float64
transform of tests/nsgt_cases.py against the stored reference results, and the status codes that need no device."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import nsgt_cases as nc


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gold():
    return np.load(nc.GOLDEN)


@pytest.fixture(scope="module")
def compiled():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the compiled reference")
    from tests.golden import make_nsgt_golden as mk
    return mk, mk.bind(ref.lib())


@pytest.mark.parametrize("name", [c.name for c in nc.CASES])
def test_plan_equals_the_stored_reference_plan_bitwise(name, gold):
    """lengths, offsets, bins, max, total, frequencies and windows of every table case"""
    p = nc.product_plan(name)
    assert same(p.len, gold[f"{name}/len"]) and same(p.bin, gold[f"{name}/bin"]) and same(p.offset, gold[f"{name}/offset"])
    assert (p.max, p.total) == tuple(gold[f"{name}/max_total"])
    assert same(p.fre, gold[f"{name}/fre"])
    assert same(p.window, gold[f"{name}/window"])


def check_against_compiled(compiled, c):
    mk, L = compiled
    st, p = nc.plan_host(af.get_lib(), c)
    assert st == 0, (c, st)
    rst, obj = mk.ref_new(L, c)
    assert rst == 0 and obj, (c, rst)
    g = mk.getters(L, obj, c.num)
    L.nsgtObj_free(obj)
    fb = mk.ref_filter_bank(L, c)
    assert same(fb["len"], g["len"]) and same(fb["fre"], g["fre"]) and same(fb["bin"], g["bin"]), ("resolve() of the table", c)
    assert same(p.len, g["len"]) and same(p.bin, g["bin"]) and same(p.fre, g["fre"]), c
    assert (p.max, p.total) == (g["max"], g["total"]), c
    assert same(p.offset, fb["offset"]) and same(p.window, fb["window"]), c


@pytest.mark.parametrize("name", [c.name for c in nc.CASES])
def test_plan_equals_the_compiled_reference_bitwise(name, compiled):
    check_against_compiled(compiled, nc.by_name(name))


@pytest.mark.parametrize("bank", [nc.EFFICIENT, nc.STANDARD])
def test_every_style_bitwise(bank, compiled):
    """styles 0 ... 10 (Gammatone is taken as Hann, Point as ones) x both bank types"""
    for style in nc.STYLE:
        for normal in ("None", "BandWidth"):
            check_against_compiled(compiled, nc.Case(f"style-{style}", 14, 10, 16000, 50.0, None, 12, 3, bank, "Mel", style, normal))
    # Area is taken as BandWidth
    check_against_compiled(compiled, nc.Case("area", 14, 10, 16000, 50.0, None, 12, 2, bank, "Bark", "Hann", "Area"))


def test_every_scale_bitwise(compiled):
    """scales 0 ... 6 at (num 16, radix2_exp 10, samplate 16000), and minimal lengths 1 and 2"""
    for scale in nc.SCALE:
        for min_len in (3, 1, 2):
            check_against_compiled(compiled, nc.Case(f"scale-{scale}", 16, 10, 16000, 100.0, None, 12, min_len, nc.EFFICIENT, scale,
                                                     "Hann", "BandWidth"))
        check_against_compiled(compiled, nc.Case(f"scale-{scale}", 16, 10, 16000, 100.0, None, 12, 3, nc.STANDARD, scale, "Slaney",
                                                 "None"))


@pytest.mark.parametrize("name", [c.name for c in nc.CASES])
def test_column_map_is_the_float32_search(name):
    c, p = nc.by_name(name), nc.product_plan(name)
    want = nc.colmap_restated(p.len, p.max, c.r, c.sr)
    assert np.array_equal(p.colmap, want)
    # a monotone sample-and-hold that starts at cell 0 and stays inside the band
    assert np.all(np.diff(p.colmap, axis=1) >= 0) and np.all(p.colmap[:, 0] == 0) and np.all(p.colmap < p.len[:, None])


@pytest.mark.parametrize("name", [c.name for c in nc.CASES])
def test_float64_transform_of_the_plan_meets_the_stored_results(name):
    """pins the restatement (cells AND matrices of the compiled reference, at the bar) and r_i <= 2e-6 for every band of every
    case, so that an edit of the table cannot loosen the bar max(1e-5, 2 r_i) silently"""
    ref = nc.reference(name)
    assert ref.r_cells.max() <= 2e-6 and ref.r_rows.max() <= 2e-6, (name, ref.r_cells.max(), ref.r_rows.max())
    from tests.conftest import parity_log
    parity_log(f"nsgt {name}: compiled reference vs float64, cells", ref.r_cells.max(), 2e-6, nc.KIND)
    parity_log(f"nsgt {name}: compiled reference vs float64, matrix", ref.r_rows.max(), 2e-6, nc.KIND)
    # the float64 results themselves pass the comparison they are the reference of (against the stored results)
    worst = nc.judge(name, range(3), ref.cells64, ref.mat64, tag=" float64 restatement")
    assert worst <= 1.0


def _new(lib, *args):
    fn = lib.nsgtObj_new
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_void_p)] + nc.NEW_ARGTYPES
    obj = C.c_void_p(0xdead)
    return fn(C.byref(obj), *args), obj


def test_status_codes_without_a_device():
    lib = af.get_lib()
    none = [None] * 9
    for r in (31, -1):
        st, obj = _new(lib, 84, r, *none)
        assert st == -100 and not obj
    st, obj = _new(lib, 84, 12, None, None, None, None, None, None, nc._pi(7), None, None)
    assert st == 1 and not obj
    for num in (1, 2050):
        st, obj = _new(lib, num, 12, *none)
        assert st == -1 and not obj
    # the octave bank of 100 bands from C1 overflows 8 kHz; a linear bank of 600 bands from 4 kHz overflows too
    st, obj = _new(lib, 100, 12, nc._pi(16000), nc._pf(32.703), *([None] * 7))
    assert st == -1 and not obj
    st, obj = _new(lib, 600, 11, nc._pi(16000), nc._pf(4000.0), None, None, None, None, nc._pi(0), None, None)
    assert st == -1 and not obj
    # a band longer than the chunk (the reference overruns its scratch): refused before any device work
    c = nc.Case("long", 12, 8, 16000, 0.0, None, 12, 300, nc.EFFICIENT, "Mel", "Hann", "BandWidth")
    st, obj = _new(lib, c.num, c.r, *nc.new_args(c))
    assert st == -4 and not obj and "band" in af.last_error()
    st, plan = nc.plan_host(lib, c)
    assert st == -4 and plan is None
    lib.nsgtObj_free.restype, lib.nsgtObj_free.argtypes = None, [C.c_void_p]
    lib.nsgtObj_free(None)


def test_void_entries_report_a_null_object():
    lib = af.get_lib()
    lib.afx_error_count.restype = C.c_int
    before = lib.afx_error_count()
    lib.nsgtObj_nsgt.restype, lib.nsgtObj_nsgt.argtypes = None, [C.c_void_p] * 4
    lib.nsgtObj_nsgt(None, None, None, None)
    lib.nsgtObj_setMinLength.restype, lib.nsgtObj_setMinLength.argtypes = None, [C.c_void_p, C.c_int]
    lib.nsgtObj_setMinLength(None, 5)
    assert lib.afx_error_count() == before + 2 and "NULL object" in af.last_error()
    for name in ("nsgtObj_getMaxTimeLength", "nsgtObj_getTotalTimeLength"):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, [C.c_void_p]
        assert f(None) == 0
    lib.nsgtObj_nsgtBatchDevice.restype = C.c_int
    lib.nsgtObj_nsgtBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 5
    assert lib.nsgtObj_nsgtBatchDevice(None, None, 1, 1, None, None, None, None, None) == -6


def test_no_cpu_fallback_without_device():
    if af.runtime_status() == 0:
        pytest.skip("a device is present; covered by the gpu tests")
    with pytest.raises(RuntimeError, match="status -2"):
        af.NSGT(num=12, radix2_exp=9, samplate=16000, low_fre=0.0, scale_type=af.SpectralFilterBankScaleType.MEL)
    with pytest.raises(ValueError):
        af.NSGT(num=2000, radix2_exp=9)
