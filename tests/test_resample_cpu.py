"""CPU-only checks of the resampler (include/dsp/resample_algorithm.h), no device needed: the numpy restatement
(tests/resample_restate.py: float32 phase, float64 sums) against the compiled reference's outputs on every case of
tests/resample_cases.py, its exact-phase variant as the control of the GPU tests, the host table of the plan functions
against the float64 closed form, the ratio state machine, the lengths, the launch plan and the refusals.

Measured, restatement vs the compiled reference (peak-relative): 441_16_best 1.17e-6, 441_16_mid 6.8e-7, 441_16_fast 5.1e-7,
48_32_best 7.7e-7, 16_441_mid 4.3e-7, 32_16_fast 4.1e-7, ratio_best 6.1e-7, 2205_16_best 7.9e-7, short_best 1.7e-7, hann_80_9
9.2e-7, gauss_24_7 5.5e-7, tukey_24_7 3.2e-7; asserted: 5e-6.  The exact-phase variant on 441_16_best: 5.9e-4."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import resample_cases as rc
from tests import resample_restate as rr

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    af.get_lib()  # (loads the HIP runtime in the order the package wants)
    return rc.bind(C.CDLL(af.LIB_PATH))  # a handle of its own: the wrapper classes set other argument types on theirs


def _peak(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("name", list(rc.CASES))
def test_restatement_meets_the_reference(name, lib):
    """float32 phase + float64 sums over THIS library's host table: within 5e-6 of the reference (its own float32 sums are
    ~1e-6 off float64; measured worst 1.2e-6, the margin is for other compilers' libm in the table)"""
    c = rc.CASES[name]
    st, p = rc.plan(lib, name)
    assert st == 0
    x = rc.case_input(name)
    want, sel = rc.expected(name)
    m = lib.afx_resample_plan_length(C.byref(p), len(x))
    got = rr.resample(x, p.values(), p.ratio, p.bitLength, m, bool(c.get("scale")))
    lib.afx_resample_plan_free(C.byref(p))
    got = got if sel is None else got[sel]
    assert len(got) == len(want), (name, len(got), len(want))  # the lengths of every case
    if len(want):
        e = _peak(got, want)
        print(f"restatement {name}: {e:.2e}")
        assert e <= 5e-6, (name, e)


def test_exact_phase_is_not_the_reference(lib):
    """the control of the GPU tests' first case: the phase kept in float64 is off by MORE than 1e-4 at 6000 samples, so a
    kernel that 'improves' the index arithmetic fails the 1e-5 bar"""
    name = "441_16_best"
    st, p = rc.plan(lib, name)
    x = rc.case_input(name)
    want, _ = rc.expected(name)
    got = rr.resample(x, p.values(), p.ratio, p.bitLength, len(want), exact_phase=True)
    lib.afx_resample_plan_free(C.byref(p))
    assert _peak(got, want) > 1e-4


# (constructor case, closed-form arguments: zeroNum, nbit, window, value, rollOff)
TABLES = {"441_16_best": (64, 9, rc.KAISER, 14.7696565, 0.9475937), "441_16_mid": (32, 9, rc.KAISER, 11.6625806, 0.8987969),
          "441_16_fast": (16, 9, rc.KAISER, 8.5555046, 0.85), "hann_16_5": (16, 5, rc.HANN, 0.0, 0.945),
          "hann_80_9": (80, 9, rc.HANN, 0.0, 0.945), "gauss_24_7": (24, 7, rc.GAUSS, 3.0, 0.9), "tukey_24_7": (24, 7, rc.TUKEY, 0.4, 0.9)}


@pytest.mark.parametrize("name", list(TABLES))
def test_host_table_is_the_closed_form(name, lib):
    """the born table (times 0.5, exact) against rollOff sinc(rollOff u) w(u) in float64.  Bar 1e-5 of the peak: the float32
    argument of sinf is up to pi zeroNum rollOff ~ 250, half an ulp of that is 7.6e-6 in the sine and 3e-8 after the
    division by the argument; the Kaiser window adds the float32 Bessel series, 15 terms of a few roundings each, at most
    ~50 ulp = 3e-6 of a value <= 1; everything else is single roundings of 6e-8"""
    fn, args = rc.ctor_args(name)
    p = rc.Plan()
    if fn == "resampleObj_new":
        st = lib.afx_resample_plan_host(args[0], None, None, None, None, None, None, None, C.byref(p))
    else:
        st = lib.afx_resample_plan_host(None, *args[:5], None, None, C.byref(p))
    assert st == 0
    z, nb, win, val, ro = TABLES[name]
    assert (p.zeroNum, p.nbit, p.bitLength, p.interpLength, p.winType) == (z, nb, 1 << nb, z * (1 << nb) + 1, win)
    assert (p.ratio, p.p, p.q, p.sourceRate, p.targetRate, p.isScale, p.isContinue) == (0.5, 1, 2, 32000, 16000, 0, 0)
    got = p.values().astype(np.float64) / 0.5
    lib.afx_resample_plan_free(C.byref(p))
    want = rr.table(z, nb, win, val, ro)
    e = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"table {name}: {e:.2e}")
    assert e <= 1e-5, (name, e)
    assert got[0] == pytest.approx(ro, rel=1e-6)  # rollOff at the centre


def test_constructor_fallbacks(lib):
    """value 0 -> 5 (Kaiser) / 2.5 (Gauss), types <= Rect -> Hann, out-of-range values -> defaults"""
    def plan(z, nb, wt, val, ro):
        p = rc.Plan()
        o = rc._opt
        assert lib.afx_resample_plan_host(None, o(C.c_int, z), o(C.c_int, nb), o(C.c_int, wt), o(C.c_float, val), o(C.c_float, ro),
                                          None, None, C.byref(p)) == 0
        out = (p.zeroNum, p.nbit, p.winType, p.value, p.rollOff, p.values())
        lib.afx_resample_plan_free(C.byref(p))
        return out
    assert plan(8, 4, rc.KAISER, 0.0, 0.9)[3] == 5.0 and plan(8, 4, rc.GAUSS, 0.0, 0.9)[3] == 2.5
    assert plan(8, 4, rc.KAISER, None, 0.9)[3] == 0.0  # (value NULL: the window's own default, 5)
    assert np.array_equal(plan(8, 4, rc.KAISER, None, 0.9)[5], plan(8, 4, rc.KAISER, 5.0, 0.9)[5])
    assert np.array_equal(plan(8, 4, rc.GAUSS, None, 0.9)[5], plan(8, 4, rc.GAUSS, 2.5, 0.9)[5])
    assert plan(8, 4, 0, None, 0.9)[2] == rc.HANN and plan(8, 4, -3, None, 0.9)[2] == rc.HANN
    assert plan(0, 30, rc.HANN, -1.0, 1.5)[:5] == (64, 9, rc.HANN, 0.0, f32(0.945))
    assert plan(None, None, None, None, None)[:5] == (64, 9, rc.HANN, 0.0, f32(0.945))
    # Tukey: alpha 0 is the rectangle, 1 the Hann window
    assert np.array_equal(plan(8, 4, rc.TUKEY, 1.0, 0.9)[5], plan(8, 4, rc.HANN, None, 0.9)[5])
    u = np.arange(8 * 16 + 1) / 16
    assert np.allclose(plan(8, 4, rc.TUKEY, 0.0, 0.9)[5] / 0.5, 0.9 * np.sinc(0.9 * u), atol=1e-6)


def test_ratio_state_machine(lib):
    """0.5 -> 16000 / 44100 -> 2.0 -> 0.7123: divide by the old ratio if it was < 1, multiply by the new one if it is < 1,
    float32, in this order -- bit for bit; rates that are equal or not positive, and negative ratios, change nothing"""
    p = rc.Plan()
    assert lib.afx_resample_plan_host(C.pointer(C.c_int(rc.FAST)), None, None, None, None, None, None, None, C.byref(p)) == 0
    t = p.values()
    r1 = f32(16000) / f32(44100)
    steps = []
    for rates in ((44100, 16000), (44100, 44100), (0, 16000), (16000, -1), (16000, 32000), -0.5, 0.7123):
        if isinstance(rates, tuple):
            assert lib.afx_resample_plan_rate(C.byref(p), rates[0], rates[1], 0.0) == 0
        else:
            assert lib.afx_resample_plan_rate(C.byref(p), 0, 0, rates) == 0
        steps.append((p.ratio, p.p, p.q, p.sourceRate, p.targetRate, p.step, p.values()))
    t1 = (t / f32(0.5)) * r1
    t2 = t1 / r1
    t3 = t2 * f32(0.7123)
    assert steps[0][:6] == (r1, 160, 441, 44100, 16000, 185) and np.array_equal(steps[0][6], t1)
    for s in steps[1:4]:  # ignored
        assert s[:6] == steps[0][:6] and np.array_equal(s[6], t1)
    assert steps[4][:6] == (2.0, 2, 1, 16000, 32000, 512) and np.array_equal(steps[4][6], t2)
    assert steps[5][:6] == steps[4][:6] and np.array_equal(steps[5][6], t2)
    assert steps[6][:6] == (f32(0.7123), 0, 0, 16000, 32000, 364) and np.array_equal(steps[6][6], t3)
    # between two ratios >= 1 the table stays as it is
    assert lib.afx_resample_plan_rate(C.byref(p), 0, 0, 3.0) == 0 and lib.afx_resample_plan_rate(C.byref(p), 0, 0, 1.5) == 0
    assert np.array_equal(p.values(), t2 * f32(0.7123) / f32(0.7123)) and p.ratio == 1.5
    lib.afx_resample_plan_free(C.byref(p))


def test_lengths_and_continue_remainders(lib):
    """floorf(dataLength * ratio) as an int x float32 product; with isContinue (dataLength - dataLength % q) p / q, and 0
    for q <= 1"""
    p = rc.Plan()
    one = C.pointer(C.c_int(1))
    assert lib.afx_resample_plan_host(C.pointer(C.c_int(rc.BEST)), None, None, None, None, None, None, None, C.byref(p)) == 0
    L = lambda n: lib.afx_resample_plan_length(C.byref(p), n)  # noqa: E731
    assert [L(n) for n in (4001, 1, 0, -5)] == [2000, 0, 0, 0]
    lib.afx_resample_plan_rate(C.byref(p), 44100, 16000, 0.0)
    r = f32(16000) / f32(44100)
    for n in (1, 2, 3, 40, 6000, 441, 44100, 300000, 1323000, 2 ** 24 + 1, 2 ** 30):
        assert L(n) == int(np.floor(f32(n) * r)), n
    assert L(44100) == 16000 and L(1323000) == 480000
    lib.afx_resample_plan_free(C.byref(p))
    assert lib.afx_resample_plan_host(C.pointer(C.c_int(rc.BEST)), None, None, None, None, None, None, one, C.byref(p)) == 0
    assert p.isContinue == 1 and [L(n) for n in (4001, 1, 2)] == [2000, 0, 1]
    lib.afx_resample_plan_rate(C.byref(p), 44100, 16000, 0.0)
    assert [L(n) for n in rc.PIECES] == [320, 0, 1600] and L(440) == 0 and L(441) == 160 and L(2 ** 30) == (2 ** 30 // 441) * 160
    lib.afx_resample_plan_rate(C.byref(p), 16000, 32000, 0.0)  # q = 1
    assert (p.p, p.q) == (2, 1) and L(1000) == 0
    lib.afx_resample_plan_rate(C.byref(p), 0, 0, 0.4)           # q = 0
    assert (p.p, p.q) == (0, 0) and L(1000) == 0
    lib.afx_resample_plan_free(C.byref(p))


def test_launch_plan(lib):
    """Best / Mid / Fast keep 128 / 64 / 32 KB tables in LDS beside the staged input of up to 4 clips, within 160 KB; a table
    above that is read from global memory"""
    for name, tab_kb, in_lds in (("441_16_best", 128, 1), ("441_16_mid", 64, 1), ("441_16_fast", 32, 1), ("hann_80_9", 160, 0)):
        st, p = rc.plan(lib, name)
        assert st == 0 and p.tableInLds == in_lds and p.group in (1, 2, 4) and p.step == 185
        assert p.taps == p.interpLength // p.step
        assert p.ldsBytes <= 160 * 1024 and (p.ldsBytes >= tab_kb * 1024 if in_lds else p.ldsBytes < 64 * 1024)
        lib.afx_resample_plan_free(C.byref(p))


def test_refusals_without_a_device(lib):
    p = rc.Plan()
    o = rc._opt
    assert lib.afx_resample_plan_host(None, o(C.c_int, 1 << 16), o(C.c_int, 9), None, None, None, None, None, C.byref(p)) == -4
    assert "2^24" in af.last_error()
    assert lib.afx_resample_plan_host(None, o(C.c_int, 1 << 15), o(C.c_int, 9), None, None, None, None, None, None) == -6
    h = np.zeros(8, np.float32)
    hp = h.ctypes.data_as(C.c_void_p)
    before = af.get_lib().afx_error_count()
    assert lib.resampleObj_resample(None, hp, 8, hp) == -6 and af.get_lib().afx_error_count() > before
    assert lib.resampleObj_resampleBatchDevice(None, hp, 1, 8, 8, hp, 8, None) == -6
    assert lib.resampleObj_calDataLength(None, 100) == 0
    lib.resampleObj_setSamplate(None, 44100, 16000)
    lib.resampleObj_setSamplateRatio(None, 0.5)
    lib.resampleObj_enableContinue(None, 1)
    lib.resampleObj_free(None)
    obj = C.c_void_p(None)
    assert lib.resampleObj_newWithWindow(C.byref(obj), o(C.c_int, 1 << 16), o(C.c_int, 9), None, None, None, None, None) == -4
    assert not obj
    if af.runtime_status() != 0:  # no device: no object, no CPU path
        assert lib.resampleObj_new(C.byref(obj), None, None, None) == -2 and not obj
        with pytest.raises(RuntimeError, match="status -2"):
            af.Resample()
        with pytest.raises(RuntimeError, match="status -2"):
            af.WindowResample()
    with pytest.raises(ValueError):
        af.Resample("finest")
    assert af.ResampleQualityType.BEST == 0 and af.ResampleQualityType.FAST == 2


def test_phase_arithmetic_of_the_header():
    """afx_resample_phase (afx_device.h, compiled here as plain C with the kernel's own expressions) gives the restatement's
    integers and weights: checked through the emulated kernel and the GPU; here the float32 facts it rests on"""
    r = f32(16000) / f32(44100)
    i = np.arange(1, 400000, 37, dtype=np.float64)
    t = (i / float(r)).astype(f32)
    frac = t - np.floor(t)
    fv = (f32(r) * frac).astype(f32) * f32(512)
    assert np.array_equal(fv.astype(np.float64), (f32(r) * frac).astype(np.float64) * 512)      # the power of two is exact
    assert np.array_equal((fv - np.floor(fv)).astype(np.float64), fv.astype(np.float64) - np.floor(fv).astype(np.float64))
    assert (np.diff(np.floor(t)) >= 0).all()                                                      # n is monotonic in i
