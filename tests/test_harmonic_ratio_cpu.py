"""CPU-only checks of the harmonic ratio: the exports and their prototypes against the reference header, the wrapper's
signature, afx_harmonic_ratio_plan_host against the compiled reference's constructor (every fixture case, NULL arguments,
the lowFre and slide fallbacks, the ignored window argument; the window table bit-equal; against the fixture where
oracle/_ref is absent), the refusals, the float64 restatement against the compiled reference on every case, and the
fixture."""
import inspect
import os
import re

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import harmonic_ratio_cases as hc
from tests import harmonic_ratio_restate as hr
from tests.harmonic_ratio_check import check_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("new", "calTimeLength", "harmonicRatio", "free")
EXTRA = ("harmonicRatioBatchDevice", "curveBatchDevice", "maxLength", "windowLength")


@pytest.fixture(scope="module")
def lib():
    lib = af.get_lib()
    assert hasattr(lib, "harmonicRatioObj_new") and hasattr(lib, "afx_harmonic_ratio_plan_host")
    return hc.bind_device(lib)


@pytest.fixture(scope="module")
def rlib():
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    return hc.bind(ref.lib())


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(hc.GOLDEN, "harmonic_ratio.npz"))


def _protos(text, prefix):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for ret, name, args in re.findall(r"(\w[\w\s\*]*?)\b(" + prefix + r"_\w+)\s*\(([^)]*)\)\s*;", text):
        norm = [re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", " * ", a)).strip() for a in args.split(",")]
        out[name] = (" ".join(ret.split()), norm)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_exports_and_prototypes_equal_the_reference_header(lib):
    prefix = "harmonicRatioObj"
    for n in ENTRY + EXTRA:
        assert hasattr(lib, f"{prefix}_{n}"), n
    ours = _protos(open(os.path.join(ROOT, "include", "mir", "harmonicRatio_algorithm.h")).read(), prefix)
    assert set(ours) == {f"{prefix}_{n}" for n in ENTRY + EXTRA}
    assert "harmonicRatio" not in open(os.path.join(ROOT, "include", "afx_batch.h")).read()
    path = os.path.join(os.path.dirname(ROOT), "reference", "src", "mir", "harmonicRatio_algorithm.h")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    theirs = _protos(open(path).read(), prefix)
    assert set(theirs) == {f"{prefix}_{n}" for n in ENTRY}
    assert {n: ours[n] for n in theirs} == theirs


def test_wrapper_signature():
    sig = inspect.signature(af.HarmonicRatio.__init__)
    got = [(p.name, p.default) for p in list(sig.parameters.values())[1:]]
    assert [n for n, _ in got] == ["samplate", "low_fre", "radix2_exp", "window_type", "slide_length"]
    assert (got[0][1], got[2][1], got[3][1], got[4][1]) == (32000, 12, af.WindowType.HAMM, 1024)
    assert abs(got[1][1] - 32.70319566257483) < 1e-12  # note_to_hz('C1')
    assert "HarmonicRatio" in af.__all__
    for m in ("cal_time_length", "harmonic_ratio", "harmonic_ratio_batch_device", "curve_batch_device"):
        assert callable(getattr(af.HarmonicRatio, m))


# (samplate, lowFre, radix2Exp, windowType, slideLength) beyond the fixture's: NULLs (window 2048), lowFre at and beyond
# samplate / 2 (9000 and 8000 at 16 kHz fall back to 25, 7999 does not; 8001 / 2 is 4000), samplate out of range, non-positive
# slides, a window argument nobody reads, maxLength capped
GRID = [(None, None, None, None, None), (16000, 9000.0, 8, None, None), (16000, 8000.0, 8, None, None), (16000, 7999.0, 8, None, None),
        (8001, 4000.0, 7, None, 16), (8001, 3999.5, 7, None, 16), (16000, 0.0, 9, None, 100), (16000, -3.0, 9, None, 100),
        (0, 30.0, 10, None, None), (200000, 30.0, 10, None, None), (196000, 30.0, 10, None, 0), (16000, 64.0, 8, None, -5),
        (16000, 64.0, 8, 1, 64), (16000, 64.0, 8, 2, 64), (16000, 64.0, 8, 9, 64), (44100, 10.0, 6, None, None),
        (22051, 90.3, 12, None, 5000), (32000, None, 11, None, None), (None, 100.5, None, 0, 300)]


def test_plan_equals_the_reference_constructor(lib, rlib):
    """every field the reference's constructor decides and the window it builds, read from the object it built"""
    for args in [hc.ctor_args(n) for n in hc.CASES] + GRID:
        st, p = hc.plan(lib, *args)
        rst, robj = hc.new(rlib, *args)
        assert st == 0 and rst == 0, args
        f, w = hc.ref_fields(robj), hc.ref_window(robj)
        rlib.harmonicRatioObj_free(robj)
        assert {k: p[k] for k in f} == f, (args, p, f)
        assert p["fftLength"] == 2 * p["windowLength"] == 2 << p["radix2Exp"] and 2 <= p["maxLength"] <= p["windowLength"] - 1
        assert same_bits(p["window"], w), args


def test_defaults_fallbacks_and_the_lds_budget(lib, gold):
    st, p = hc.plan(lib)
    assert (st, p["samplate"], p["lowFre"], p["radix2Exp"], p["windowLength"], p["fftLength"], p["slideLength"], p["maxLength"]) == \
        (0, 32000, 25.0, 11, 2048, 4096, 512, 1280)
    st, p = hc.plan(lib, r=12)  # what the wrapper passes
    assert (p["windowLength"], p["fftLength"], p["slideLength"], p["maxLength"]) == (4096, 8192, 1024, 1280)
    assert p["ldsBytes"] == 256 + 8 * (8192 + 256 + 1) <= 80 * 1024  # two workgroups share a CU's 160 KB
    for r in range(6, 13):
        assert hc.plan(lib, r=r)[1]["ldsBytes"] == 256 + 8 * ((2 << r) + (2 << r >> 5) + 1)
    assert [hc.plan(lib, sr=16000, lo=lo, r=8)[1]["lowFre"] for lo in (9000.0, 8000.0, 7999.0)] == [25.0, 25.0, 7999.0]
    assert hc.plan(lib, sr=16000, lo=7999.0, r=8)[1]["maxLength"] == 2
    assert hc.plan(lib, sr=16000, lo=20.0, r=7)[1]["maxLength"] == 127  # capped at N - 1
    assert [hc.plan(lib, r=8, hop=h)[1]["slideLength"] for h in (None, 0, -4, 1, 5000)] == [64, 64, 64, 1, 5000]
    base = hc.plan(lib, sr=16000, lo=64.0, r=8, hop=64)[1]
    for window in (0, 1, 2, 9):  # read by nobody: always the Hamming table
        p = hc.plan(lib, sr=16000, lo=64.0, r=8, window=window, hop=64)[1]
        assert same_bits(p.pop("window"), base["window"]) and p == {k: v for k, v in base.items() if k != "window"}
    # the periodic Hamming window, as stored from the reference's object
    for N in (64, 128, 256):
        assert same_bits(hc.plan(lib, r=N.bit_length() - 1)[1]["window"], gold[f"window/{N}"])
    n = np.arange(256)
    assert np.abs(base["window"] - (0.54 - 0.46 * np.cos(2 * np.pi * n / 256))).max() < 1e-6


def test_plan_equals_the_fixture(lib, gold):
    """without the compiled reference: what it decided for the fixture's cases, as stored"""
    for name in hc.CASES:
        st, p = hc.plan(lib, *hc.ctor_args(name))
        assert st == 0, name
        assert [p["windowLength"], p["fftLength"], p["slideLength"], p["maxLength"]] == gold[name + "/plan"].tolist(), name


def test_refusals(lib):
    for r in (5, 13, 0, -1, 31):
        st, obj = hc.new(lib, r=r)
        assert st == -100 and not obj
        st, p = hc.plan(lib, r=r)
        assert st == -100 and p["window"] is None
    assert lib.harmonicRatioObj_new(None, None, None, None, None, None) == -1
    assert lib.harmonicRatioObj_calTimeLength(None, 5000) == 0
    assert lib.harmonicRatioObj_maxLength(None) == 0 and lib.harmonicRatioObj_windowLength(None) == 0
    lib.harmonicRatioObj_free(None)
    with pytest.raises(RuntimeError, match="-100"):
        af.HarmonicRatio(radix2_exp=13, slide_length=2048)
    with pytest.raises(RuntimeError, match="-100"):
        af.HarmonicRatio(radix2_exp=5, slide_length=8)


def test_cal_time_length_equals_the_reference(rlib):
    """(the library's own object needs a device: tests/test_harmonic_ratio_gpu.py, tests/test_harmonic_ratio_hoststub.py)"""
    for r, hop in ((8, 64), (8, 300), (10, 333)):
        rst, robj = hc.new(rlib, 16000, 80.0, r, None, hop)
        assert rst == 0
        for n in (0, (1 << r) - 1, 1 << r, (1 << r) + hop - 1, (1 << r) + hop, 5 * (1 << r) + 17):
            assert rlib.harmonicRatioObj_calTimeLength(robj, n) == hc.frames(n, r, hop), (r, hop, n)
        rlib.harmonicRatioObj_free(robj)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_restatement_against_the_compiled_reference(name, rlib, gold):
    """the reference's values under the acceptance rule, and equal to what the fixture stores"""
    from tests.golden.make_harmonic_ratio_golden import reference_case
    value, eps, frames, f, window = reference_case(rlib, name)
    w = check_case(name, frames, eps, value, f["maxLength"])
    assert w["explained"] == 0
    assert same_bits(gold[name + "/value"], value) and np.array_equal(gold[name + "/eps"], eps)
    assert gold[name + "/plan"].tolist() == [f["windowLength"], f["fftLength"], f["slideLength"], f["maxLength"]]
    assert gold[name + "/first"].tolist() == [fr["first"] for fr in frames] and gold[name + "/lag"].tolist() == [fr["lag"] for fr in frames]
    # what the reference's distance from float64 is outside the ill-conditioned frames: well below the floor of the rule
    if name != "step_r10":
        off = np.abs(value.astype(np.float64) - [fr["value"] for fr in frames])
        assert off.max() <= 1.1e-6 and (eps == np.float32(1e-5)).all(), (name, off.max())


def test_fixture_self_check(lib, gold):
    """every case is there with 3 ... 10 frames; the stored decisions are the restatement's; the classes the cases are there for
    occur; the file stays small"""
    assert os.path.getsize(os.path.join(hc.GOLDEN, "harmonic_ratio.npz")) < 64 * 1024
    assert len(hc.CASES) == 16 and set(hc.SMALL) <= set(hc.CASES)
    for name, c in hc.CASES.items():
        r, hop, T = c[2], c[3], c[5]
        st, p = hc.plan(lib, *hc.ctor_args(name))
        assert st == 0 and hc.frames(hc.data_length(name), r, hop) == T and 3 <= T <= 10
        value, eps, first, lag = (gold[f"{name}/{k}"] for k in ("value", "eps", "first", "lag"))
        assert len(value) == len(eps) == len(first) == len(lag) == T and (eps >= np.float32(1e-5)).all() and np.isfinite(value).all()
        frames = hr.harmonic_ratio(hc.case_input(name), p["window"], r, hop, p["maxLength"])
        assert [fr["first"] for fr in frames] == first.tolist() and [fr["lag"] for fr in frames] == lag.tolist(), name
        assert np.allclose(gold[name + "/value64"], [fr["value"] for fr in frames], rtol=1e-9, atol=1e-12), name
        check_case(name + " (stored)", frames, eps, value, p["maxLength"])
    found = {n: [fr["own"] is not None for fr in hr.harmonic_ratio(hc.case_input(n), hc.plan(lib, *hc.ctor_args(n))[1]["window"],
                                                                  hc.CASES[n][2], hc.CASES[n][3], int(gold[n + "/plan"][3]))]
             for n in ("carry_r8", "dc_r8")}
    assert found["carry_r8"] == [True] * 3 + [False] * 7 and gold["carry_r8/first"].tolist()[2:] == [2] * 8
    assert not any(found["dc_r8"]) and not gold["dc_r8/first"].any() and (np.abs(gold["dc_r8/value"] - 0.99985) < 1e-4).all()
    assert gold["short_r8/plan"][3] == 4 and gold["short_r8/lag"][3] == -1 and gold["short_r8/value"][3] == 0
    assert gold["cap_r7/plan"][3] == 127 and not gold["zero_r9/value"].any()
    rs = [c[2] for c in hc.CASES.values()]
    assert {6, 7, 8, 9, 10, 11, 12} <= set(rs) and rs.count(12) == 1
    assert any(c[3] > (1 << c[2]) for c in hc.CASES.values()) and any(c[3] % 2 for c in hc.CASES.values())
