"""CPU-only checks of the HPS / LHS pitch trackers: the exports and their prototypes against the reference headers, the
wrappers' signatures, afx_pitch_hs_plan_host against the compiled reference's constructors over a parameter grid (every
fallback, and the places where the two reference constructors differ), the three refusals, calTimeLength of continuing and
non-continuing objects, the float64 restatement against the compiled reference on every case, and the fixture."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import pitch_hs_cases as hc
from tests import pitch_hs_restate as hr
from tests.pitch_hs_check import check_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("new", "calTimeLength", "pitch", "enableDebug", "free")
EXTRA = ("pitchBatchDevice", "curveBatchDevice", "minIndex", "maxIndex", "harmonicCount", "interpLength")


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("samplate", "radix2Exp", "fftLength", "slideLength", "isContinue")] + \
               [("lowFre", C.c_float), ("highFre", C.c_float)] + \
               [(n, C.c_int) for n in ("windowType", "interpLength", "minIndex", "maxIndex", "harmonicCount", "lastBin", "transforms",
                                       "sliceInLds")] + [("sliceFloats", C.c_longlong), ("ldsBytes", C.c_longlong)]


@pytest.fixture(scope="module")
def lib():
    lib = af.get_lib()
    assert hasattr(lib, "pitchHPSObj_new") and hasattr(lib, "pitchLHSObj_new")
    lib.afx_pitch_hs_plan_host.restype = C.c_int
    lib.afx_pitch_hs_plan_host.argtypes = [C.c_int, hc.ip, hc.fp, hc.fp, hc.ip, hc.ip, hc.ip, hc.ip, hc.ip, C.POINTER(Plan)]
    return lib


@pytest.fixture(scope="module")
def rlib():
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    return hc.bind(ref.lib())


def plan(lib, kind, sr=None, lo=None, hi=None, r=None, hop=None, window=None, count=None, cont=None):
    p = Plan()
    o = lambda v, t: None if v is None else C.pointer(t(v))  # noqa: E731
    st = lib.afx_pitch_hs_plan_host(kind, o(sr, C.c_int), o(lo, C.c_float), o(hi, C.c_float), o(r, C.c_int), o(hop, C.c_int),
                                    o(window, C.c_int), o(count, C.c_int), o(cont, C.c_int), C.byref(p))
    return st, p


def _protos(text, prefix):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for ret, name, args in re.findall(r"(\w[\w\s\*]*?)\b(" + prefix + r"_\w+)\s*\(([^)]*)\)\s*;", text):
        norm = [re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", " * ", a)).strip() for a in args.split(",")]
        out[name] = (" ".join(ret.split()), norm)
    return out


@pytest.mark.parametrize("k", ["HPS", "LHS"])
def test_exports_and_prototypes_equal_the_reference_header(k, lib):
    for n in ENTRY + EXTRA:
        assert hasattr(lib, f"pitch{k}Obj_{n}"), n
    ours = _protos(open(os.path.join(ROOT, "include", "mir", f"_pitch_{k.lower()}.h")).read(), f"pitch{k}Obj")
    assert set(ours) == {f"pitch{k}Obj_{n}" for n in ENTRY + EXTRA}
    path = os.path.join(os.path.dirname(ROOT), "reference", "src", "mir", f"_pitch_{k.lower()}.h")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    theirs = _protos(open(path).read(), f"pitch{k}Obj")
    assert set(theirs) == {f"pitch{k}Obj_{n}" for n in ENTRY}
    assert {n: ours[n] for n in theirs} == theirs


def test_wrapper_signatures():
    for cls in (af.PitchHPS, af.PitchLHS):
        sig = inspect.signature(cls.__init__)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
            ("samplate", 32000), ("low_fre", 32.0), ("high_fre", 2000.0), ("radix2_exp", 12), ("slide_length", 1024),
            ("window_type", af.WindowType.HAMM), ("harmonic_count", 5)]
        assert cls.__name__ in af.__all__
        for m in ("cal_time_length", "pitch", "pitch_batch_device", "curve_batch_device"):
            assert callable(getattr(cls, m))


def test_round_power_two(lib):
    for sr, M in ((44100, 32768), (48000, 32768), (16000, 16384), (32000, 32768), (8000, 8192), (24576, 32768), (24575, 16384),
                  (196000, 131072), (256, 256)):
        st, p = plan(lib, hc.HPS, sr=sr, r=6, hi=min(2000.0, sr / 2 - 1.5), count=1)
        assert (st, p.interpLength, hc.round_pow2(sr)) == (0, M, M), sr


GRID = list(itertools.product((None, 8000, 44100, 48000, 0, 200000),             # samplate: default, values, out of range
                              (None, 20.0, 100.5),                               # lowFre: below 27 -> 32
                              (None, 90.0, 1500.7, 3999.0, 4000.0, 30000.0),     # highFre: inside, at samplate / 2, beyond
                              (None, 9),                                         # windowType: Hamm, above Hamm
                              (None, 1, 40, 0)))                                 # harmonicCount


@pytest.mark.parametrize("kind", [hc.HPS, hc.LHS], ids=["HPS", "LHS"])
def test_plan_equals_the_reference_constructor(kind, lib, rlib):
    """every field the reference's constructor decides, read from the object it built; plans this library refuses (-6) are
    those where the reference would read past its spectrum or overrun its frame buffer"""
    seen = {0: 0, -6: 0}
    for sr, lo, hi, window, count in GRID:
        for r, hop in ((10, None), (7, 300)):
            st, p = plan(lib, kind, sr, lo, hi, r, hop, window, count)
            rst, robj = hc.new(rlib, kind, sr, lo, hi, r, hop, window, count)
            assert rst == 0
            f = hc.ref_fields(robj)
            hc.free(rlib, kind, robj)
            what = (sr, lo, hi, r, hop, window, count)
            assert st in (0, -6), what
            seen[st] += 1
            assert (p.fftLength, p.slideLength, p.interpLength, p.minIndex, p.maxIndex, p.harmonicCount) == \
                (f["fftLength"], f["slideLength"], f["interpLength"], f["minIndex"], f["maxIndex"], f["harmonicCount"]), what
            over = f["fftLength"] > f["interpLength"] or f["maxIndex"] * f["harmonicCount"] >= f["interpLength"]
            assert (st == -6) == over, what
    assert seen[0] > 100 and seen[-6] > 20, seen


def test_where_the_two_reference_constructors_differ(lib):
    # a window type above Hamm: HPS keeps Hamm, LHS takes it
    assert plan(lib, hc.HPS, window=5)[1].windowType == 2 and plan(lib, hc.LHS, window=5)[1].windowType == 5
    # the count: LHS clamps to samplate / (maxIndex + 1), HPS runs it as given -- and is refused where that reads past M
    st, p = plan(lib, hc.LHS, sr=8000, hi=3000.0, r=10, count=5)
    assert (st, p.harmonicCount, p.lastBin) == (0, 2, 6000)
    st, p = plan(lib, hc.HPS, sr=8000, hi=3000.0, r=10, count=5)
    assert (st, p.harmonicCount) == (-6, 5)
    st, p = plan(lib, hc.LHS, sr=32000, count=40)
    assert (st, p.harmonicCount) == (0, 15)
    # defaults
    for kind in (hc.HPS, hc.LHS):
        st, p = plan(lib, kind)
        assert (st, p.samplate, p.lowFre, p.highFre, p.radix2Exp, p.slideLength, p.windowType, p.harmonicCount, p.interpLength,
                p.minIndex, p.maxIndex, p.lastBin, p.transforms, p.sliceInLds) == \
            (0, 32000, 32.0, 2000.0, 12, 1024, 2, 5, 32768, 32, 2000, 10000, 5, 1)
        assert p.sliceFloats == 10001 + 10000 // 32 and p.ldsBytes <= 160 * 1024
        # a highFre outside (lowFre, samplate / 2) resets both; samplate / 2 is an integer division
        st, p = plan(lib, kind, sr=8001, lo=100.0, hi=4000.0)
        assert (p.lowFre, p.highFre) == (32.0, 2000.0)
        st, p = plan(lib, kind, sr=8002, lo=100.0, hi=4000.0, r=10, count=1)
        assert (st, p.lowFre, p.highFre) == (0, 100.0, 4000.0)
        # transforms per frame and the slice placement
        assert plan(lib, kind, sr=8000, r=13, count=3)[1].transforms == 1
        assert plan(lib, kind, sr=16000, r=13)[1].transforms == 2
        assert plan(lib, kind, sr=8000, r=6, count=3)[1].transforms == 65
        st, p = plan(lib, kind, sr=32000, hi=15000.0, count=2)
        assert (st, p.sliceInLds, p.lastBin) == (0, 0, 30000)
        assert plan(lib, kind, sr=32000, hi=15000.0, count=2, r=10)[1].sliceInLds == 1


@pytest.mark.parametrize("kind", [hc.HPS, hc.LHS], ids=["HPS", "LHS"])
def test_refusals(kind, lib):
    for r in (5, 14, 0, 31):
        st, obj = hc.new(hc.bind(lib), kind, r=r)
        assert st == -100 and not obj
    st, obj = hc.new(lib, kind, sr=2000, hi=900.0, r=12, count=1)  # fftLength 4096 above M = 2048
    assert st == -6 and not obj
    st, obj = hc.new(lib, kind, sr=44100, hi=8000.0, r=10, count=5)  # bin 40000 of a 32768-point spectrum
    assert st == -6 and not obj and "beyond" in af.last_error()
    assert plan(lib, kind, r=14)[0] == -100


@pytest.mark.parametrize("kind", [hc.HPS, hc.LHS], ids=["HPS", "LHS"])
def test_cal_time_length_equals_the_reference(kind, lib, rlib):
    """non-continuing objects need no device; the continuing rule is afx_frametail's, exercised in tests/test_pitch_cpu.py
    and, with the object, in tests/test_pitch_hs_hoststub.py"""
    if af.runtime_status() != 0:
        # without a device no object exists: the rule is the shared afx_frames / afx_frametail_frames
        lib.afx_test_frametail.restype = C.c_int
        for r, hop in ((8, 64), (8, 300), (10, 333)):
            N = 1 << r
            rst, robj = hc.new(rlib, kind, 16000, 60.0, 2000.0, r, hop, 2, 3, 1)
            x = np.zeros(5 * N + 7 * hop, np.float32)
            lens = np.array([N // 3, N, 1, 2 * N + hop + 5, 17], np.int32)
            frames, tails, cur = (np.zeros(len(lens), np.int32) for _ in range(3))
            sums = np.zeros(len(lens), np.float64)
            assert lib.afx_test_frametail(N, hop, 1, x.ctypes.data_as(hc.fp), lens.ctypes.data_as(hc.ip), len(lens),
                                          frames.ctypes.data_as(hc.ip), tails.ctypes.data_as(hc.ip), cur.ctypes.data_as(hc.ip),
                                          sums.ctypes.data_as(C.POINTER(C.c_double))) == 0
            at = 0
            for i, n in enumerate(lens):
                assert hc.cal_time_length(rlib, kind, robj, int(n)) == frames[i], (r, hop, i)
                hc.call(rlib, kind, robj, x[at:at + n])
                at += n
            hc.free(rlib, kind, robj)
        return
    hc.bind(lib)
    for cont in (0, 1):
        for r, hop in ((8, 64), (8, 300), (10, 333)):
            N = 1 << r
            st, obj = hc.new(lib, kind, 16000, 60.0, 2000.0, r, hop, 2, 3, cont)
            rst, robj = hc.new(rlib, kind, 16000, 60.0, 2000.0, r, hop, 2, 3, cont)
            assert st == 0 and rst == 0
            x = np.zeros(5 * N + 7 * hop, np.float32)
            at = 0
            for n in (N // 3, N, 1, 2 * N + hop + 5, 17):
                assert hc.cal_time_length(lib, kind, obj, n) == hc.cal_time_length(rlib, kind, robj, n), (cont, r, hop, n)
                hc.call(lib, kind, obj, x[at:at + n])
                hc.call(rlib, kind, robj, x[at:at + n])
                at += n
            hc.free(lib, kind, obj)
            hc.free(rlib, kind, robj)


@pytest.mark.parametrize("name,kind", hc.pairs(), ids=[f"{n}-{hc.KIND_NAME[k]}" for n, k in hc.pairs()])
def test_restatement_against_the_compiled_reference(name, kind, rlib):
    """the reference's decisions and its own curve rows under the acceptance rule, and equal to what the fixture stores"""
    from tests.golden.make_pitch_hs_golden import reference_case
    gold = np.load(os.path.join(hc.GOLDEN, "pitch_hs.npz"))
    sr = hc.CASES[name][1]
    fre, eps, frames = reference_case(rlib, name, kind)
    M = hc.round_pow2(sr)
    fre64 = np.array([hr.fre_of(f["index"], sr, M) for f in frames], np.float32)
    check_case(name, frames, eps, fre64, fre, sr, M)
    key = f"{name}/{hc.KIND_NAME[kind]}"
    assert np.array_equal(gold[key + "/fre"].view(np.uint32), fre.view(np.uint32)) and np.array_equal(gold[key + "/eps"], eps)


def test_fixture_self_check():
    """every case and kind is there with 3 ... 12 frames; fre is (index + 1) * samplate / M of a candidate; silent frames
    hold minIndex; the stored curves are the restatement's; the file stays small"""
    path = os.path.join(hc.GOLDEN, "pitch_hs.npz")
    gold = np.load(path)
    assert os.path.getsize(path) < 600 * 1024 < os.path.getsize(os.path.join(hc.GOLDEN, "nsgt.npz"))
    for name, kind in hc.pairs():
        _, sr, lo, hi, r, hop, window, count, sig, n = hc.CASES[name]
        key = f"{name}/{hc.KIND_NAME[kind]}"
        M, mn, mx, cnt, wt = hc.plan(kind, sr, lo, hi, r, hop, window, count)
        fre, eps = gold[key + "/fre"], gold[key + "/eps"]
        T = hc.frames(n, r, hop)
        assert 3 <= T <= 12 and len(fre) == len(eps) == T and (eps >= 1e-5).all(), key
        idx = np.rint(fre.astype(np.float64) / (sr / M)).astype(int) - 1
        assert ((idx >= mn) & (idx <= mx)).all(), key
        assert np.array_equal(fre, np.array([hr.fre_of(i, sr, M) for i in idx], np.float32)), key
        if sig == "zero":
            assert (idx == mn).all()
        if name in hc.CURVES:
            frames = hr.pitch(kind, hc.case_input(name), sr, r, hop, wt, M, mn, mx, cnt)
            c64 = gold[key + "/curve64"]
            assert c64.shape == (T, mx + 1)
            for t, f in enumerate(frames):
                assert np.array_equal(c64[t], f["curve"].astype(np.float32)), (key, t)
    # the D classes, both sides of M against the samplate, and both slice placements are all present
    ds = {hc.round_pow2(c[1]) >> c[4] for c in hc.CASES.values()}
    assert {1, 2, 8, 16, 128} <= ds
    assert any(hc.round_pow2(c[1]) < c[1] for c in hc.CASES.values()) and any(hc.round_pow2(c[1]) > c[1] for c in hc.CASES.values())
