"""CPU-only checks of the NCF and cepstrum pitch trackers: the exports and their prototypes against the reference headers,
the wrappers' signatures, afx_pitch_ncf_plan_host / afx_pitch_cep_plan_host against the compiled reference's constructors
over a parameter grid (every fallback and reset, CEP's <= Hamm rule; the window tables bit-equal; against the fixture's
stored tables where oracle/_ref is absent), the refusals, calTimeLength of continuing and non-continuing objects, the
float64 restatement against the compiled reference on every case, and the fixture."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import pitch_lag_cases as pc
from tests import pitch_lag_restate as pr
from tests.pitch_lag_check import check_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("new", "calTimeLength", "pitch", "enableDebug", "free")
EXTRA = ("pitchBatchDevice", "curveBatchDevice", "minIndex", "maxIndex")


@pytest.fixture(scope="module")
def lib():
    lib = af.get_lib()
    for k in pc.KINDS:
        assert hasattr(lib, f"pitch{k}Obj_new") and hasattr(lib, f"afx_pitch_{k.lower()}_plan_host"), k
    return pc.bind_device(lib)


@pytest.fixture(scope="module")
def rlib():
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    return pc.bind(ref.lib())


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(pc.GOLDEN, "pitch_lag.npz"))


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


@pytest.mark.parametrize("kind", pc.KINDS)
def test_exports_and_prototypes_equal_the_reference_header(kind, lib):
    prefix = f"pitch{kind}Obj"
    for n in ENTRY + EXTRA:
        assert hasattr(lib, f"{prefix}_{n}"), n
    header = f"_pitch_{kind.lower()}.h"
    ours = _protos(open(os.path.join(ROOT, "include", "mir", header)).read(), prefix)
    assert set(ours) == {f"{prefix}_{n}" for n in ENTRY + EXTRA}
    # the device prototypes live in the two headers: include/afx_batch.h has none of them
    assert "pitchNCF" not in open(os.path.join(ROOT, "include", "afx_batch.h")).read()
    assert "pitchCEP" not in open(os.path.join(ROOT, "include", "afx_batch.h")).read()
    path = os.path.join(os.path.dirname(ROOT), "reference", "src", "mir", header)
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    theirs = _protos(open(path).read(), prefix)
    assert set(theirs) == {f"{prefix}_{n}" for n in ENTRY}
    assert {n: ours[n] for n in theirs} == theirs


def test_wrapper_signatures():
    for cls, window in ((af.PitchNCF, af.WindowType.RECT), (af.PitchCEP, af.WindowType.HAMM)):
        sig = inspect.signature(cls.__init__)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
            ("samplate", 32000), ("low_fre", 32.0), ("high_fre", 2000.0), ("radix2_exp", 12), ("slide_length", 1024),
            ("window_type", window)]
        assert cls.__name__ in af.__all__
        for m in ("cal_time_length", "pitch", "pitch_batch_device", "curve_batch_device"):
            assert callable(getattr(cls, m))
    with pytest.raises(ValueError):  # raised before any library call, as in python/audioflux/mir/pitch_cep.py:72
        af.PitchCEP(low_fre=2000.0)


def _refused(kind, f):
    """where the reference itself overruns its buffers (the headers' deviations)"""
    N = f["fftLength"]
    return f["maxIndex"] > (N - 1 if kind == "NCF" else 2 * N - 1)


BAND = list(itertools.product((None, 8000, 44100, 22051, 0, 200000),  # samplate: default, values, odd, out of range
                              (None, 20.0, 100.5),                    # lowFre: below 27 is ignored
                              (None, 90.0, 1500.7, "half", "beyond")))  # highFre: inside, at samplate / 2, beyond
SIZES = ((6, None), (7, 300), (9, 133), (10, None), (12, None))
WINDOWS = (None, 0, 1, 2, 5, 9)


def _compare(lib, rlib, kind, args, seen):
    st, p = pc.plan(lib, kind, *args)
    rst, robj = pc.new(rlib, kind, *args)
    assert rst == 0
    f, w = pc.ref_fields(robj), pc.ref_window(robj)
    pc.fn(rlib, kind, "free")(robj)  # (constructed and freed only: its pitch() would overrun on the refused plans)
    assert st in (0, -6), (kind, args)
    seen[st] += 1
    assert (p["fftLength"], p["slideLength"], p["radix2Exp"], p["lagLength"], p["minIndex"], p["maxIndex"]) == \
        (f["fftLength"], f["slideLength"], f["radix2Exp"], f["lagLength"], f["minIndex"], f["maxIndex"]), (kind, args)
    assert p["lagLength"] == 2 * p["fftLength"] and p["minIndex"] >= 1
    assert same_bits(p["window"], w), (kind, args)
    assert (st == -6) == _refused(kind, f), (kind, args, f)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_plan_equals_the_reference_constructor(kind, lib, rlib):
    """every field the reference's constructor decides and the window it builds, read from the object it built; the plans this
    library refuses (-6) are exactly those where the reference would overrun"""
    seen = {0: 0, -6: 0}
    for sr, lo, hi in BAND:
        half = (sr if sr and 0 < sr <= 196000 else 32000) // 2
        hi = {"half": float(half), "beyond": half + 100.0}.get(hi, hi)
        for r, hop in SIZES:
            _compare(lib, rlib, kind, (sr, lo, hi, r, hop, None), seen)
    for window in WINDOWS:
        for r, hop in ((7, None), (10, 333)):
            _compare(lib, rlib, kind, (16000, 130.0, None, r, hop, window), seen)
    assert seen[0] > 100 and seen[-6] > 50, seen


def test_window_rule(lib):
    """NCF takes any type; CEP keeps Hamm for anything above it"""
    for window in WINDOWS:
        assert pc.plan(lib, "NCF", r=8, window=window)[1]["windowType"] == (0 if window is None else window)
        assert pc.plan(lib, "CEP", r=8, window=window)[1]["windowType"] == (window if window in (0, 1, 2) else 2)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_plan_equals_the_fixture(kind, lib, gold):
    """without the compiled reference: what it decided for the fixture's cases, the windows of the small ones, as stored"""
    for name in pc.CASES:
        st, p = pc.plan(lib, kind, *pc.ctor_args(name))
        assert st == 0 and [p["minIndex"], p["maxIndex"]] == gold[f"{kind}/{name}/plan"].tolist(), (kind, name)
        assert p["windowType"] == pc.window_of(kind, name)
        if name in pc.CURVES:
            assert same_bits(p["window"], gold[f"{kind}/{name}/window"]), (kind, name)


def test_defaults_fallbacks_and_the_lds_budget(lib):
    for kind, window in (("NCF", 0), ("CEP", 2)):
        st, p = pc.plan(lib, kind)
        assert (st, p["samplate"], p["lowFre"], p["highFre"], p["radix2Exp"], p["fftLength"], p["slideLength"], p["windowType"],
                p["isContinue"], p["minIndex"], p["maxIndex"], p["lagLength"]) == (0, 32000, 32.0, 2000.0, 12, 4096, 1024, window, 0, 16, 1000, 8192)
        # the 8192-point complex buffer with its padding: two workgroups share a CU's 160 KB
        assert p["ldsBytes"] == 256 + 8 * (8192 + 256 + 1) <= 80 * 1024
        for r in range(6, 13):
            assert pc.plan(lib, kind, sr=44100, r=r, lo=700.0)[1]["ldsBytes"] == 256 + 8 * ((2 << r) + (2 << r >> 5) + 1)
        # a highFre outside (lowFre, samplate / 2) resets both; samplate / 2 is an integer division
        assert [pc.plan(lib, kind, sr=8001, lo=100.0, hi=4000.0, r=8)[1][k] for k in ("lowFre", "highFre")] == [32.0, 2000.0]
        assert [pc.plan(lib, kind, sr=8002, lo=100.0, hi=4000.0, r=8)[1][k] for k in ("lowFre", "highFre")] == [100.0, 4000.0]
        # lowFre below 27 is ignored; a non-positive hop is N / 4; the indices are rounded in float32
        p = pc.plan(lib, kind, sr=22051, lo=20.0, hi=1500.7, r=9, hop=0)[1]
        assert (p["lowFre"], p["slideLength"], p["minIndex"], p["maxIndex"]) == (32.0, 128, 15, 689)
        assert pc.plan(lib, kind, hop=5000)[1]["slideLength"] == 5000
        assert pc.plan(lib, kind, cont=1)[1]["isContinue"] == 1


def test_refusals(lib):
    for kind in pc.KINDS:
        for r in (5, 13, 0, 31):
            st, obj = pc.new(lib, kind, r=r)
            assert st == -100 and not obj
            st, p = pc.plan(lib, kind, r=r)
            assert st == -100 and p["window"] is None
    # NCF: maxIndex = 250 of N = 64 -- the reference's rearrangement writes 501 floats into 128
    st, obj = pc.new(lib, "NCF", sr=8000, lo=32.0, r=6)
    assert st == -6 and not obj and "maxIndex 250" in af.last_error()
    st, p = pc.plan(lib, "NCF", sr=8000, lo=32.0, r=6)
    assert st == -6 and p["maxIndex"] == 250 and p["window"] is not None
    assert pc.plan(lib, "NCF", sr=8000, lo=127.0, r=6)[0] == 0   # maxIndex 63 = N - 1
    assert pc.plan(lib, "NCF", sr=8000, lo=125.0, r=6)[0] == -6  # maxIndex 64
    # CEP: its row has 2N entries
    assert pc.plan(lib, "CEP", sr=8000, lo=63.0, r=6)[0:1] == (0,) and pc.plan(lib, "CEP", sr=8000, lo=63.0, r=6)[1]["maxIndex"] == 127
    st, obj = pc.new(lib, "CEP", sr=8000, lo=62.0, r=6)
    assert st == -6 and not obj and "maxIndex 129" in af.last_error()
    with pytest.raises(RuntimeError, match="-100"):
        af.PitchNCF(radix2_exp=13, slide_length=2048)
    with pytest.raises(RuntimeError, match="-100"):
        af.PitchCEP(radix2_exp=5, slide_length=8)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_cal_time_length_equals_the_reference(kind, lib, rlib):
    """non-continuing objects need no device; the continuing rule is afx_frametail's, exercised in tests/test_pitch_cpu.py
    and, with the object, in tests/test_pitch_lag_hoststub.py"""
    cases = ((8, 64), (8, 300), (10, 333))
    ctl = pc.fn(rlib, kind, "calTimeLength")
    if af.runtime_status() != 0:
        # without a device no object exists: the rule is the shared afx_frames / afx_frametail_frames
        lib.afx_test_frametail.restype = C.c_int
        for cont in (0, 1):
            for r, hop in cases:
                N = 1 << r
                rst, robj = pc.new(rlib, kind, 16000, 80.0, 2000.0, r, hop, cont=cont)
                assert rst == 0
                x = np.zeros(5 * N + 7 * hop, np.float32)
                lens = np.array([N // 3, N, 1, 2 * N + hop + 5, 17], np.int32)
                frames, tails, cur = (np.zeros(len(lens), np.int32) for _ in range(3))
                sums = np.zeros(len(lens), np.float64)
                assert lib.afx_test_frametail(N, hop, cont, x.ctypes.data_as(pc.fp), lens.ctypes.data_as(pc.ip), len(lens),
                                              frames.ctypes.data_as(pc.ip), tails.ctypes.data_as(pc.ip), cur.ctypes.data_as(pc.ip),
                                              sums.ctypes.data_as(C.POINTER(C.c_double))) == 0
                at = 0
                for i, n in enumerate(lens):
                    assert ctl(robj, int(n)) == frames[i], (kind, cont, r, hop, i)
                    pc.call(rlib, kind, robj, x[at:at + n])
                    at += n
                pc.fn(rlib, kind, "free")(robj)
        return
    for cont in (0, 1):
        for r, hop in cases:
            N = 1 << r
            st, obj = pc.new(lib, kind, 16000, 80.0, 2000.0, r, hop, cont=cont)
            rst, robj = pc.new(rlib, kind, 16000, 80.0, 2000.0, r, hop, cont=cont)
            assert st == 0 and rst == 0
            x = np.zeros(5 * N + 7 * hop, np.float32)
            at = 0
            for n in (N // 3, N, 1, 2 * N + hop + 5, 17):
                assert pc.fn(lib, kind, "calTimeLength")(obj, n) == ctl(robj, n), (kind, cont, r, hop, n)
                pc.call(lib, kind, obj, x[at:at + n])
                pc.call(rlib, kind, robj, x[at:at + n])
                at += n
            pc.fn(lib, kind, "free")(obj)
            pc.fn(rlib, kind, "free")(robj)


@pytest.mark.parametrize("name", list(pc.CASES))
@pytest.mark.parametrize("kind", pc.KINDS)
def test_restatement_against_the_compiled_reference(kind, name, rlib, gold):
    """the reference's decisions and its own curve rows under the acceptance rule, and equal to what the fixture stores"""
    from tests.golden.make_pitch_lag_golden import reference_case
    fre, eps, frames, f, window = reference_case(rlib, kind, name)
    sr = pc.CASES[name][0]
    fre64 = pr.fre_of([fr["index"] for fr in frames], sr)
    w = check_case(f"{kind}/{name}", frames, eps, fre64, fre, sr)
    assert w["explained"] == 0, name  # the decision is well conditioned on these inputs: the reference IS the float64 argmax
    assert same_bits(fre64, fre)
    key = f"{kind}/{name}"
    assert same_bits(gold[key + "/fre"], fre) and np.array_equal(gold[key + "/eps"], eps)
    assert gold[key + "/plan"].tolist() == [f["minIndex"], f["maxIndex"]]


def test_fixture_self_check(lib, gold):
    """every case is there for both trackers with 3 ... 10 frames; fre is samplate / (index + 1) of a candidate; silent frames
    hold samplate / (minIndex + 1); the stored curves are the restatement's; the file stays small"""
    path = os.path.join(pc.GOLDEN, "pitch_lag.npz")
    assert os.path.getsize(path) < 128 * 1024
    for kind in pc.KINDS:
        for name, c in pc.CASES.items():
            sr, r, hop, sig, T = c[0], c[3], c[4], c[6], c[7]
            key = f"{kind}/{name}"
            st, p = pc.plan(lib, kind, *pc.ctor_args(name))
            assert st == 0
            mn, mx = (int(v) for v in gold[key + "/plan"])
            assert mx <= (1 << r) - 1, name  # every row runs on both trackers
            fre, eps = gold[key + "/fre"], gold[key + "/eps"]
            assert pc.frames(pc.data_length(name), r, hop) == T and 3 <= T <= 10
            assert len(fre) == len(eps) == T and (eps >= 1e-5).all(), key
            cand = set(pr.fre_of(np.arange(mn, mx + 1), sr).view(np.uint32).tolist())
            assert all(int(b) in cand for b in fre.view(np.uint32)), key
            if sig == "zero":
                assert (fre == pr.fre_of(mn, sr)).all()
            if name in pc.CURVES:
                frames = pr.pitch(kind, pc.case_input(name), pc.restate_window(p), r, hop, mn, mx)
                c64 = gold[key + "/curve64"]
                assert c64.shape == (T, mx + 1)
                for t, f in enumerate(frames):
                    assert np.array_equal(c64[t], f["curve"].astype(np.float32), equal_nan=True), (key, t)
    # the classes the cases are there for
    rs = [c[3] for c in pc.CASES.values()]
    assert {6, 8, 9, 10, 11, 12} <= set(rs) and rs.count(12) == 1 and len(pc.CASES) == 12
    assert any(c[4] > (1 << c[3]) for c in pc.CASES.values()) and any(c[4] % 2 for c in pc.CASES.values())
    assert {c[5] for c in pc.CASES.values()} == {None, pc.RECT, pc.HANN, pc.HAMM}
    assert {c[6].split(":")[0] for c in pc.CASES.values()} >= {"tone", "stack", "glide", "snr", "noise", "step", "zero", "tiny"}
