"""CPU-only checks of the PEF pitch tracker: the exports and their prototypes against the reference header, the wrapper's
signature and ValueErrors, afx_pitch_pef_plan_host against the compiled reference's constructor over a parameter grid (every
fallback and reset: minIndex / maxIndex / filterPadNum equal, the four tables bit-equal; against the fixture's stored tables
where oracle/_ref is absent), the refusals, calTimeLength of continuing and non-continuing objects, the float64 restatement
against the compiled reference on every case, and the fixture."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import pitch_pef_cases as pc
from tests import pitch_pef_restate as pr
from tests.pitch_pef_check import check_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("new", "calTimeLength", "setFilterParams", "pitch", "enableDebug", "free")
EXTRA = ("pitchBatchDevice", "curveBatchDevice", "minIndex", "maxIndex", "filterPadNum", "logLength")
TABLES = ("lg", "bw", "h", "window")


@pytest.fixture(scope="module")
def lib():
    lib = af.get_lib()
    assert hasattr(lib, "pitchPEFObj_new") and hasattr(lib, "afx_pitch_pef_plan_host")
    return pc.bind_device(lib)


@pytest.fixture(scope="module")
def rlib():
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    return pc.bind(ref.lib())


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(pc.GOLDEN, "pitch_pef.npz"))


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
    for n in ENTRY + EXTRA:
        assert hasattr(lib, f"pitchPEFObj_{n}"), n
    ours = _protos(open(os.path.join(ROOT, "include", "mir", "_pitch_pef.h")).read(), "pitchPEFObj")
    assert set(ours) == {f"pitchPEFObj_{n}" for n in ENTRY + EXTRA}
    path = os.path.join(os.path.dirname(ROOT), "reference", "src", "mir", "_pitch_pef.h")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    theirs = _protos(open(path).read(), "pitchPEFObj")
    assert set(theirs) == {f"pitchPEFObj_{n}" for n in ENTRY}
    assert {n: ours[n] for n in theirs} == theirs


def test_wrapper_signature_and_value_errors():
    sig = inspect.signature(af.PitchPEF.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("samplate", 32000), ("low_fre", 32.0), ("high_fre", 2000.0), ("cut_fre", 4000.0), ("radix2_exp", 12), ("slide_length", 1024),
        ("window_type", af.WindowType.HAMM), ("alpha", 10.0), ("beta", 0.5), ("gamma", 1.8)]
    assert "PitchPEF" in af.__all__
    for m in ("cal_time_length", "set_filter_params", "pitch", "pitch_batch_device", "curve_batch_device"):
        assert callable(getattr(af.PitchPEF, m))
    for kw in ({"low_fre": 2000.0}, {"cut_fre": 2000.0}, {"alpha": 0.0}, {"beta": -0.1}, {"beta": 1.5}, {"gamma": 1.0}):
        with pytest.raises(ValueError):  # raised before any library call, as in python/audioflux/mir/pitch_pef.py:85-94
            af.PitchPEF(**kw)


def _refused(f, N):
    """where the reference itself reads out of bounds (include/mir/_pitch_pef.h, the deviations)"""
    return f["minIndex"] < 0 or f["maxIndex"] <= f["minIndex"] or min(f["maxIndex"] + 1, 2 * N + f["filterPadNum"] - 1) != f["maxIndex"] + 1


BAND = list(itertools.product((None, 8000, 44100, 22051, 0, 200000),           # samplate: default, values, odd, out of range
                              (None, 20.0, 100.5),                             # lowFre: below 27 is ignored
                              (None, 90.0, 101.0, 1500.7, 3999.0, 4000.0, 30000.0),  # highFre: inside, at samplate / 2, beyond
                              (None, 1000.0, 3000.0, 30000.0)))                # cutFre: below highFre, between, above samplate / 2
FILTER = list(itertools.product(((None, None, None), (0.0, -1.0, 1.0), (0.3, 0.5, 1.3), (10.0, 1.0, 1.8), (4.0, 0.05, 3.0)),
                                (None, 0, 5, 9),                               # windowType: any is taken
                                ((6, None), (9, 133), (12, None))))


def _compare(lib, rlib, args, seen):
    st, p = pc.plan(lib, *args)
    rst, robj = pc.new(rlib, *args)
    assert rst == 0
    f, t = pc.ref_fields(robj), pc.ref_tables(robj)
    rlib.pitchPEFObj_free(robj)
    assert st in (0, -6), args
    seen[st] += 1
    assert (p["fftLength"], p["slideLength"], p["minIndex"], p["maxIndex"], p["filterPadNum"], p["refXcorrLength"]) == \
        (f["fftLength"], f["slideLength"], f["minIndex"], f["maxIndex"], f["filterPadNum"], f["xcorrFFTLength"]), args
    assert p["logLength"] == 2 * p["fftLength"] and p["corrLength"] == 4 * p["fftLength"]
    for k in TABLES:
        assert same_bits(p[k], t[k]), (args, k)
    assert same_bits(pc.lin_table(p["samplate"], p["fftLength"]), t["lin"]), args
    assert (st == -6) == _refused(f, f["fftLength"]), (args, f)


def test_plan_equals_the_reference_constructor(lib, rlib):
    """every field the reference's constructor decides and every table it builds, read from the object it built; the plans
    this library refuses (-6) are exactly those where the reference would read out of bounds"""
    seen = {0: 0, -6: 0}
    for sr, lo, hi, cut in BAND:
        for r, hop in ((10, None), (7, 300)):
            _compare(lib, rlib, (sr, lo, hi, cut, r, hop, None, None, None, None), seen)
    for (alpha, beta, gamma), window, (r, hop) in FILTER:
        _compare(lib, rlib, (None, None, None, None, r, hop, window, alpha, beta, gamma), seen)
    assert seen[0] > 400 and seen[-6] > 50, seen


def test_plan_tables_equal_the_fixture(lib, gold):
    """without the compiled reference: the tables it built for the fixture's small cases, as stored"""
    for name in pc.CURVES:
        st, p = pc.plan(lib, *pc.ctor_args(name))
        assert st == 0
        assert [p["minIndex"], p["maxIndex"], p["filterPadNum"]] == gold[name + "/plan"].tolist(), name
        for k in TABLES:
            assert same_bits(p[k], gold[f"{name}/{k}"]), (name, k)
    for name in pc.CASES:
        st, p = pc.plan(lib, *pc.ctor_args(name))
        assert st == 0 and [p["minIndex"], p["maxIndex"], p["filterPadNum"]] == gold[name + "/plan"].tolist(), name


def test_defaults_fallbacks_and_the_lds_budget(lib):
    st, p = pc.plan(lib)
    assert (st, p["samplate"], p["lowFre"], p["highFre"], p["cutFre"], p["radix2Exp"], p["slideLength"], p["windowType"], p["isContinue"]) == \
        (0, 32000, 32.0, 2000.0, 4000.0, 12, 1024, 2, 0)
    assert (np.float32(p["alpha"]), np.float32(p["beta"]), np.float32(p["gamma"])) == (np.float32(10), np.float32(0.5), np.float32(1.8))
    assert (p["minIndex"], p["maxIndex"], p["filterPadNum"], p["logLength"], p["refXcorrLength"], p["corrLength"]) == \
        (1590, 7243, 933, 8192, 32768, 16384)
    # the log grid ends at cutFre 4000 of 16000 Hz: bins 0 ... 1025 of the 4097 are read; two workgroups fit a CU's 160 KB
    assert p["pwLength"] == 1026 and p["ldsBytes"] == 128 + 8 * (8192 + 256 + 1) + 4 * 1028 <= 80 * 1024
    # cutFre above samplate / 2: the grid ends one hertz below it, every bin is read
    q = pc.plan(lib, sr=8000, cut=30000.0, r=8)[1]
    assert q["pwLength"] == 257 and q["ldsBytes"] == 128 + 8 * (512 + 16 + 1) + 4 * 260
    # a highFre outside (lowFre, samplate / 2) resets both; samplate / 2 is an integer division
    assert [pc.plan(lib, sr=8001, lo=100.0, hi=4000.0, r=8)[1][k] for k in ("lowFre", "highFre")] == [32.0, 2000.0]
    assert [pc.plan(lib, sr=8002, lo=100.0, hi=4000.0, cut=4000.5, r=8)[1][k] for k in ("lowFre", "highFre")] == [100.0, 4000.0]
    # cutFre below highFre becomes highFre -- and the plan is then refused: maxIndex stays 0
    st, p = pc.plan(lib, cut=1000.0, r=8)
    assert (st, p["cutFre"], p["maxIndex"]) == (-6, 2000.0, 0)
    # alpha <= 0, beta <= 0, gamma <= 1 are ignored
    p = pc.plan(lib, r=8, alpha=0.0, beta=-1.0, gamma=1.0)[1]
    assert (p["alpha"], p["beta"], np.float32(p["gamma"])) == (10.0, 0.5, np.float32(1.8))
    # P = 0 with beta 1 (the reference then correlates at 4N), P = N with alpha + beta < 1
    assert [pc.plan(lib, r=9, beta=1.0)[1][k] for k in ("filterPadNum", "refXcorrLength")] == [0, 2048]
    assert [pc.plan(lib, r=8, alpha=0.3)[1][k] for k in ("filterPadNum", "refXcorrLength")] == [256, 2048]
    for r in range(6, 13):
        assert pc.plan(lib, r=r)[1]["ldsBytes"] <= 160 * 1024


def test_refusals(lib):
    for r in (5, 13, 0, 31):
        st, obj = pc.new(lib, r=r)
        assert st == -100 and not obj
        st, p = pc.plan(lib, r=r)
        assert st == -100 and p["lg"] is None
    # lowFre and highFre between the same two log frequencies (N = 64: the grid steps by 5 %): minIndex stays -1
    st, obj = pc.new(lib, sr=16000, lo=100.0, hi=100.5, r=6)
    assert st == -6 and not obj and "candidate range" in af.last_error()
    assert pc.plan(lib, sr=16000, lo=100.0, hi=100.5, r=6)[1]["minIndex"] == -1
    # highFre at the last log frequency: maxIndex stays 0
    st, obj = pc.new(lib, sr=16000, hi=2000.0, cut=2000.0, r=9)
    assert st == -6 and not obj
    with pytest.raises(RuntimeError, match="-100"):
        af.PitchPEF(radix2_exp=13, slide_length=2048)


def test_cal_time_length_equals_the_reference(lib, rlib):
    """non-continuing objects need no device; the continuing rule is afx_frametail's, exercised in tests/test_pitch_cpu.py
    and, with the object, in tests/test_pitch_pef_hoststub.py"""
    cases = ((8, 64), (8, 300), (10, 333))
    if af.runtime_status() != 0:
        # without a device no object exists: the rule is the shared afx_frames / afx_frametail_frames
        lib.afx_test_frametail.restype = C.c_int
        for r, hop in cases:
            N = 1 << r
            rst, robj = pc.new(rlib, 16000, 60.0, 2000.0, None, r, hop, cont=1)
            x = np.zeros(5 * N + 7 * hop, np.float32)
            lens = np.array([N // 3, N, 1, 2 * N + hop + 5, 17], np.int32)
            frames, tails, cur = (np.zeros(len(lens), np.int32) for _ in range(3))
            sums = np.zeros(len(lens), np.float64)
            assert lib.afx_test_frametail(N, hop, 1, x.ctypes.data_as(pc.fp), lens.ctypes.data_as(pc.ip), len(lens),
                                          frames.ctypes.data_as(pc.ip), tails.ctypes.data_as(pc.ip), cur.ctypes.data_as(pc.ip),
                                          sums.ctypes.data_as(C.POINTER(C.c_double))) == 0
            at = 0
            for i, n in enumerate(lens):
                assert rlib.pitchPEFObj_calTimeLength(robj, int(n)) == frames[i], (r, hop, i)
                pc.call(rlib, robj, x[at:at + n])
                at += n
            rlib.pitchPEFObj_free(robj)
        return
    for cont in (0, 1):
        for r, hop in cases:
            N = 1 << r
            st, obj = pc.new(lib, 16000, 60.0, 2000.0, None, r, hop, cont=cont)
            rst, robj = pc.new(rlib, 16000, 60.0, 2000.0, None, r, hop, cont=cont)
            assert st == 0 and rst == 0
            x = np.zeros(5 * N + 7 * hop, np.float32)
            at = 0
            for n in (N // 3, N, 1, 2 * N + hop + 5, 17):
                assert lib.pitchPEFObj_calTimeLength(obj, n) == rlib.pitchPEFObj_calTimeLength(robj, n), (cont, r, hop, n)
                pc.call(lib, obj, x[at:at + n])
                pc.call(rlib, robj, x[at:at + n])
                at += n
            lib.pitchPEFObj_free(obj)
            rlib.pitchPEFObj_free(robj)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_against_the_compiled_reference(name, rlib, gold):
    """the reference's decisions and its own curve rows under the acceptance rule, and equal to what the fixture stores"""
    from tests.golden.make_pitch_pef_golden import reference_case
    fre, eps, frames, f, tables = reference_case(rlib, name)
    fre64 = np.array([tables["lg"][fr["index"]] for fr in frames], np.float32)
    w = check_case(name, frames, eps, fre64, fre, tables["lg"], f["minIndex"])
    assert w["explained"] == 0, name  # the decision is well conditioned on these inputs: the reference IS the float64 argmax
    assert same_bits(gold[name + "/fre"], fre) and np.array_equal(gold[name + "/eps"], eps)
    assert gold[name + "/plan"].tolist() == [f["minIndex"], f["maxIndex"], f["filterPadNum"]]


def test_set_filter_params_of_the_reference_changes_nothing(rlib):
    """the observable behaviour include/mir/_pitch_pef.h keeps: validate, rebuild from the stored values"""
    x = pc.case_input("r8_stack")
    st, robj = pc.new(rlib, *pc.ctor_args("r8_stack"))
    before, h0 = pc.call(rlib, robj, x), pc.ref_tables(robj)["h"]
    rlib.pitchPEFObj_setFilterParams(robj, 5.0, 0.7, 2.5)
    after, h1 = pc.call(rlib, robj, x), pc.ref_tables(robj)["h"]
    rlib.pitchPEFObj_free(robj)
    assert same_bits(before, after) and same_bits(h0, h1)


def test_fixture_self_check(lib, gold):
    """every case is there with 3 ... 10 frames; fre is an entry of the case's log-frequency table inside the candidate range;
    silent frames hold lg[minIndex]; the stored curves are the restatement's; the file stays small"""
    path = os.path.join(pc.GOLDEN, "pitch_pef.npz")
    assert os.path.getsize(path) < 128 * 1024 < os.path.getsize(os.path.join(pc.GOLDEN, "pitch_hs.npz"))
    for name, c in pc.CASES.items():
        sr, r, hop, sig, n = c[0], c[4], c[5], c[10], c[11]
        st, p = pc.plan(lib, *pc.ctor_args(name))
        assert st == 0
        mn, mx, pad = (int(v) for v in gold[name + "/plan"])
        fre, eps = gold[name + "/fre"], gold[name + "/eps"]
        T = pc.frames(n, r, hop)
        assert 3 <= T <= 10 and len(fre) == len(eps) == T and (eps >= 1e-5).all(), name
        cand = set(p["lg"][mn:mx + 1].view(np.uint32).tolist())
        assert all(int(b) in cand for b in fre.view(np.uint32)), name
        if sig == "zero":
            assert (fre == p["lg"][mn]).all()
        if name in pc.CURVES:
            tables = dict(p, lin=pc.lin_table(sr, 1 << r))
            frames = pr.pitch(pc.case_input(name), tables, r, hop, pad, mn, mx)
            c64 = gold[name + "/curve64"]
            assert c64.shape == (T, mx + 1)
            for t, f in enumerate(frames):
                assert np.array_equal(c64[t], f["curve"].astype(np.float32)), (name, t)
    # the classes the issue names are all present
    rs = {c[4] for c in pc.CASES.values()}
    assert {6, 8, 9, 10, 11, 12} <= rs and sum(c[4] == 12 for c in pc.CASES.values()) == 1
    assert any(c[5] > (1 << c[4]) for c in pc.CASES.values()) and any(c[5] % 2 for c in pc.CASES.values())
    pads = {int(gold[n + "/plan"][2]) for n in pc.CASES}
    assert 0 in pads and 256 in pads
    assert {c[10].split(":")[0] for c in pc.CASES.values()} >= {"tone", "stack", "glide", "snr", "noise", "step", "zero"}
