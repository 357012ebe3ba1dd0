"""CPU-only: what the onset feature decides without a device.  The pick parameters of afx_onset_plan_host against the grid the
fixture recorded from the compiled reference's onsetObj_debug (pairs where a product lands on an integer included); the
restatement of tests/onset_restate.py -- filter, novelty, normalisation in float64, the pick rule in float64 and float32 --
against the compiled reference when oracle/_ref exists and against the fixture otherwise; the refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import onset_cases as oc
from tests import onset_restate as rs
from tests.onset_check import FLOOR, marginal_frames, reference_eps


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "onset.npz"))


@pytest.fixture(scope="module")
def lib():
    return oc.bind_device(af.get_lib())


def test_plan_matches_the_recorded_grid(lib, gold):
    pairs, params, delta = gold["grid/pairs"], gold["grid/params"], gold["grid/delta"]
    assert len(pairs) == len(oc.GRID) >= 30 and np.array_equal(pairs, np.array(oc.GRID, np.int32))
    on_integer = 0
    for (sr, hop), want, d in zip(pairs.tolist(), params.tolist(), delta):
        got, gd = oc.plan(lib, sr, hop)
        assert got == want and np.float32(gd) == d == np.float32(0.07), (sr, hop, got, want)
        assert rs.pick_params(sr, hop)[0] == want, (sr, hop)
        s, h = (sr if sr > 0 else 32000), (hop if hop >= 1 else 512)
        on_integer += any(abs(v - round(v)) < 1e-9 and round(v) > 0 for v in (0.03 * s / h, 0.1 * s / h))
    assert on_integer >= 8, on_integer  # products that land on (or a rounding away from) an integer decide a parameter
    assert lib.afx_onset_plan_host(32000, 512, None, None) == -6
    out = (C.c_int * 5)()
    assert lib.afx_onset_plan_host(44100, 441, out, None) == 0 and list(out) == [3, 1, 10, 11, 3]


def test_plan_matches_the_live_reference():
    if not ref.available():
        pytest.skip("needs oracle/_ref (make -C oracle); the recorded grid covers it otherwise")
    grid = [(sr, hop) for sr in (8000, 22050, 32000, 44100, 48000) for hop in (64, 100, 147, 160, 441, 480, 512, 1000)]
    params, delta = oc.debug_params(ref.REF_PATH, grid)
    lib = oc.bind_device(af.get_lib())
    for (sr, hop), want in zip(grid, params.tolist()):
        assert oc.plan(lib, sr, hop)[0] == want, (sr, hop)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_restatement_against_the_reference(name, gold):
    """the float64 envelope within the yardstick of the reference's, the float64 and float32 pick rules reproduce its points,
    no marginal decision: what the generator demanded of the fixture, re-checked (live when oracle/_ref exists)"""
    c = oc.CASES[name]
    spec, phase = oc.case_input(name)
    evn, pts = gold[name + "/evn"], gold[name + "/points"]
    if ref.available():
        live_evn, live_pts = oc.run_case(oc.bind(ref.lib()), name, spec, phase)
        assert np.array_equal(live_evn.view(np.uint32), evn.view(np.uint32)) and np.array_equal(live_pts, pts), name
    pick, delta = rs.pick_params(c["sr"], c["hop"])
    assert pick == gold[name + "/pick"].tolist()
    e64 = rs.envelope64(spec, phase, c["kind"], c["order"], c["param"], c["index"])
    eps = reference_eps(e64, evn)
    assert eps == float(gold[name + "/eps"][0]) and eps <= 4e-5, (name, eps)
    assert np.array_equal(rs.pick(e64, pick, delta, np.float64), pts), name
    assert np.array_equal(rs.pick(evn, pick, delta, np.float32), pts), name  # the float32 rule on the reference's own envelope
    assert len(marginal_frames(e64, pick, delta, eps)) == 0, name
    assert len(pts) >= 3 and evn.min() == 0 and evn.max() == 1


def test_max_filter_restatement_against_the_reference():
    if not ref.available():
        pytest.skip("needs oracle/_ref (make -C oracle); the fixture cases with order >= 2 cover it otherwise")
    L = ref.lib()
    L.__mmaxfilter.restype = None
    L.__mmaxfilter.argtypes = [oc.fp, C.c_int, C.c_int, C.c_int, C.c_int, oc.fp]
    rng = np.random.default_rng(1)
    for rows, cols in ((3, 1), (4, 5), (2, 33)):
        x = rng.standard_normal((rows, cols)).astype(np.float32)
        for order in (1, 2, 3, 4, 5, cols, cols + 4):
            y = np.zeros_like(x)
            L.__mmaxfilter(x.ctypes.data_as(oc.fp), rows, cols, 1, order, y.ctypes.data_as(oc.fp))
            assert np.array_equal(y, rs.max_filter(x, order)), (rows, cols, order)


def test_wait_rule_suppresses_a_candidate(gold):
    """flux_o5_p3 (44100 / 441: wait = 3) holds a candidate that only the wait rule rejects"""
    evn = gold["flux_o5_p3/evn"]
    pick = gold["flux_o5_p3/pick"].tolist()
    with_wait = rs.pick(evn, pick, 0.07, np.float32)
    without = rs.pick(evn, pick[:4] + [0], 0.07, np.float32)
    assert np.array_equal(with_wait, gold["flux_o5_p3/points"]) and len(without) > len(with_wait)


def test_no_device_no_object(lib):
    if af.runtime_status() == 0:
        pytest.skip("a device is present; covered by the gpu tests")
    st, obj = oc.new(lib, 10, 4, 512)
    assert st == -2 and not obj
    assert oc.new(lib, 0, 4, 512)[0] == -6 and oc.new(lib, 10, 0, 512)[0] == -6  # refused before the device is asked for
    lib.afx_error_count.restype = C.c_int
    before = lib.afx_error_count()
    p = np.ones(4, np.float32)
    lib.util_powerToDB(p.ctypes.data_as(oc.fp), 4, -80.0, None)  # a void call: the failure is counted, the wrapper raises
    assert lib.afx_error_count() > before and (p == 1).all()
    with pytest.raises(RuntimeError, match="util_powerToDB failed"):
        af.power_to_db(np.ones((2, 2), np.float32))
    with pytest.raises(RuntimeError, match="status -2"):
        af.Onset(10, 4, 512)
    assert FLOOR == 1e-5


def test_abi_values():
    assert [int(v) for v in af.NoveltyType] == list(range(11)) and af.NoveltyType.BROADBAND == 10
    assert C.sizeof(af.NoveltyParam) == 32 and [f[0] for f in af.NoveltyParam._fields_] == [
        "step", "p", "isPostive", "isExp", "type", "threshold", "isNorm", "gamma"]
    hdr = open(os.path.join(os.path.dirname(oc.GOLDEN), "..", "include", "mir", "onset_algorithm.h")).read()
    assert "Novelty_Flux = 0" in hdr and hdr.index("Novelty_RCD") < hdr.index("Novelty_Broadband")
