"""Drop-in boundary of the HPS / LHS pitch trackers: the reference's OWN unmodified `audioflux.PitchHPS` / `audioflux.PitchLHS`
wrappers, staged as tests/dropin/test_dropin.py stages them, run their docstring flow once on the stock library and once
on libaudioflux_mi355x.so, in fresh interpreters (tests/dropin/flows_pitch_hs.py): the frame count is identical and the
frequencies meet the rule of tests/pitch_hs_check.py.  CPU part: the wrappers resolve every pitchHPSObj_* / pitchLHSObj_*
symbol they look up from the product library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402

needs_inputs = pytest.mark.skipif(
    not (os.path.exists(flows.STOCK) and os.path.exists(flows.PRODUCT) and os.path.exists(flows.WRAPPER_ZIP)),
    reason="needs the compiled reference with its wrapper archive and the built product library")


def _run(tmp, mode):
    out = os.path.join(tmp, f"pitch_hs_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_pitch_hs.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_pitch_hs.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrappers_resolve_every_pitch_hs_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {f"pitch{k}Obj_{n}" for k in ("HPS", "LHS") for n in ("new", "calTimeLength", "pitch", "free")}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrappers look up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_pitch_hs"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("kind", [0, 1], ids=["HPS", "LHS"])
def test_docstring_flow_matches_stock(both, kind):
    from tests import pitch_hs_cases as hc
    from tests import pitch_hs_restate as hr
    from tests.pitch_hs_check import check_case
    from flows_pitch_hs import CASE
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    k = hc.KIND_NAME[kind]
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[CASE]
    M, mn, mx, cnt, wt = hc.plan(kind, sr, lo, hi, r, hop, window, count)
    assert int(got[f"{k}/frames"]) == int(want[f"{k}/frames"]) == len(want[f"{k}/fre"])
    assert got[f"{k}/fre"].dtype == want[f"{k}/fre"].dtype and got[f"{k}/fre2"].shape == want[f"{k}/fre2"].shape
    eps = np.load(os.path.join(hc.GOLDEN, "pitch_hs.npz"))[f"{CASE}/{k}/eps"]
    x = hc.case_input(CASE)
    frames = hr.pitch(kind, x, sr, r, hop, wt, M, mn, mx, cnt)
    check_case(f"dropin {k}", frames, eps, want[f"{k}/fre"], got[f"{k}/fre"], sr, M)
    check_case(f"dropin {k} channel 0", frames, eps, want[f"{k}/fre2"][0], got[f"{k}/fre2"][0], sr, M)
    rev = hr.pitch(kind, x[::-1].copy(), sr, r, hop, wt, M, mn, mx, cnt)
    check_case(f"dropin {k} channel 1", rev, np.full(len(rev), 1e-5), want[f"{k}/fre2"][1], got[f"{k}/fre2"][1], sr, M)
