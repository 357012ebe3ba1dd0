"""Drop-in boundary of the PEF pitch tracker: the reference's OWN unmodified `audioflux.PitchPEF` wrapper, staged as
tests/dropin/test_dropin.py stages it, runs its docstring flow once on the stock library and once on
libaudioflux_mi355x.so, in fresh interpreters (tests/dropin/flows_pitch_pef.py): the frame count is identical, the
frequencies meet the rule of tests/pitch_pef_check.py, and set_filter_params changes nothing on either.  CPU part: the
wrapper resolves every pitchPEFObj_* symbol it looks up from the product library."""
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
    out = os.path.join(tmp, f"pitch_pef_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_pitch_pef.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_pitch_pef.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_pitch_pef_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {f"pitchPEFObj_{n}" for n in ("new", "calTimeLength", "setFilterParams", "pitch", "free")}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrapper looks up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_pitch_pef"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
def test_docstring_flow_matches_stock(both):
    import audioflux_amd
    from tests import pitch_pef_cases as pc
    from tests import pitch_pef_restate as pr
    from tests.pitch_pef_check import check_case
    from flows_pitch_pef import CASE
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    c = pc.CASES[CASE]
    st, tables = pc.plan(pc.bind_plan(audioflux_amd.get_lib()), *pc.ctor_args(CASE))
    assert st == 0
    tables["lin"] = pc.lin_table(c[0], 1 << c[4])
    mn, mx, pad = tables["minIndex"], tables["maxIndex"], tables["filterPadNum"]
    assert int(got["frames"]) == int(want["frames"]) == len(want["fre"])
    assert got["fre"].dtype == want["fre"].dtype and got["fre2"].shape == want["fre2"].shape
    eps = np.load(os.path.join(pc.GOLDEN, "pitch_pef.npz"))[f"{CASE}/eps"]
    x = pc.case_input(CASE)
    frames = pr.pitch(x, tables, c[4], c[5], pad, mn, mx)
    check_case("dropin", frames, eps, want["fre"], got["fre"], tables["lg"], mn)
    check_case("dropin channel 0", frames, eps, want["fre2"][0], got["fre2"][0], tables["lg"], mn)
    rev = pr.pitch(x[::-1].copy(), tables, c[4], c[5], pad, mn, mx)
    check_case("dropin channel 1", rev, np.full(len(rev), 1e-5), want["fre2"][1], got["fre2"][1], tables["lg"], mn)
    for d in (want, got):  # set_filter_params: no change, on either library
        assert np.array_equal(d["fre_after_set"].view(np.uint32), d["fre"].view(np.uint32))
