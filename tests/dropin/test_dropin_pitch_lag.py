"""Drop-in boundary of the NCF and cepstrum pitch trackers: the reference's OWN unmodified `audioflux.PitchNCF` /
`audioflux.PitchCEP` wrappers, staged as tests/dropin/test_dropin.py stages them, run their docstring flow once on the stock
library and once on libaudioflux_mi355x.so, in fresh interpreters (tests/dropin/flows_pitch_lag.py): the frame count is
identical and the frequencies meet the rule of tests/pitch_lag_check.py.  CPU part: the wrappers resolve every
pitchNCFObj_* / pitchCEPObj_* symbol they look up from the product library."""
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
    out = os.path.join(tmp, f"pitch_lag_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_pitch_lag.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_pitch_lag.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrappers_resolve_every_pitch_lag_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {f"pitch{k}Obj_{n}" for k in ("NCF", "CEP") for n in ("new", "calTimeLength", "pitch", "free")}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrappers look up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_pitch_lag"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("kind", ["NCF", "CEP"])
def test_docstring_flow_matches_stock(kind, both):
    import audioflux_amd
    from tests import pitch_lag_cases as pc
    from tests import pitch_lag_restate as pr
    from tests.pitch_lag_check import check_case
    from flows_pitch_lag import CASE
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    c = pc.CASES[CASE]
    st, p = pc.plan(pc.bind_plan(audioflux_amd.get_lib()), kind, *pc.ctor_args(CASE))
    assert st == 0
    mn, mx, w = p["minIndex"], p["maxIndex"], pc.restate_window(p)
    fre, fre2 = kind + "/fre", kind + "/fre2"
    assert int(got[kind + "/frames"]) == int(want[kind + "/frames"]) == len(want[fre])
    assert got[fre].dtype == want[fre].dtype and got[fre2].shape == want[fre2].shape
    eps = np.load(os.path.join(pc.GOLDEN, "pitch_lag.npz"))[f"{kind}/{CASE}/eps"]
    x = pc.case_input(CASE)
    frames = pr.pitch(kind, x, w, c[3], c[4], mn, mx)
    check_case("dropin", frames, eps, want[fre], got[fre], c[0])
    check_case("dropin channel 0", frames, eps, want[fre2][0], got[fre2][0], c[0])
    rev = pr.pitch(kind, x[::-1].copy(), w, c[3], c[4], mn, mx)
    check_case("dropin channel 1", rev, np.full(len(rev), 1e-5), want[fre2][1], got[fre2][1], c[0])
