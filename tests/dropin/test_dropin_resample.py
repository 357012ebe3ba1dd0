"""Drop-in boundary of the resampler: the reference's OWN unmodified `audioflux.Resample` / `audioflux.WindowResample`
wrappers, staged as tests/dropin/test_dropin.py stages them, run their docstring flow once on the stock library and once on
libaudioflux_mi355x.so, in fresh interpreters (tests/dropin/flows_resample.py): shapes and dtypes are identical and the
samples agree to 1e-5 peak- and L2-relative.  CPU part: the wrapper resolves every resampleObj_* symbol it looks up from the
product library."""
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
    out = os.path.join(tmp, f"resample_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_resample.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_resample.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_resample_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {f"resampleObj_{n}" for n in ("new", "newWithWindow", "setSamplate", "calDataLength", "resample", "free")}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrapper looks up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_resample"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("flow", ["best", "fast", "window", "up_scaled"])
def test_docstring_flow_matches_stock(flow, both):
    from tests.conftest import assert_parity
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    for key in (flow + "/one", flow + "/two"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and want[key].shape[-1] >= 2000, key
        assert_parity(got[key], want[key], what=f"dropin/resample/{key}")
    assert_parity(got[flow + "/two"][1], want[flow + "/two"][1], what=f"dropin/resample/{flow}/channel 1")
