"""Drop-in boundary of the NSGT: the reference's OWN unmodified `audioflux.NSGT` wrapper, staged as tests/dropin/test_dropin.py
stages it, runs its docstring flow once on the stock library and once on libaudioflux_mi355x.so, in fresh interpreters
(tests/dropin/flows_nsgt.py): getters and coordinates identical, the complex result and its magnitude per band at the bar of
tests/nsgt_cases.py.  CPU part: the wrapper resolves every nsgtObj_* symbol it looks up from the product library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import parity_log

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402

needs_inputs = pytest.mark.skipif(
    not (os.path.exists(flows.STOCK) and os.path.exists(flows.PRODUCT) and os.path.exists(flows.WRAPPER_ZIP)),
    reason="needs the compiled reference with its wrapper archive and the built product library")


def _run(tmp, mode):
    out = os.path.join(tmp, f"nsgt_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_nsgt.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_nsgt.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_nsgt_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    assert len(meta["symbols"]) >= 9 and "nsgtObj_new" in meta["symbols"] and "nsgtObj_setMinLength" in meta["symbols"]
    assert meta["missing"] == [], f"nsgt.py looks up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_nsgt"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("flow", ["oct84", "mel12"])
def test_docstring_flow_matches_stock(both, flow):
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    for k in ("max", "total", "len", "fre", "bin", "x_coords", "y_coords"):
        a, b = got[f"{flow}/{k}"], want[f"{flow}/{k}"]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (flow, k)
    for k in ("spec", "abs"):
        a, b = got[f"{flow}/{k}"], want[f"{flow}/{k}"]
        assert a.shape == b.shape and a.dtype == b.dtype and np.all(np.isfinite(a)), (flow, k)
        peak = np.abs(b).max(axis=-1)
        assert np.all(peak > 0), (flow, k)
        e = np.abs(a - b).max(axis=-1) / peak  # per band; the stock result's own distance from float64 is <= 3.7e-7: bar 1e-5
        parity_log(f"dropin nsgt {flow}/{k}", e.max(), 1e-5, "nsgt: per band max|got - want| / max|want|")
        print(f"dropin nsgt {flow}/{k}: worst band {e.max():.2e}")
        assert e.max() <= 1e-5, (flow, k, int(np.argmax(e)), e.max())
