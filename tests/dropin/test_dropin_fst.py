"""Drop-in boundary of the FST: the reference's OWN unmodified `audioflux.FST` wrapper, staged as tests/dropin/test_dropin.py
stages it, runs its docstring flow once on the stock library and once on libaudioflux_mi355x.so, in fresh interpreters
(tests/dropin/flows_fst.py): sizes, coordinates and get_fre_band_arr identical, the complex result and its magnitude at the
bar of tests/fst_cases.py.  CPU part: the wrapper resolves fstObj_new, fstObj_fst and fstObj_free from the product library."""
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
    out = os.path.join(tmp, f"fst_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_fst.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_fst.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_fst_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    assert meta["symbols"] == ["fstObj_free", "fstObj_fst", "fstObj_new"]
    assert meta["missing"] == [], f"fst.py looks up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_fst"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("flow,shape", [("doc", (1024, 4096)), ("default", (255, 512))])
def test_docstring_flow_matches_stock(both, flow, shape):
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    for k in ("num", "fft_length", "fre", "x_coords", "y_coords"):
        a, b = got[f"{flow}/{k}"], want[f"{flow}/{k}"]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (flow, k)
    for k in ("spec", "abs"):
        a, b = got[f"{flow}/{k}"], want[f"{flow}/{k}"]
        assert a.shape == b.shape == shape and a.dtype == b.dtype and np.all(np.isfinite(a)), (flow, k)
        # the metric of tests/fst_cases.py with the peak of the rows at hand (<= the chunk's: not a wider bar); the stock
        # result's own distance from float64 is <= 4e-7 there
        e = np.abs(a - b).max() / np.abs(b).max()
        parity_log(f"dropin fst {flow}/{k}", e, 1e-5, "fst: max|got - want| over the rows / max|want|")
        print(f"dropin fst {flow}/{k}: {e:.2e}")
        assert e <= 1e-5, (flow, k, e)
