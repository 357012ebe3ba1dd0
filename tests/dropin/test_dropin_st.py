"""Drop-in boundary of the ST: the reference's OWN unmodified `audioflux.ST` wrapper, staged as tests/dropin/test_dropin.py
stages it, runs its flows once on the stock library and once on libaudioflux_mi355x.so, in fresh interpreters
(tests/dropin/flows_st.py): sizes, coordinates and get_fre_band_arr identical, the complex results (st, after set_value, after
use_bin_arr) at the bar of tests/st_cases.py.  CPU part: the wrapper resolves every stObj_* it looks up from the product
library."""
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
    out = os.path.join(tmp, f"st_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_st.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_st.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_st_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    assert meta["symbols"] == ["stObj_free", "stObj_new", "stObj_setValue", "stObj_st", "stObj_useBinArr"]
    assert meta["missing"] == [], f"st.py looks up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_st"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("flow,shape,keys", [("doc", (1024, 4096), ("spec", "abs")),
                                             ("default", (255, 512), ("spec", "abs", "spec_set_value", "spec_bin_arr"))])
def test_flows_match_stock(both, flow, shape, keys):
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    for k in ("num", "fft_length", "fre", "x_coords", "y_coords"):
        a, b = got[f"{flow}/{k}"], want[f"{flow}/{k}"]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (flow, k)
    for k in keys:
        a, b = got[f"{flow}/{k}"], want[f"{flow}/{k}"]
        assert a.shape == b.shape == shape and a.dtype == b.dtype and np.all(np.isfinite(a)), (flow, k)
        # the metric of tests/st_cases.py: the peak of the requested rows; the stock result's own distance from float64 is
        # <= 4.3e-7 on these inputs, so the floor of the bar governs
        e = np.abs(a - b).max() / np.abs(b).max()
        parity_log(f"dropin st {flow}/{k}", e, 1e-5, "st: max|got - want| over the rows / max|want|")
        print(f"dropin st {flow}/{k}: {e:.2e}")
        assert e <= 1e-5, (flow, k, e)
    if flow == "default":  # the float32 words of use_bin_arr are refused by both libraries: the rows stay as they were
        for d in (got, want):
            assert np.array_equal(d["default/spec_bin_arr"], d["default/spec_set_value"])
            assert not np.array_equal(d["default/spec_set_value"], d["default/spec"])
