"""Drop-in boundary of time stretch and pitch shift: the reference's OWN unmodified `audioflux.TimeStretch` /
`audioflux.PitchShift` wrappers, staged as tests/dropin/test_dropin.py stages them, run their docstring flows once on the stock
library and once on libaudioflux_mi355x.so, in fresh interpreters (tests/dropin/flows_timestretch.py): shapes and dtypes are
identical and the samples agree within the bars the fixture records per flow and channel (measured from the reference
alone, tests/golden/make_timestretch_golden.py).  CPU part: the wrappers resolve every timeStretchObj_* /
pitchShiftObj_* symbol they look up from the product library, pitchShiftObj__free included."""
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

FLOWS = ("stretch_0.8", "stretch_0.5", "stretch_1.5", "shift_+3", "shift_-5")  # timestretch_cases.DROPIN_STRETCH / DROPIN_SHIFT


def _run(tmp, mode):
    out = os.path.join(tmp, f"timestretch_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_timestretch.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_timestretch.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrappers_resolve_every_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {f"timeStretchObj_{n}" for n in ("new", "calDataCapacity", "timeStretch", "free")}
    want |= {"pitchShiftObj_new", "pitchShiftObj_pitchShift", "pitchShiftObj__free"}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrappers look up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_timestretch"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
@pytest.mark.parametrize("flow", FLOWS)
def test_docstring_flow_matches_stock(flow, both):
    from tests import timestretch_cases as tc
    assert set(FLOWS) == set(tc.DROPIN_STRETCH) | set(tc.DROPIN_SHIFT)
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    for key in (flow + "/one", flow + "/two"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and want[key].shape[-1] >= 2000, key
        assert np.isfinite(got[key]).all(), key
        for ch, (g, w) in enumerate(zip(np.atleast_2d(got[key]), np.atleast_2d(want[key]))):
            bp, bl = tc.bar(f"dropin/{flow}/{ch}")
            p, l2 = tc.errors(g, w)
            print(f"dropin/timestretch/{key}[{ch}]: peak-rel {p:.3e} (bar {bp:.1e}), l2-rel {l2:.3e} (bar {bl:.1e})")
            assert p <= bp and l2 <= bl, (key, ch, p, l2)
    assert np.array_equal(got[flow + "/two"][0], got[flow + "/one"])
