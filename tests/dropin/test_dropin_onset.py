"""Drop-in boundary of onset detection: the reference's OWN unmodified `audioflux.Onset` wrapper and
`audioflux.utils.power_to_db`, staged as tests/dropin/test_dropin.py stages them, run the Onset docstring flow (BFT ->
power_to_db -> Onset.onset) once on the stock library and once on libaudioflux_mi355x.so, in fresh interpreters
(tests/dropin/flows_onset.py).  Shapes and dtypes are identical; the dB planes agree within what the 1e-5 peak-relative bar
of the mel power allows per element (d dB = 10 / ln 10 * d p / p); the product's envelope and points meet the rule of
tests/onset_check.py against the compiled reference run on the product's own dB plane.  CPU part: the wrapper resolves every
symbol it looks up from the product library."""
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
    out = os.path.join(tmp, f"onset_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_onset.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_onset.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_onset_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {"onsetObj_new", "onsetObj_onset", "onsetObj_free", "util_powerToDB"}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrapper looks up symbols the library does not export: {meta['missing']}"


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dropin_onset"))
    return _run(tmp, "stock"), _run(tmp, "mi355x")


@pytest.mark.gpu
@needs_inputs
def test_docstring_flow_matches_stock(both):
    from oracle import ref
    from tests import onset_cases as oc
    from tests import onset_restate as rs
    from tests.onset_check import check_case, reference_eps
    from flows_onset import HOP, SR
    (want, wmeta), (got, gmeta) = both
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    for k in want.files:
        if k != "meta" and not k.startswith(("point", "time", "value")):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    for k in ("point", "time", "value"):
        assert got[k].dtype == want[k].dtype and got[k].ndim == want[k].ndim, k
    # mel power at the library's bar; dB within what that allows per element
    peak = np.abs(want["power"]).max()
    assert np.abs(got["power"] - want["power"]).max() <= 1e-5 * peak
    for k, p in (("db", want["power"]), ("db2", np.stack([want["power"], 2 * want["power"]]))):
        allowed = 10 / np.log(10) * 1e-5 * p.reshape(got[k].shape[:-2] + (-1,)).max(axis=-1).reshape(got[k].shape[:-2] + (1, 1)) / \
            np.maximum(p, 1e-30) * 1.5 + 1e-4
        clamped = (want[k] <= -80) | (got[k] <= -80)
        assert (np.abs(got[k] - want[k]) <= np.where(clamped, np.inf, allowed)).all(), k
        assert np.abs(got[k] - want[k])[clamped].max(initial=0) <= allowed[clamped].max(initial=0) + 1e-3
    assert np.array_equal(got["db2"][0].view(np.uint32), got["db"].view(np.uint32))
    # the product's onset on its own dB plane, against the compiled reference on the same plane
    lib = oc.bind(ref.lib())
    pick, delta = rs.pick_params(SR, HOP)
    par = (1, 2.0, 0, 1, 0, 0.0, 0, 1.0)
    for tag, db, evn, pts in (("one channel", got["db"], got["evn"], got["point"]),
                              ("default parameters", got["db"], got["evn_default"], got["point_default"])):
        rows = np.ascontiguousarray(db.T)  # [time, fre]
        p = (1, 1.0, 1, 0, 1, 0.0, 1, 1.0) if tag.startswith("default") else par
        st, obj = oc.new(lib, rows.shape[0], rows.shape[1], HOP, SR)
        n, ref_evn, ref_pts = oc.call(lib, obj, rows, None, p)
        lib.onsetObj_free(obj)
        e64 = rs.envelope64(rows, None, oc.FLUX, 1, p)
        check_case(f"dropin {tag}", e64, reference_eps(e64, ref_evn), ref_pts, evn, pts, pick, delta)
    assert np.array_equal(got["value"], got["evn"][got["point"]]) and np.allclose(got["time"], got["point"] * HOP / SR)
    assert len(got["point"]) >= 3 and len(want["point"]) >= 3
