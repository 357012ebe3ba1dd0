"""Drop-in boundary of the harmonic ratio: the reference's OWN unmodified `audioflux.HarmonicRatio` wrapper, staged as
tests/dropin/test_dropin.py stages it, runs its flow once on the stock library and once on libaudioflux_mi355x.so, in fresh
interpreters (tests/dropin/flows_harmonic_ratio.py): the frame count is identical and the values meet the rule of
tests/harmonic_ratio_check.py.  CPU part: the wrapper resolves every harmonicRatioObj_* symbol it looks up from the product
library."""
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
    out = os.path.join(tmp, f"harmonic_ratio_{mode}.npz")
    env = dict(os.environ, AFX_HIP_RUNTIME="system")
    res = subprocess.run([sys.executable, os.path.join(HERE, "flows_harmonic_ratio.py"), os.path.join(tmp, "pkg_" + mode), out, mode],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=tmp)
    assert res.returncode == 0, f"flows_harmonic_ratio.py {mode} died (rc {res.returncode}):\n{res.stdout[-4000:]}"
    data = np.load(out)
    return data, json.loads(str(data["meta"]))


@needs_inputs
def test_wrapper_resolves_every_harmonic_ratio_symbol(tmp_path):
    _, meta = _run(str(tmp_path), "cpu")
    assert os.path.realpath(meta["lib"]) == os.path.realpath(flows.PRODUCT)
    want = {f"harmonicRatioObj_{n}" for n in ("new", "calTimeLength", "harmonicRatio", "free")}
    assert want <= set(meta["symbols"]), meta["symbols"]
    assert meta["missing"] == [], f"the wrapper looks up symbols the library does not export: {meta['missing']}"


@pytest.mark.gpu
@needs_inputs
def test_wrapper_flow_matches_stock(tmp_path):
    import audioflux_amd
    from tests import harmonic_ratio_cases as hc
    from tests import harmonic_ratio_restate as hr
    from tests.harmonic_ratio_check import check_case, reference_eps
    from flows_harmonic_ratio import CASE
    tmp = str(tmp_path)
    (want, wmeta), (got, gmeta) = _run(tmp, "stock"), _run(tmp, "mi355x")
    assert os.path.realpath(wmeta["lib"]) == os.path.realpath(flows.STOCK)
    assert os.path.realpath(gmeta["lib"]) == os.path.realpath(flows.PRODUCT)
    c = hc.CASES[CASE]
    st, p = hc.plan(hc.bind_device(audioflux_amd.get_lib()), *hc.ctor_args(CASE))
    assert st == 0
    assert int(got["frames"]) == int(want["frames"]) == len(want["value"]) == c[5]
    assert got["value"].dtype == want["value"].dtype and got["value2"].shape == want["value2"].shape == (2, c[5])
    eps = np.load(os.path.join(hc.GOLDEN, "harmonic_ratio.npz"))[f"{CASE}/eps"]
    x = hc.case_input(CASE)
    frames = hr.harmonic_ratio(x, p["window"], c[2], c[3], p["maxLength"])
    check_case("dropin", frames, eps, got["value"], p["maxLength"])
    check_case("dropin channel 0", frames, eps, got["value2"][0], p["maxLength"])
    # the second channel is no fixture case: its yardstick is the stock library's own distance from the restatement, as the rule says
    rev = hr.harmonic_ratio(x[::-1].copy(), p["window"], c[2], c[3], p["maxLength"])
    eps1 = [reference_eps(f, want["value2"][1][t]) for t, f in enumerate(rev)]
    check_case("dropin channel 1", rev, eps1, got["value2"][1], p["maxLength"])
