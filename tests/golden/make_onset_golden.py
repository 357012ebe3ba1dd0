#!/usr/bin/env python3
"""Writes tests/golden/onset.npz: the outputs of the compiled reference's onsetObj_onset and util_powerToDB (oracle.ref.lib())
for the cases of tests/onset_cases.py.  Inputs are regenerated from seeds; only outputs are stored.
Keys: <case>/evn [T], /points, /eps [1] (the yardstick of tests/onset_check.py), /pick [5] (the reference's pick parameters
of the case's samplate / slideLength); grid/pairs [n, 2], grid/params [n, 5], grid/delta [n]: the pick parameters parsed from
what onsetObj_debug prints in a child process; db/out: util_powerToDB of the plane tests/onset_cases.py: burst_power(60, 16, 7).
A case is REFUSED when the reference itself has a marginal pick decision (tests/onset_check.py) or its points differ from the
float64 restatement's: replace such a case, the bar stays.

    python tests/golden/make_onset_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import onset_cases as oc  # noqa: E402
from tests import onset_restate as rs  # noqa: E402
from tests.onset_check import check_case, marginal_frames, reference_eps  # noqa: E402


def reference_case(lib, name, pick, delta):
    """-> evn, points, eps, e64 of one case run through the compiled reference; refuses a marginal case"""
    c = oc.CASES[name]
    spec, phase = oc.case_input(name)
    evn, pts = oc.run_case(lib, name, spec, phase)
    e64 = rs.envelope64(spec, phase, c["kind"], c["order"], c["param"], c["index"])
    eps = reference_eps(e64, evn)
    assert eps <= 4e-5, f"{name}: the reference's envelope is {eps / 4:.2e} from the restatement: no yardstick"
    marg = marginal_frames(e64, pick, delta, eps)
    assert len(marg) == 0, f"{name}: REFUSED, the reference's decision is marginal at frames {marg.tolist()}"
    p64 = rs.pick(e64, pick, delta, np.float64)
    assert np.array_equal(p64, pts), f"{name}: REFUSED, reference points {pts.tolist()} != float64 points {p64.tolist()}"
    check_case(f"{name} (reference)", e64, eps, pts, evn, pts, pick, delta)
    return evn, pts, eps, e64


def main():
    from oracle import ref
    lib = oc.bind(ref.lib())
    out = {}
    params, deltas = oc.debug_params(ref.REF_PATH, oc.GRID)
    out["grid/pairs"], out["grid/params"], out["grid/delta"] = np.array(oc.GRID, np.int32), params, deltas
    for (sr, hop), row, d in zip(oc.GRID, params, deltas):
        mine, md = rs.pick_params(sr, hop)
        assert mine == row.tolist() and md == d, (sr, hop, mine, row)
    for name, c in oc.CASES.items():
        pick, delta = oc.debug_params(ref.REF_PATH, [(c["sr"], c["hop"])])
        pick, delta = pick[0].tolist(), delta[0]
        evn, pts, eps, _ = reference_case(lib, name, pick, delta)
        out[name + "/evn"], out[name + "/points"] = evn, pts
        out[name + "/eps"], out[name + "/pick"] = np.array([eps], np.float64), np.array(pick, np.int32)
        print(f"{name}: T {c['T']}, eps {eps:.2e}, pick {pick}, {len(pts)} points {pts[:8].tolist()}")
    p = oc.burst_power(60, 16, 7).astype(np.float32)
    db = np.zeros(p.size, np.float32)
    lib.util_powerToDB(p.reshape(-1).ctypes.data_as(oc.fp), p.size, C.c_float(-80.0), db.ctypes.data_as(oc.fp))
    out["db/out"] = db.reshape(p.shape)
    path = os.path.join(ROOT, "tests", "golden", "onset.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
