#!/usr/bin/env python3
"""Writes tests/golden/pitch_hs.npz: the outputs of the compiled reference's pitchHPSObj_pitch / pitchLHSObj_pitch
(oracle.ref.lib()) for the cases of tests/pitch_hs_cases.py.  Inputs are regenerated from seeds; only outputs are stored.
Keys: <case>/<HPS|LHS>/fre [T], /eps [T] (the yardstick of tests/pitch_hs_check.py: the reference's own distance from the
float64 restatement, from the curve rows the reference kept), and for a few cases /curve64 [T, maxIndex + 1] (the
restatement's curve as float32).  Every case is first held to the acceptance rule itself, reference against restatement:
the inputs are then known to keep the reference inside the cap that the library is held to.

    python tests/golden/make_pitch_hs_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import pitch_hs_cases as hc  # noqa: E402
from tests import pitch_hs_restate as hr  # noqa: E402
from tests.pitch_hs_check import check_case, check_curve, reference_eps  # noqa: E402


def reference_case(lib, name, kind, x=None):
    """-> fre, eps, frames64 of one case run through the compiled reference"""
    _, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
    x = hc.case_input(name) if x is None else x
    M, mn, mx, cnt, wt = hc.plan(kind, sr, lo, hi, r, hop, window, count)
    st, obj = hc.new(lib, kind, sr, lo, hi, r, hop, window, count)
    assert st == 0 and obj, (name, st)
    fre = hc.call(lib, kind, obj, x)
    f = hc.ref_fields(obj)
    assert (f["interpLength"], f["minIndex"], f["maxIndex"]) == (M, mn, mx), (name, f)
    rows = hc.ref_curves(obj, kind)
    hc.free(lib, kind, obj)
    frames = hr.pitch(kind, x, sr, r, hop, wt, M, mn, mx, cnt)
    eps = np.array([reference_eps(fr, rows[t]) for t, fr in enumerate(frames)], np.float32)
    for t, fr in enumerate(frames):
        # the reference's own rows under the curve rule (the three entries its peak pick overwrote taken as correct): a frame
        # where float32 rounding turned one of ITS bins into an exact 0 / -inf is no yardstick -- such a case is replaced
        row = np.where(np.isnan(rows[t]), fr["curve"], rows[t].astype(np.float64))
        check_curve(f"{name}/{hc.KIND_NAME[kind]} (reference)", t, fr, float(eps[t]), row)
    return fre, eps, frames


def main():
    from oracle import ref
    lib = hc.bind(ref.lib())
    out = {}
    for name, kind in hc.pairs():
        sr = hc.CASES[name][1]
        fre, eps, frames = reference_case(lib, name, kind)
        M = hc.round_pow2(sr)
        fre64 = np.array([hr.fre_of(f["index"], sr, M) for f in frames], np.float32)
        w = check_case(f"{name}/{hc.KIND_NAME[kind]} (reference)", frames, eps, fre64, fre, sr, M)
        key = f"{name}/{hc.KIND_NAME[kind]}"
        out[key + "/fre"], out[key + "/eps"] = fre, eps
        if name in hc.CURVES:
            out[key + "/curve64"] = np.array([f["curve"] for f in frames], np.float32)
        print(f"{key}: {len(fre)} frames, eps up to {eps.max():.2e}, {w['explained']} explained, fre {fre[:4]}")
    path = os.path.join(ROOT, "tests", "golden", "pitch_hs.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
