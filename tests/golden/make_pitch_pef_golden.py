#!/usr/bin/env python3
"""Writes tests/golden/pitch_pef.npz: the outputs of the compiled reference's pitchPEFObj_pitch (oracle.ref.lib()) for the
cases of tests/pitch_pef_cases.py.  Inputs are regenerated from seeds; only outputs are stored.
Keys: <case>/fre [T], /eps [T] (the yardstick of tests/pitch_pef_check.py: the reference's own distance from the float64
restatement, from the curve rows the reference kept), /plan [minIndex, maxIndex, filterPadNum], and for a few small cases
/curve64 [T, maxIndex + 1] (the restatement's curve as float32) and the float32 tables /lg /bw /h /window the reference
built.  A case is REFUSED when the reference itself breaks the acceptance rule against the restatement, or when its curve
is further than 1e-5 S from it (it is no yardstick there): replace such a case, the bar stays.

    python tests/golden/make_pitch_pef_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import pitch_pef_cases as pc  # noqa: E402
from tests import pitch_pef_restate as pr  # noqa: E402
from tests.pitch_pef_check import FLOOR, check_case, check_curve, reference_eps  # noqa: E402


def reference_case(lib, name, x=None):
    """-> fre, eps, frames64, fields, tables of one case run through the compiled reference"""
    c = pc.CASES[name]
    x = pc.case_input(name) if x is None else x
    st, obj = pc.new(lib, *pc.ctor_args(name))
    assert st == 0 and obj, (name, st)
    fre = pc.call(lib, obj, x)
    f, tables, rows = pc.ref_fields(obj), pc.ref_tables(obj), pc.ref_curves(obj)
    lib.pitchPEFObj_free(obj)
    frames = pr.pitch(x, tables, c[4], c[5], f["filterPadNum"], f["minIndex"], f["maxIndex"])
    eps = np.array([reference_eps(fr, rows[t]) for t, fr in enumerate(frames)], np.float32)
    assert (eps <= FLOOR).all(), f"{name}: the reference's curve is {eps.max() / 4:.2e} S from the restatement: no yardstick"
    for t, fr in enumerate(frames):
        check_curve(f"{name} (reference)", t, fr, float(eps[t]), rows[t])
    return fre, eps, frames, f, tables


def main():
    from oracle import ref
    lib = pc.bind(ref.lib())
    out = {}
    for name in pc.CASES:
        fre, eps, frames, f, tables = reference_case(lib, name)
        fre64 = np.array([tables["lg"][fr["index"]] for fr in frames], np.float32)
        w = check_case(f"{name} (reference)", frames, eps, fre64, fre, tables["lg"], f["minIndex"])
        out[name + "/fre"], out[name + "/eps"] = fre, eps
        out[name + "/plan"] = np.array([f["minIndex"], f["maxIndex"], f["filterPadNum"]], np.int32)
        if name in pc.CURVES:
            out[name + "/curve64"] = np.array([fr["curve"] for fr in frames], np.float32)
            for k in ("lg", "bw", "h", "window"):
                out[f"{name}/{k}"] = tables[k]
        print(f"{name}: {len(fre)} frames, eps up to {eps.max():.2e}, {w['explained']} explained, fre {fre[:4]}")
    path = os.path.join(ROOT, "tests", "golden", "pitch_pef.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
