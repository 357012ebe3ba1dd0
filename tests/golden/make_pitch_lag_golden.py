#!/usr/bin/env python3
"""Writes tests/golden/pitch_lag.npz: the outputs of the compiled reference's pitchNCFObj_pitch / pitchCEPObj_pitch
(oracle.ref.lib()) for the cases of tests/pitch_lag_cases.py.  Inputs are regenerated from seeds; only outputs are stored.
Keys, kind = NCF / CEP: <kind>/<case>/fre [T], /eps [T] (the yardstick of tests/pitch_lag_check.py: the reference's own
distance from the float64 restatement, from the curve rows the reference kept), /plan [minIndex, maxIndex], and for a few
small cases /curve64 [T, maxIndex + 1] (the restatement's curve as float32) and /window (the float32 table the reference
built).  A case is REFUSED when the reference itself breaks the acceptance rule against the restatement: replace such a
case, the bar stays.

    python tests/golden/make_pitch_lag_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import pitch_lag_cases as pc  # noqa: E402
from tests import pitch_lag_restate as pr  # noqa: E402
from tests.pitch_lag_check import check_case, check_curve, reference_eps  # noqa: E402


def reference_case(lib, kind, name, x=None):
    """-> fre, eps, frames64, fields, window of one case run through the compiled reference (a fresh object: its row buffer
    holds no NaN of an earlier call)"""
    c = pc.CASES[name]
    x = pc.case_input(name) if x is None else x
    st, obj = pc.new(lib, kind, *pc.ctor_args(name))
    assert st == 0 and obj, (kind, name, st)
    fre = pc.call(lib, kind, obj, x)
    f, window, rows = pc.ref_fields(obj), pc.ref_window(obj), pc.ref_curves(obj)
    pc.fn(lib, kind, "free")(obj)
    assert f["maxIndex"] <= (f["fftLength"] - 1 if kind == "NCF" else 2 * f["fftLength"] - 1), (kind, name, f)
    w = None if pc.window_of(kind, name) == pc.RECT else window
    frames = pr.pitch(kind, x, w, c[3], c[4], f["minIndex"], f["maxIndex"])
    eps = np.array([reference_eps(fr, rows[t]) for t, fr in enumerate(frames)], np.float32)
    for t, fr in enumerate(frames):
        live = np.isfinite(rows[t]) | np.isnan(fr["curve"])  # not overwritten by the peak pick
        g = np.where(live, rows[t].astype(np.float64), fr["curve"])
        check_curve(f"{kind}/{name} (reference)", t, fr, float(eps[t]), g)
    return fre, eps, frames, f, window


def main():
    from oracle import ref
    lib = pc.bind(ref.lib())
    out = {}
    for kind in pc.KINDS:
        for name in pc.CASES:
            fre, eps, frames, f, window = reference_case(lib, kind, name)
            sr = pc.CASES[name][0]
            fre64 = pr.fre_of([fr["index"] for fr in frames], sr)
            w = check_case(f"{kind}/{name} (reference)", frames, eps, fre64, fre, sr)
            key = f"{kind}/{name}"
            out[key + "/fre"], out[key + "/eps"] = fre, eps
            out[key + "/plan"] = np.array([f["minIndex"], f["maxIndex"]], np.int32)
            if name in pc.CURVES:
                out[key + "/curve64"] = np.array([fr["curve"] for fr in frames], np.float32)
                out[key + "/window"] = window
            print(f"{key}: {len(fre)} frames, eps up to {eps.max():.2e}, {w['explained']} explained, fre {fre[:4]}")
    path = os.path.join(ROOT, "tests", "golden", "pitch_lag.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
