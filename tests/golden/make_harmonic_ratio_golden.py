#!/usr/bin/env python3
"""Writes tests/golden/harmonic_ratio.npz: the outputs of the compiled reference's harmonicRatioObj_harmonicRatio
(oracle.ref.lib()) for the cases of tests/harmonic_ratio_cases.py.  Inputs are regenerated from seeds; only outputs are
stored.  Keys: <case>/value [T] (the reference's), /eps [T] (the yardstick of tests/harmonic_ratio_check.py: the reference's own
distance from the float64 restatement in units of the value's weight), /plan [windowLength, fftLength, slideLength,
maxLength], /first and /lag [T] (the restatement's decisions) and /value64 [T]; `window/<N>` holds the float32 Hamming table
the reference built, for the sizes up to 256.  AFX_PARITY_LOG=<file> receives the measured figures.

    python tests/golden/make_harmonic_ratio_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import harmonic_ratio_cases as hc  # noqa: E402
from tests import harmonic_ratio_restate as hr  # noqa: E402
from tests.conftest import parity_log  # noqa: E402
from tests.harmonic_ratio_check import check_case, reference_eps  # noqa: E402


def reference_case(lib, name, x=None):
    """-> value, eps, frames64, fields, window of one case run through the compiled reference"""
    c = hc.CASES[name]
    x = hc.case_input(name) if x is None else x
    st, obj = hc.new(lib, *hc.ctor_args(name))
    assert st == 0 and obj, (name, st)
    value = hc.call(lib, obj, x)
    f, window = hc.ref_fields(obj), hc.ref_window(obj)
    lib.harmonicRatioObj_free(obj)
    frames = hr.harmonic_ratio(x, window, c[2], c[3], f["maxLength"])
    eps = np.array([reference_eps(fr, value[t]) for t, fr in enumerate(frames)], np.float32)
    return value, eps, frames, f, window


def main():
    from oracle import ref
    lib = hc.bind(ref.lib())
    out = {}
    for name in hc.CASES:
        value, eps, frames, f, window = reference_case(lib, name)
        check_case(f"{name} (reference)", frames, eps, value, f["maxLength"])
        out[name + "/value"], out[name + "/eps"] = value, eps
        out[name + "/plan"] = np.array([f["windowLength"], f["fftLength"], f["slideLength"], f["maxLength"]], np.int32)
        out[name + "/first"] = np.array([fr["first"] for fr in frames], np.int32)
        out[name + "/lag"] = np.array([fr["lag"] for fr in frames], np.int32)
        out[name + "/value64"] = np.array([fr["value"] for fr in frames], np.float64)
        if f["windowLength"] <= 256:
            out[f"window/{f['windowLength']}"] = window
        W = np.array([fr["W"] for fr in frames])
        off = np.abs(value.astype(np.float64) - out[name + "/value64"])
        rel = np.where(W > 0, off / np.where(W > 0, W, 1.0), 0.0)
        parity_log(f"harmonic_ratio/reference/{name}", float(rel.max()), 1e-5, "harmonic_ratio: |reference - float64| / W",
                   {"worst_abs": float(off.max()), "eps_max": float(eps.max())})
        print(f"{name}: {len(value)} frames, |ref - f64| up to {off.max():.2e} ({rel.max():.2e} of W), eps up to {eps.max():.2e}, "
              f"found {[int(fr['own'] is not None) for fr in frames]}, first {out[name + '/first'].tolist()}, value {value[:4]}")
    path = os.path.join(ROOT, "tests", "golden", "harmonic_ratio.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
