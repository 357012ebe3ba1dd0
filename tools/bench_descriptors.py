#!/usr/bin/env python3
"""Times spectralObj_computeDevice on rows that are resident on the device (device events, warm-up, timed loops of >= 0.4 s):
934 000 x 128 mel rows (the headline batch of bench.py) and 233 500 x 1025 linear rows; (i) centroid alone, (ii) the 19
row-local descriptors in one call, (iii) flux + novelty + mkl, (iv) all 30.  Prints ms per call and algorithmic TB/s, where
algorithmic bytes = rows x edge length x 4 (x 2 with phase) + slots x rows x 4.

    python tools/bench_descriptors.py [--rows-scale 1.0] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = ("flatness", "rolloff", "centroid", "spread", "skewness", "kurtosis", "entropy", "crest", "slope", "decrease", "bandwidth",
       "rms", "energy", "hfc", "eef", "eer", "max", "mean", "var")
DEFAULTS = {"rolloff": ((), (0.95,)), "bandwidth": ((), (2.0,)), "energy": ((0,), (10.0,)), "eer": ((0,), (1.0,)),
            "flux": ((1, 0, 0, 0), (2.0,)), "sd": ((1, 0), ()), "sf": ((1, 0), ()), "novelty": ((1, 0, 0), (0.0,))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-scale", type=float, default=1.0)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import torch

    import audioflux_amd as af
    from audioflux_amd.spectral import KINDS, request

    def reqs(names):
        return [request(n, *DEFAULTS.get(n, ((), ()))) for n in names]

    cases = (("centroid alone", ("centroid",)), ("19 row-local", ROW), ("flux + novelty + mkl", ("flux", "novelty", "mkl")),
             ("all 30", KINDS))
    results = []
    for label, rows, num in (("mel", int(934000 * a.rows_scale), 128), ("linear", int(233500 * a.rows_scale), 1025)):
        g = torch.Generator(device="cuda").manual_seed(1)
        spec = torch.rand((rows, num), generator=g, device="cuda") ** 4 * 50.0 + 1e-3
        phase = (torch.rand((rows, num), generator=g, device="cuda") - 0.5) * 6.0
        o = af.Spectral(num, np.arange(num, dtype=np.float32) * 15.625)
        for cname, names in cases:
            rq = reqs(names)
            use_phase = any(n in ("pd", "wpd", "nwpd", "cd", "rcd") for n in names)
            out = o.compute_device(spec, rq, phase=phase if use_phase else None)
            slots = out.shape[0]
            for _ in range(5):
                o.compute_device(spec, rq, phase=phase if use_phase else None, out=out)
            torch.cuda.synchronize()
            best, total, loops = None, 0.0, 0
            while total < 0.4 or loops < 3:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                n = 10
                e0.record()
                for _ in range(n):
                    o.compute_device(spec, rq, phase=phase if use_phase else None, out=out)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1) / n
                best = ms if best is None else min(best, ms)
                total += ms * n / 1e3
                loops += 1
            nbytes = rows * num * 4 * (2 if use_phase else 1) + slots * rows * 4
            rec = {"rows": rows, "num": num, "case": cname, "slots": slots, "ms_per_call": round(best, 4),
                   "algorithmic_TBps": round(nbytes / (best * 1e-3) / 1e12, 3)}
            results.append(rec)
            if not a.json:
                print(f"{label:6s} {rows:7d} x {num:4d}  {cname:22s} {slots:2d} slots  {best:8.4f} ms  {rec['algorithmic_TBps']:6.3f} TB/s", flush=True)
        del spec, phase
    if a.json:
        print(json.dumps(results))


if __name__ == "__main__":
    main()
