#!/usr/bin/env python3
"""Onset detection on resident rows (onsetObj_onsetBatchDevice), hipEvent timing: `--clips` clips x `--frames` frames x `--bins`
mel rows in dB, flux with the default parameters at filter order 1 and at `--order` (default 3), envelope + points + counts out.
In the SAME run, rounds alternating: spectralObj_computeDevice with the flux request alone on the same rows -- the parent
library's code and the floor of the onset call; the difference is what normalisation and pick (order 1) and the filtered copy
(order >= 2) cost.  Also the primitives alone (afx_maxFilterDevice, afx_peakPickDevice, afx_powerToDbDevice) with the bytes
each must move, and the compiled reference (oracle/_ref, when built) on one CPU thread of the same machine for a few clips.
Warm-up, then the median and the best of `--iters` timed calls per variant.  Every line is printed and appended to --out.

    python tools/bench_onset.py [--clips 1000] [--frames 934] [--bins 128] [--order 3] [--iters 20]
                                [--out profiles/onset_mi355x.txt] [--reference-clips 4]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR, HOP = 32000, 512


def reference_lines(clips, T, M, order, host_db):
    from oracle import ref
    from tests import onset_cases as oc
    if not ref.available():
        return [{"reference": None, "reason": "oracle/_ref is not built"}]
    lib = oc.bind(ref.lib())
    lines = []
    for o in (1, order):
        st, obj = oc.new(lib, T, M, HOP, SR, o)
        t0 = time.perf_counter()
        for c in range(clips):
            oc.call(lib, obj, host_db[c])
        dt = (time.perf_counter() - t0) / clips
        lib.onsetObj_free(obj)
        lines.append({"reference": "onsetObj_onset", "order": o, "frames": T, "bins": M, "ms_per_clip": round(dt * 1e3, 3),
                      "clips_per_s": round(1 / dt, 1), "note": "one CPU thread, rows in host memory"})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=934)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onset_mi355x.txt"))
    ap.add_argument("--reference-clips", type=int, default=4)
    a = ap.parse_args()
    import torch

    import audioflux_amd as af
    from tests.onset_suite import SpectralRequest
    out = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    B, T, M = a.clips, a.frames, a.bins
    g = torch.Generator(device="cuda").manual_seed(0)
    # decaying bursts per clip and band, 5 % multiplicative noise, as power; then the library's own dB map
    t = torch.arange(T, device="cuda", dtype=torch.float32)[None, :, None]
    p = torch.full((B, T, M), 1e-6, device="cuda")
    for _ in range(12):
        t0 = torch.randint(1, T - 1, (B, 1, 1), device="cuda", generator=g).float()
        tau = 2 + 7 * torch.rand((B, 1, 1), device="cuda", generator=g)
        band = torch.rand((B, 1, M), device="cuda", generator=g) * (torch.rand((B, 1, M), device="cuda", generator=g) < 0.3)
        p += torch.where(t >= t0, torch.exp(-(t - t0).clamp(min=0) / tau), torch.zeros((), device="cuda")) * band
    p *= (1 + 0.05 * torch.randn((B, T, M), device="cuda", generator=g)).clamp(0.5, 1.5)
    db = af.power_to_db_device(p.reshape(B, T * M)).reshape(B, T, M)
    torch.cuda.synchronize()

    lib = af.get_lib()
    lib.spectralObj_new.restype, lib.spectralObj_new.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_float)]
    lib.spectralObj_computeDevice.restype = C.c_int
    lib.spectralObj_computeDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.POINTER(SpectralRequest),
                                              C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    sp = C.c_void_p()
    fre = (C.c_float * M)(*range(M))
    assert lib.spectralObj_new(C.byref(sp), M, fre) == 0
    req = SpectralRequest(1, (C.c_int * 4)(1, 1, 0, 0), (C.c_float * 2)(1.0, 0.0))
    raw = torch.empty(B * T, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def flux_alone():
        assert lib.spectralObj_computeDevice(sp, db.data_ptr(), None, B * T, T, C.byref(req), 1, raw.data_ptr(), B * T, stream) == 0

    o1 = af.Onset(T, M, HOP, samplate=SR, filter_order=1)
    o3 = af.Onset(T, M, HOP, samplate=SR, filter_order=a.order)
    evn = torch.empty((B, T), device="cuda")
    filt = torch.empty((B * T, M), device="cuda")
    variants = {
        "flux_alone (spectralObj_computeDevice)": flux_alone,
        "onset order 1": lambda: o1.onset_device(db),
        f"onset order {a.order}": lambda: o3.onset_device(db),
        "max filter alone": lambda: af.max_filter_device(db.reshape(B * T, M), a.order),
        "peak pick alone": lambda: af.peak_pick_device(evn, 1, 1, 6, 7, 1, 0.07),
        "power to dB alone": lambda: af.power_to_db_device(p.reshape(B, T * M), out=filt.reshape(B, T * M)),
    }
    e0, pts, cnt = o1.onset_device(db)
    evn.copy_(e0)
    for fn in variants.values():  # warm-up: code objects, scratch, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.iters):  # rounds alternate the variants: what shares the machine with us hits all of them alike
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e))
    rows_b = 4.0 * B * T * M
    must_move = {  # bytes each variant has to move through HBM at the least
        "flux_alone (spectralObj_computeDevice)": rows_b + 4.0 * B * T,
        "onset order 1": rows_b + 3 * 4.0 * B * T + 4.0 * B * T,  # rows in, raw out + in, envelope out, points
        f"onset order {a.order}": 3 * rows_b + 3 * 4.0 * B * T + 4.0 * B * T,  # + filtered copy out and in again
        "max filter alone": 2 * rows_b,
        "peak pick alone": 2 * 4.0 * B * T,
        "power to dB alone": 3 * rows_b,  # read for the maxima, read and write for the map
    }
    med = {}
    for k, v in times.items():
        v = sorted(v)
        med[k] = v[len(v) // 2]
        emit({"variant": k, "clips": B, "frames": T, "bins": M, "median_ms": round(med[k], 4), "best_ms": round(v[0], 4),
              "worst_ms": round(v[-1], 4), "iters": len(v), "bytes_at_least": int(must_move[k]),
              "GBps_at_median": round(must_move[k] / med[k] / 1e6, 1)})
    base = med["flux_alone (spectralObj_computeDevice)"]
    emit({"summary": "onset call minus the flux request alone, same rows, same run",
          "normalise_and_pick_ms": round(med["onset order 1"] - base, 4),
          f"filtered_copy_order_{a.order}_ms": round(med[f"onset order {a.order}"] - med["onset order 1"], 4),
          "filtered_copy_bytes": int(2 * rows_b), "points_per_clip_mean": round(float(cnt.float().mean()), 2),
          "clips_per_s_order_1": round(B / med["onset order 1"] * 1e3), f"clips_per_s_order_{a.order}": round(B / med[f"onset order {a.order}"] * 1e3)})
    host_db = db[:max(a.reference_clips, 1)].cpu().numpy()
    for d in reference_lines(a.reference_clips, T, M, a.order, host_db):
        emit(d)


if __name__ == "__main__":
    main()
