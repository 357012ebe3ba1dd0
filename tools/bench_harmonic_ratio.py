#!/usr/bin/env python3
"""Harmonic ratio, device-resident in and out (harmonicRatioObj_harmonicRatioBatchDevice), hipEvent timing: clips x seconds @
32 kHz at window 1024 / 2048 / 4096 (hop window / 4, the wrapper's default low_fre), value, lag and first out.  Warm-up, then
the median of `--iters` timed calls.  Per frame the kernel runs TWO 2 x window-point complex transforms in LDS, as
pitchNCFObj_pitchBatchDevice does at the same size: NCF runs on the same clips in the same process as the yardstick, and the
ratio of the two rates is reported.  Three inputs: harmonic clips (every frame has a zero crossing of its own), a DC batch (no
frame has one: all inherit 0, nothing is run again) and noise in front of DC (all but the first frames inherit a minIndex
that is not 0: every such frame runs twice, the worst case of the design).  With oracle/_ref present the compiled reference
runs one clip on one CPU thread of the same machine.  Every line is printed and appended to --out.

    python tools/bench_harmonic_ratio.py [--clips 200] [--seconds 30] [--iters 10] [--window 1024 2048 4096]
                                         [--out profiles/harmonic_ratio_mi355x.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 32000


def timed(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0]


def reference_rate(x, r, hop, low_fre):
    """frames/s of the compiled reference on one clip (its frame loop is serial), or None"""
    path = os.path.join(ROOT, "oracle", "_ref", "libaudioflux_ref.so")
    if not os.path.exists(path):
        return None
    import numpy as np
    lib = C.CDLL(path)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.harmonicRatioObj_new.argtypes = [C.POINTER(C.c_void_p), ip, fp, ip, ip, ip]
    lib.harmonicRatioObj_calTimeLength.argtypes = [C.c_void_p, C.c_int]
    lib.harmonicRatioObj_harmonicRatio.restype, lib.harmonicRatioObj_harmonicRatio.argtypes = None, [C.c_void_p, fp, C.c_int, fp]
    lib.harmonicRatioObj_free.restype, lib.harmonicRatioObj_free.argtypes = None, [C.c_void_p]
    obj = C.c_void_p()
    lib.harmonicRatioObj_new(C.byref(obj), C.byref(C.c_int(SR)), C.byref(C.c_float(low_fre)), C.byref(C.c_int(r)), None, C.byref(C.c_int(hop)))
    x = np.ascontiguousarray(x, np.float32)
    T = lib.harmonicRatioObj_calTimeLength(obj, len(x))
    out = np.zeros(T, np.float32)
    t0 = time.perf_counter()
    lib.harmonicRatioObj_harmonicRatio(obj, x.ctypes.data_as(fp), len(x), out.ctypes.data_as(fp))
    dt = time.perf_counter() - t0
    lib.harmonicRatioObj_free(obj)
    return T / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--window", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmonic_ratio_mi355x.txt"))
    a = ap.parse_args()
    import torch

    import audioflux_amd as af
    out = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    n = int(SR * a.seconds)
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / SR
    f0 = 80.0 + 800.0 * torch.rand((a.clips, 1), device="cuda", generator=g)
    x = 0.4 * torch.sin(2 * torch.pi * f0 * t) + 0.2 * torch.sin(4 * torch.pi * f0 * t)
    x += 0.01 * torch.randn((a.clips, n), device="cuda", generator=g)
    dc = (0.4 + 0.3 * torch.sin(2 * torch.pi * 60.0 * t)).repeat(a.clips, 1).contiguous()
    del t
    for N in a.window:
        r = N.bit_length() - 1
        o = af.HarmonicRatio(samplate=SR, radix2_exp=r, slide_length=N // 4)
        ncf = af.PitchNCF(samplate=SR, radix2_exp=r, slide_length=N // 4)
        frames = a.clips * o.cal_time_length(n)
        assert frames == a.clips * ncf.cal_time_length(n)
        nmed, nbest = timed(lambda: ncf.pitch_batch_device(x), a.iters)
        nfps = frames / nmed * 1e3
        emit({"kind": "PitchNCF", "window": N, "hop": N // 4, "clips": a.clips, "clip_seconds": a.seconds, "frames": frames,
              "ms": round(nmed, 3), "best_ms": round(nbest, 3), "frames_per_s": round(nfps), "transforms_per_frame": "2 x 2N complex"})
        noisy = dc.clone()
        noisy[:, :N] = 0.3 * torch.randn((a.clips, N), device="cuda", generator=g)  # frame 0 finds a crossing, the rest inherit it
        for what, inp in (("harmonic", x), ("dc", dc), ("noise_then_dc", noisy)):
            med, best = timed(lambda: o.harmonic_ratio_batch_device(inp), a.iters)
            first = o.harmonic_ratio_batch_device(inp)[2]
            torch.cuda.synchronize()
            fps = frames / med * 1e3
            emit({"kind": "HarmonicRatio", "input": what, "window": N, "hop": N // 4, "clips": a.clips, "clip_seconds": a.seconds,
                  "frames": frames, "ms": round(med, 3), "best_ms": round(best, 3), "frames_per_s": round(fps),
                  "rate_over_ncf": round(fps / nfps, 3), "max_length": o.max_length,
                  "frames_with_min_index_0": int((first == 0).sum()), "transforms_per_frame": "2 x 2N complex, twice for a frame run again",
                  "hbm_bytes_in_per_frame": N, "hbm_bytes_out_per_frame": 12, "scratch_bytes_per_frame": 8})
        rate = reference_rate(x[0].cpu().numpy(), r, N // 4, o.low_fre)
        if rate:
            emit({"kind": "reference, one CPU thread", "window": N, "hop": N // 4, "clips": 1, "clip_seconds": a.seconds,
                  "frames_per_s": round(rate)})
        del o, ncf, noisy


if __name__ == "__main__":
    main()
