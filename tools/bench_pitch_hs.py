#!/usr/bin/env python3
"""HPS / LHS pitch tracking, device-resident in and out (pitchHPSObj_pitchBatchDevice / pitchLHSObj_pitchBatchDevice),
hipEvent timing: clips x seconds @ 32 kHz at n_fft 1024 / 2048 / 4096 (hop n_fft / 4, Hamm, 5 harmonics, 32 ... 2000 Hz),
frequency and value out.  Warm-up, then the median of `--iters` timed calls.  Each line carries the per-frame accounting:
transforms of n_fft points, HBM bytes in (4 * hop: neighbouring frames overlap in L2) and out.

    python tools/bench_pitch_hs.py [--clips 200] [--seconds 30] [--iters 10] [--nfft 1024 2048 4096]
    python tools/bench_pitch_hs.py --reference     # the compiled reference (oracle/_ref) on one clip: no GPU touched
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 32000


def reference_time(seconds):
    from oracle import ref
    from tests import pitch_hs_cases as hc
    from tests.pitch_cases import signal
    if not ref.available():
        print(json.dumps({"reference": None, "reason": "oracle/_ref is not built"}))
        return
    lib = hc.bind(ref.lib())
    x = signal("stack:196", int(SR * seconds), SR, seed=1)
    for kind in (hc.HPS, hc.LHS):
        for r in (10, 11, 12):
            N = 1 << r
            st, obj = hc.new(lib, kind, SR, 32.0, 2000.0, r, N // 4, hc.HAMM, 5)
            t0 = time.perf_counter()
            hc.call(lib, kind, obj, x)
            dt = time.perf_counter() - t0
            hc.free(lib, kind, obj)
            frames = (len(x) - N) // (N // 4) + 1
            print(json.dumps({"reference": hc.KIND_NAME[kind], "n_fft": N, "clip_seconds": seconds, "frames": frames,
                              "ms": round(dt * 1e3, 1), "frames_per_s": round(frames / dt)}), flush=True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nfft", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    if a.reference:
        return reference_time(a.seconds)
    import torch

    import audioflux_amd as af
    n = int(SR * a.seconds)
    # harmonic clips with a different f0 each plus a little noise
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / SR
    f0 = 80.0 + 800.0 * torch.rand((a.clips, 1), device="cuda", generator=g)
    x = 0.4 * torch.sin(2 * torch.pi * f0 * t) + 0.2 * torch.sin(4 * torch.pi * f0 * t)
    x += 0.01 * torch.randn((a.clips, n), device="cuda", generator=g)
    del t
    for cls in (af.PitchHPS, af.PitchLHS):
        for nfft in a.nfft:
            r = nfft.bit_length() - 1
            o = cls(samplate=SR, radix2_exp=r, slide_length=nfft // 4)
            frames = a.clips * o.cal_time_length(n)
            med, best = timed(lambda: o.pitch_batch_device(x), a.iters)
            d = o.interp_length // nfft
            print(json.dumps({"kind": cls.__name__, "n_fft": nfft, "hop": nfft // 4, "clips": a.clips, "clip_seconds": a.seconds,
                              "frames": frames, "pitch_ms": round(med, 3), "best_ms": round(best, 3),
                              "frames_per_s": round(frames / med * 1e3), "transforms_per_frame": 1 if d == 1 else d // 2 + 1,
                              "hbm_bytes_in_per_frame": nfft, "hbm_bytes_out_per_frame": 8,
                              "bins_kept": o.max_index * o.harmonic_count + 1}), flush=True)
            del o


if __name__ == "__main__":
    main()
