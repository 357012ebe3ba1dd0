#!/usr/bin/env python3
"""NCF and cepstrum pitch tracking, device-resident in and out (pitchNCFObj_pitchBatchDevice, pitchCEPObj_pitchBatchDevice),
hipEvent timing: clips x seconds @ 32 kHz at n_fft 1024 / 2048 / 4096 (hop n_fft / 4, 32 ... 2000 Hz, each tracker's default
window), frequency and value out.  Warm-up, then the median of `--iters` timed calls.  Per frame the kernel runs TWO
2 n_fft-point complex transforms in LDS.  PitchYIN (two n_fft-point transforms per frame, auto_length n_fft / 2) runs on the
same clips in the same process as the nearest relative.  Every line is printed and appended to --out.

    python tools/bench_pitch_lag.py [--clips 200] [--seconds 30] [--iters 10] [--nfft 1024 2048 4096]
                                    [--out profiles/pitch_lag_mi355x.txt]
"""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nfft", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_lag_mi355x.txt"))
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
    # harmonic clips with a different f0 each plus a little noise
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / SR
    f0 = 80.0 + 800.0 * torch.rand((a.clips, 1), device="cuda", generator=g)
    x = 0.4 * torch.sin(2 * torch.pi * f0 * t) + 0.2 * torch.sin(4 * torch.pi * f0 * t)
    x += 0.01 * torch.randn((a.clips, n), device="cuda", generator=g)
    del t
    for nfft in a.nfft:
        r = nfft.bit_length() - 1
        for kind, cls in (("PitchNCF", af.PitchNCF), ("PitchCEP", af.PitchCEP)):
            o = cls(samplate=SR, radix2_exp=r, slide_length=nfft // 4)
            frames = a.clips * o.cal_time_length(n)
            med, best = timed(lambda: o.pitch_batch_device(x), a.iters)
            fps = frames / med * 1e3
            # two 2N-point complex transforms per frame; in N-point units (n log n): 2 * 2 * (r + 1) / r
            emit({"kind": kind, "n_fft": nfft, "hop": nfft // 4, "clips": a.clips, "clip_seconds": a.seconds, "frames": frames,
                  "pitch_ms": round(med, 3), "best_ms": round(best, 3), "frames_per_s": round(fps),
                  "transforms_per_frame": "2 x 2N complex", "transforms_per_s": round(2 * fps),
                  "n_point_equivalents_per_s": round(4 * (r + 1) / r * fps), "min_index": o.min_index, "max_index": o.max_index,
                  "window_type": int(o.window_type), "hbm_bytes_in_per_frame": nfft, "hbm_bytes_out_per_frame": 8})
            del o
        y = af.PitchYIN(samplate=SR, radix2_exp=r, slide_length=nfft // 4, auto_length=nfft // 2)
        frames = a.clips * y.cal_time_length(n)
        med, best = timed(lambda: y.pitch_device(x), a.iters)
        fps = frames / med * 1e3
        emit({"kind": "PitchYIN", "n_fft": nfft, "hop": nfft // 4, "clips": a.clips, "clip_seconds": a.seconds, "frames": frames,
              "pitch_ms": round(med, 3), "best_ms": round(best, 3), "frames_per_s": round(fps), "transforms_per_frame": "2 x N complex",
              "transforms_per_s": round(2 * fps), "n_point_equivalents_per_s": round(2 * fps)})
        del y


if __name__ == "__main__":
    main()
