#!/usr/bin/env python3
"""PEF pitch tracking, device-resident in and out (pitchPEFObj_pitchBatchDevice), hipEvent timing: clips x seconds @ 32 kHz
at n_fft 1024 / 2048 / 4096 (hop n_fft / 4, Hamm, 32 ... 2000 Hz, cutFre 4000, alpha 10, beta 0.5, gamma 1.8), frequency and
value out.  Warm-up, then the median of `--iters` timed calls.  Per frame the kernel runs ONE n_fft-point and TWO
2 n_fft-point complex transforms in LDS: transforms/s below counts those three, next to YIN's two n_fft-point transforms per
frame (profiles/pitch_yin_bench_mi355x.txt).  The compiled reference (oracle/_ref, when built) runs one clip on one CPU
thread of the same machine.  Every line is printed and appended to --out.

    python tools/bench_pitch_pef.py [--clips 200] [--seconds 30] [--iters 10] [--nfft 1024 2048 4096]
                                    [--out profiles/pitch_pef_mi355x.txt] [--reference-seconds 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 32000


def yin_transforms_per_s():
    """n_fft -> YIN's measured transforms/s (2 per frame), from its profile"""
    out = {}
    path = os.path.join(ROOT, "profiles", "pitch_yin_bench_mi355x.txt")
    if os.path.exists(path):
        for line in open(path):
            if line.startswith('{"n_fft"'):
                d = json.loads(line)
                out[d["n_fft"]] = 2 * d["frames_per_s"]
    return out


def reference_lines(seconds, nffts):
    from oracle import ref
    from tests import pitch_pef_cases as pc
    from tests.pitch_cases import signal
    if not ref.available():
        return [{"reference": None, "reason": "oracle/_ref is not built"}]
    lib = pc.bind(ref.lib())
    x = signal("stack:196", int(SR * seconds), SR, seed=1)
    lines = []
    for nfft in nffts:
        r = nfft.bit_length() - 1
        st, obj = pc.new(lib, SR, None, None, None, r, nfft // 4)
        t0 = time.perf_counter()
        pc.call(lib, obj, x)
        dt = time.perf_counter() - t0
        lib.pitchPEFObj_free(obj)
        frames = (len(x) - nfft) // (nfft // 4) + 1
        lines.append({"reference": "PEF", "n_fft": nfft, "clip_seconds": seconds, "frames": frames, "ms": round(dt * 1e3, 1),
                      "frames_per_s": round(frames / dt), "transforms_per_frame": "1 x 2N + 3 x 8N real, one CPU thread"})
    return lines


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_pef_mi355x.txt"))
    ap.add_argument("--reference-seconds", type=float, default=10.0)
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
    yin = yin_transforms_per_s()
    for nfft in a.nfft:
        r = nfft.bit_length() - 1
        o = af.PitchPEF(samplate=SR, radix2_exp=r, slide_length=nfft // 4)
        frames = a.clips * o.cal_time_length(n)
        med, best = timed(lambda: o.pitch_batch_device(x), a.iters)
        fps = frames / med * 1e3
        # one N-point and two 2N-point complex transforms per frame; in N-point units (n log n): 1 + 2 * 2 * (r + 1) / r
        emit({"kind": "PitchPEF", "n_fft": nfft, "hop": nfft // 4, "clips": a.clips, "clip_seconds": a.seconds, "frames": frames,
              "pitch_ms": round(med, 3), "best_ms": round(best, 3), "frames_per_s": round(fps),
              "transforms_per_frame": "1 x N + 2 x 2N complex", "transforms_per_s": round(3 * fps),
              "n_point_equivalents_per_s": round((1 + 4 * (r + 1) / r) * fps), "yin_transforms_per_s": yin.get(nfft),
              "min_index": o.min_index, "max_index": o.max_index, "filter_pad_num": o.filter_pad_num,
              "hbm_bytes_in_per_frame": nfft, "hbm_bytes_out_per_frame": 8})
        del o
    for d in reference_lines(a.reference_seconds, a.nfft):
        emit(d)


if __name__ == "__main__":
    main()
