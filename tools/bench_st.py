#!/usr/bin/env python3
"""ST throughput on one device, chunks and results resident in HBM.

Timed region: stObj_stBatchDevice between two device events (hipEvent through torch.cuda.Event), 3 warm-ups, median of 10
runs, for
  2^12 samples, rows 1 ... 2047 (the wrapper's default range), 16 chunks;
  2^14 samples, rows 1 ... 2048, 4 chunks.
Each time is set against two floors taken from the project's other profiles, not from this code:
  stores  -- the 8 rows N output bytes of a chunk at the 6.3 TB/s a float4 copy reaches (profiles/fst_mi355x.txt);
  LDS FFT -- one N-point transform per row at the rate the same LDS routine reaches per transform in the pitch trackers
             (profiles/pitch_yin_bench_mi355x.txt: 51 M 4096-point transforms/s; profiles/pitch_hs_mi355x.txt: 37 M/s).  There is
             no measured rate for 2^14 points: the 4096-point rate scaled by N log2 N is printed as an estimate, not a floor.
The forward pass of the same chunks is timed on its own by a one-row object (row 0 is a broadcast, no transform).

    python tools/bench_st.py [--runs 10] [--warmup 3]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 6.3e12          # MI355X: what a float4 copy reaches (profiles/fst_mi355x.txt)
FFT4096_YIN = 51e6        # 4096-point LDS transforms/s, profiles/pitch_yin_bench_mi355x.txt
FFT4096_HPS = 37e6        # the same, profiles/pitch_hs_mi355x.txt


def timed(fn, warmup, runs):
    import torch
    ms = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) * 1e-3, min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert a.runs >= 10 and a.warmup >= 3
    import torch

    import audioflux_amd as af
    print(f"ST on {torch.cuda.get_device_name(0)}: device events around stObj_stBatchDevice, {a.warmup} warm-ups, median of {a.runs}")
    for r, lo, hi, chunks in ((12, 1, 2047, 16), (14, 1, 2048, 4)):
        N, rows = 1 << r, hi - lo + 1
        o = af.ST(radix2_exp=r, min_index=lo, max_index=hi)
        x = torch.from_numpy((0.1 * np.random.default_rng(r).standard_normal((chunks, N))).astype(np.float32)).cuda()
        s = torch.cuda.current_stream()
        re, im = o.st_device(x, stream=s)
        t, t_lo, t_hi = timed(lambda: o.st_device(x, out_real=re, out_imag=im, stream=s), a.warmup, a.runs)
        one = af.ST(radix2_exp=r, min_index=lo, max_index=hi)
        one.use_bin_arr([0])
        re1, im1 = one.st_device(x, stream=s)
        t_f, _, _ = timed(lambda: one.st_device(x, out_real=re1, out_imag=im1, stream=s), a.warmup, a.runs)
        out_bytes, transforms = 8 * rows * N * chunks, rows * chunks
        scale = (4096 * 12) / (N * r)
        kind = "floor" if r == 12 else "estimate: the 4096-point rate scaled by N log2 N, no profile has 2^14"
        print(f"2^{r}, rows {lo} ... {hi}, {chunks} chunks: median {t * 1e3:.3f} ms (min {t_lo:.3f}, max {t_hi:.3f}) -> "
              f"{chunks / t:,.0f} chunks/s, {transforms / t / 1e6:.1f} M rows/s, {out_bytes / t / 1e9:.0f} GB/s of stores")
        print(f"    stores floor: {out_bytes} bytes at 6.3 TB/s = {out_bytes / HBM_BPS * 1e3:.3f} ms -> the call is at "
              f"{100 * out_bytes / HBM_BPS / t:.1f} % of it")
        print(f"    LDS-FFT {kind}: {transforms} transforms at {FFT4096_YIN * scale / 1e6:.1f} M/s (YIN) = "
              f"{transforms / (FFT4096_YIN * scale) * 1e3:.3f} ms, at {FFT4096_HPS * scale / 1e6:.1f} M/s (HPS) = "
              f"{transforms / (FFT4096_HPS * scale) * 1e3:.3f} ms")
        print(f"    forward pass + one broadcast row of the same {chunks} chunks: {t_f * 1e3:.3f} ms")
        del o, one, re, im, re1, im1


if __name__ == "__main__":
    main()
