#!/usr/bin/env python3
"""NSGT throughput on one device: num 84, radix2_exp 15, 32 kHz, octave scale from C1, Slaney windows, BandWidth
normalisation (the reference wrapper's defaults at 2^15), 256 chunks resident on the device.

Timed region: nsgtObj_nsgtBatchDevice between two device events (hipEvent through torch.cuda.Event), 3 warm-ups, median
of 10 runs; with and without the cell planes.  Reported: chunks/s, the algorithmic bytes per chunk 4 N + 8 num maxLength
(+ 8 totalLength with the cells) against the 6.3 TB/s of HBM -- what a kernel that touched memory once would need --, the
float32 work of the direct per-band DFTs (8 sum L^2 flop per chunk) against the vector peak, and the compiled reference's
chunks/s for the same configuration on the same machine, one process, where it is present.

    python tools/bench_nsgt.py [--chunks 256] [--runs 10] [--ref-chunks 3]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS, VECTOR_FLOPS = 6.3e12, 157.3e12  # MI355X: HBM3E bandwidth, float32 vector peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-chunks", type=int, default=3)
    a = ap.parse_args()
    import torch

    import audioflux_amd as af
    num, r, sr = 84, 15, 32000
    N = 1 << r
    o = af.NSGT(num=num, radix2_exp=r, samplate=sr, low_fre=32.703, bin_per_octave=12,
                scale_type=af.SpectralFilterBankScaleType.OCTAVE, style_type=af.SpectralFilterBankStyleType.SLANEY,
                normal_type=af.SpectralFilterBankNormalType.BAND_WIDTH)
    mx, tot, lens = o.get_max_time_length(), o.get_total_time_length(), o.get_time_length_arr().astype(np.int64)
    x = (0.1 * np.random.default_rng(0).standard_normal((a.chunks, N))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    re = torch.empty((a.chunks, num, mx), dtype=torch.float32, device="cuda")
    im = torch.empty_like(re)
    print(f"NSGT num {num}, N 2^{r}, {sr} Hz, octave / Slaney / BandWidth: lengths {lens.min()} ... {lens.max()}, "
          f"{len(set(lens.tolist()))} distinct, maxLength {mx}, totalLength {tot}; {a.chunks} chunks on {torch.cuda.get_device_name(0)}")
    flop = 8.0 * float((lens * lens).sum())
    for cells in (False, True):
        ms = []
        for i in range(a.warmup + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o.nsgt_device(xd, out_real=re, out_imag=im, cells=cells)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        t = statistics.median(ms) * 1e-3
        per = 4 * N + 8 * num * mx + (8 * tot if cells else 0)
        rate = a.chunks / t
        print(f"cells {'on ' if cells else 'off'}: median {t * 1e3:.3f} ms of {a.runs} runs (min {min(ms):.3f}, max {max(ms):.3f}) -> "
              f"{rate:,.0f} chunks/s; {per} algorithmic bytes per chunk -> {rate * per / 1e9:.1f} GB/s = "
              f"{100 * rate * per / HBM_BPS:.2f} % of 6.3 TB/s; direct DFTs {flop / 1e6:.2f} Mflop per chunk -> "
              f"{rate * flop / 1e12:.2f} Tflop/s = {100 * rate * flop / VECTOR_FLOPS:.1f} % of the float32 vector peak")
    from oracle import ref
    if ref.available():
        from tests import nsgt_cases as nc
        from tests.golden import make_nsgt_golden as mk
        L = mk.bind(ref.lib())
        c = nc.by_name("oct84")
        st, obj = mk.ref_new(L, c)
        assert st == 0
        mk.ref_transform(L, obj, x[0], num, mx, tot)
        t0 = time.perf_counter()
        for q in range(a.ref_chunks):
            mk.ref_transform(L, obj, x[q % a.chunks], num, mx, tot)
        dt = (time.perf_counter() - t0) / a.ref_chunks
        L.nsgtObj_free(obj)
        print(f"compiled reference, same configuration, one process on this machine's CPU: {dt * 1e3:.1f} ms per chunk -> "
              f"{1 / dt:,.1f} chunks/s")
    else:
        print("compiled reference: not present on this machine")


if __name__ == "__main__":
    main()
