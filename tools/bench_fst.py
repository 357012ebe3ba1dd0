#!/usr/bin/env python3
"""FST throughput on one device, chunks resident in HBM.

Timed region: fstObj_fstBatchDevice between two device events (hipEvent through torch.cuda.Event), 3 warm-ups, median of 10
runs, for
  2^12 samples, rows 0 ... 2048 (the full range), matrix form;
  2^14 samples, rows 1 ... 2048, matrix form;
  both sizes in the cells-only form (spectrum + cells, no matrix).
Reported: chunks/s and the algorithmic bytes per chunk -- 4 N + 8 rows N with the matrix, 4 N + 8 (N/2 + 1) with the cells
only: what a kernel that touched memory once would need -- against the 6.3 TB/s a float4 copy reaches on the device.  The
split: the cells-only form of the same batch is the forward pass + k_fst_cells; the matrix form minus that is k_fst_expand
(the launches of a call run back to back on one stream).  A kernel trace gives the split per kernel name.

    python tools/bench_fst.py [--runs 10] [--warmup 3]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 6.3e12  # MI355X: what a float4 copy reaches


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
    import ctypes as C

    import torch

    import audioflux_amd as af
    print(f"FST on {torch.cuda.get_device_name(0)}: device events around fstObj_fstBatchDevice, {a.warmup} warm-ups, median of {a.runs}")
    for r, lo, hi, chunks, cell_chunks in ((12, 0, 2048, 16, 4096), (14, 1, 2048, 4, 1024)):
        N, rows = 1 << r, hi - lo + 1
        o = af.FST(radix2_exp=r)
        fn = o._lib.fstObj_fstBatchDevice
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 5
        x = torch.from_numpy((0.1 * np.random.default_rng(r).standard_normal((cell_chunks, N))).astype(np.float32)).cuda()
        re = torch.empty((chunks, rows, N), dtype=torch.float32, device="cuda")
        im = torch.empty_like(re)
        cre = torch.empty((cell_chunks, N // 2 + 1), dtype=torch.float32, device="cuda")
        cim = torch.empty_like(cre)
        s = torch.cuda.current_stream().cuda_stream

        def call(n, matrix, cells):
            st = fn(o._obj, x.data_ptr(), n, N, lo, hi, re.data_ptr() if matrix else None, im.data_ptr() if matrix else None,
                    cre.data_ptr() if cells else None, cim.data_ptr() if cells else None, s)
            assert st == 0, af.last_error()

        t_m, lo_m, hi_m = timed(lambda: call(chunks, True, False), a.warmup, a.runs)
        t_s, _, _ = timed(lambda: call(chunks, False, True), a.warmup, a.runs)
        t_c, lo_c, hi_c = timed(lambda: call(cell_chunks, False, True), a.warmup, a.runs)
        per_m, per_c = 4 * N + 8 * rows * N, 4 * N + 8 * (N // 2 + 1)
        print(f"2^{r}, rows {lo} ... {hi}, {chunks} chunks, matrix: median {t_m * 1e3:.3f} ms (min {lo_m:.3f}, max {hi_m:.3f}) -> "
              f"{chunks / t_m:,.0f} chunks/s; {per_m} algorithmic bytes per chunk -> {chunks * per_m / t_m / 1e9:.0f} GB/s = "
              f"{100 * chunks * per_m / t_m / HBM_BPS:.1f} % of 6.3 TB/s")
        print(f"    split: forward pass + k_fst_cells of the same {chunks} chunks {t_s * 1e3:.3f} ms; k_fst_expand (the rest) "
              f"{(t_m - t_s) * 1e3:.3f} ms -> {chunks * 8 * rows * N / max(t_m - t_s, 1e-9) / 1e9:.0f} GB/s of stores = "
              f"{100 * chunks * 8 * rows * N / max(t_m - t_s, 1e-9) / HBM_BPS:.1f} % of 6.3 TB/s")
        print(f"2^{r}, {cell_chunks} chunks, cells only: median {t_c * 1e3:.3f} ms (min {lo_c:.3f}, max {hi_c:.3f}) -> "
              f"{cell_chunks / t_c:,.0f} chunks/s; {per_c} algorithmic bytes per chunk -> {cell_chunks * per_c / t_c / 1e9:.0f} GB/s = "
              f"{100 * cell_chunks * per_c / t_c / HBM_BPS:.1f} % of 6.3 TB/s")
        del o, re, im


if __name__ == "__main__":
    main()
