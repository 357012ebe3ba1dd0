#!/usr/bin/env python3
"""Harmonic / percussive separation, device-resident in and out (hpssObj_hpssBatchDevice / hpssObj_spectraBatchDevice),
hipEvent timing: clips x seconds @ 16 kHz at n_fft 1024 / 2048 / 4096, orders 21 / 31, with the parts timed on their own
objects (forward STFT, the separation kernel = spectra call - forward, the two inverses).

    python tools/bench_hpss.py [--clips 1000] [--seconds 30] [--iters 10] [--chunk-mb M] [--nfft 1024 2048 4096]
    python tools/bench_hpss.py --reference     # the compiled reference (oracle/_ref) on one 30 s clip: no GPU touched
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_time(seconds):
    from oracle import ref
    from tests import hpss_cases as hc
    from tests.golden.make_hpss_golden import bind, run
    if not ref.available():
        print(json.dumps({"reference": None, "reason": "oracle/_ref is not built"}))
        return
    lib = ref.lib()
    bind(lib)
    x = hc.signal("mix", int(16000 * seconds), seed=1)
    for r in (10, 11, 12):
        t0 = time.perf_counter()
        run(lib, x, r, hc.HAMM, 21, 31)
        dt = time.perf_counter() - t0
        frames = (len(x) - (1 << r)) // ((1 << r) // 4) + 1
        print(json.dumps({"reference_n_fft": 1 << r, "clip_seconds": seconds, "frames": frames, "ms": round(dt * 1e3, 1),
                          "frames_per_s": round(frames / dt)}))


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
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk-mb", type=int, default=0)
    ap.add_argument("--nfft", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    if a.reference:
        return reference_time(a.seconds)
    if a.chunk_mb:
        os.environ["AFX_HPSS_CHUNK_MB"] = str(a.chunk_mb)
    import torch

    import audioflux_amd as af
    n = int(16000 * a.seconds)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = 0.1 * torch.randn((a.clips, n), device="cuda", generator=g)
    for nfft in a.nfft:
        r = nfft.bit_length() - 1
        o = af.HPSS(radix2_exp=r)
        st = af.STFT(radix2_exp=r, window_type=af.WindowType.HAMM, slide_length=nfft // 4)
        frames = a.clips * o.cal_time_length(n)
        m = o.cal_data_length(n)
        h = torch.zeros((a.clips, m), device="cuda")
        p = torch.zeros_like(h)
        s = torch.cuda.current_stream().cuda_stream
        fn = o._lib.hpssObj_hpssBatchDevice
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]

        def both():
            assert fn(o._obj, x.data_ptr(), a.clips, n, x.stride(0), h.data_ptr(), p.data_ptr(), m, s) == 0

        def one():
            assert fn(o._obj, x.data_ptr(), a.clips, n, x.stride(0), h.data_ptr(), None, m, s) == 0

        med, best = timed(both, a.iters)
        med1, _ = timed(one, a.iters)
        spec, _ = timed(lambda: o.spectra_device(x), a.iters)
        # parts on a chunk-sized batch (the full spectra of 1000 clips do not fit next to the batch): scaled to the batch
        sub = max(1, min(a.clips, 16))
        xs = x[:sub].contiguous()
        fwd, _ = timed(lambda: st.stft_device(xs), a.iters)
        re, im = st.stft_device(xs)
        inv, _ = timed(lambda: st.istft_device(re, im), a.iters)
        k = a.clips / sub
        print(json.dumps({"n_fft": nfft, "orders": [21, 31], "clips": a.clips, "frames": frames, "chunk_mb": a.chunk_mb or 1024,
                          "hpss_two_outputs_ms": round(med, 3), "best_ms": round(best, 3), "frames_per_s": round(frames / med * 1e3),
                          "hpss_one_output_ms": round(med1, 3), "spectra_only_ms": round(spec, 3),
                          "parts_scaled_from_%d_clips" % sub: {"stft_full_spectrum_ms": round(fwd * k, 3),
                                                               "one_istft_ms": round(inv * k, 3)}}), flush=True)
        del o, st, h, p, re, im


if __name__ == "__main__":
    main()
