#!/usr/bin/env python3
"""Resampling, device-resident in and out (resampleObj_resampleBatchDevice), hipEvent timing: `--clips` x `--seconds` clips
44100 -> 16000 and 48000 -> 16000 at Best and Fast, and 16000 -> 44100 at Best.  Warm-up, then the median of `--iters` timed
calls.  Next to each: the compiled reference (oracle/_ref/libaudioflux_ref.so, when present) on ONE clip and one CPU thread
of the same machine, and the kernel's LDS-read bound -- taps per output x (2 table reads / clips per work item + 1 sample
read) x outputs / the ds_read_b32 rate that `--lds-bin` (tools/micro/lds_read_b32_rate.hip, built beforehand) measures in the
same run, conflict-free and with the kernel's own address patterns.  Every line is printed and appended to --out.

    python tools/bench_resample.py [--clips 1000] [--seconds 30] [--iters 5] [--lds-bin PATH] [--out profiles/resample_mi355x.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref", "libaudioflux_ref.so")
CASES = (("best", 44100, 16000), ("fast", 44100, 16000), ("best", 48000, 16000), ("fast", 48000, 16000), ("best", 16000, 44100))
QUAL = {"best": 0, "mid": 1, "fast": 2}
ZEROS = {"best": 64, "mid": 32, "fast": 16}


def timed(fn, iters, warmup=2):
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


def reference_seconds(qual, src, tgt, x):
    """one clip through the compiled reference on this thread: seconds, or None without the library"""
    if not os.path.exists(REF):
        return None
    import numpy as np
    lib = C.CDLL(REF)
    obj = C.c_void_p(None)
    lib.resampleObj_new(C.byref(obj), C.pointer(C.c_int(QUAL[qual])), None, None)
    lib.resampleObj_setSamplate.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.resampleObj_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.resampleObj_free.argtypes = [C.c_void_p]
    lib.resampleObj_setSamplate(obj, src, tgt)
    best = None
    for _ in range(2):
        out = np.zeros(int(len(x) * max(1.0, tgt / src)) + 16, np.float32)
        t0 = time.perf_counter()
        lib.resampleObj_resample(obj, x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    lib.resampleObj_free(obj)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--lds-bin", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_mi355x.txt"))
    a = ap.parse_args()
    import torch

    import audioflux_amd as af
    out = open(a.out, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    rates = {}
    if a.lds_bin:
        res = subprocess.run([a.lds_bin], capture_output=True, text=True, timeout=120)
        for line in res.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                emit(dict(d, kind="ds_read_b32"))
                rates[d["pattern"]] = max(rates.get(d["pattern"], 0.0), d["g_reads_per_s"] * 1e9)
    for qual, src, tgt in CASES:
        n = int(src * a.seconds)
        g = torch.Generator(device="cuda").manual_seed(0)
        x = 0.5 * torch.randn((a.clips, n), device="cuda", generator=g)
        o = af.Resample(qual, is_scale=False)
        o.set_samplate(src, tgt)
        m = o.cal_data_length(n)
        y = torch.empty((a.clips, m), dtype=torch.float32, device="cuda")
        med, best = timed(lambda: o.resample_batch_device(x, out=y), a.iters)
        ratio = tgt / src
        taps = 2 * int(ZEROS[qual] * 512 // int(min(1.0, ratio) * 512))  # both sides, away from the clip's ends
        group = min(4, a.clips)
        macs = a.clips * m * taps
        reads_table, reads_input = macs * 2 / group, macs
        d = {"kind": "resample", "quality": qual, "source_rate": src, "target_rate": tgt, "clips": a.clips, "clip_seconds": a.seconds,
             "samples_in": n, "samples_out": m, "resample_ms": round(med, 3), "best_ms": round(best, 3),
             "clip_seconds_per_s": round(a.clips * a.seconds / med * 1e3), "out_samples_per_s": round(a.clips * m / med * 1e3),
             "taps_per_output": taps, "gmacs_per_s": round(macs / med / 1e6, 1), "clips_per_work_item": group,
             "hbm_gb_per_s": round(4 * a.clips * (n + m) / med / 1e6, 1)}
        if rates:
            d["lds_bound_ms_conflict_free"] = round((reads_table + reads_input) / rates["linear"] * 1e3, 3)
            d["lds_bound_ms_own_patterns"] = round((reads_table / rates["table"] + reads_input / rates["input"]) * 1e3, 3)
        ref = reference_seconds(qual, src, tgt, x[0].cpu().numpy())
        if ref is not None:
            d["reference_cpu_s_per_clip"] = round(ref, 4)
            d["reference_cpu_s_all_clips"] = round(ref * a.clips, 1)
            d["speedup_vs_one_cpu_thread"] = round(ref * a.clips / (med * 1e-3))
        emit(d)
        del x, y, o
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
