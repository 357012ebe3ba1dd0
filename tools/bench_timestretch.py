#!/usr/bin/env python3
"""Time stretch and pitch shift, device-resident in and out (timeStretchObj_timeStretchBatchDevice,
pitchShiftObj_pitchShiftBatchDevice), hipEvent timing: `--clips` x `--seconds` clips at 44.1 kHz and ONE such clip, n_fft 4096 /
hop 1024, time stretch at rates 0.8 and 1.25, pitch shift at +4 semitones.  Warm-up, then the median of `--iters` timed calls.
Next to each: the compiled reference (oracle/_ref/libaudioflux_ref.so, when present) on ONE clip and one CPU thread of the same
machine, and the bytes every stage of a call moves, computed from the shapes (stage_mb: forward STFT, the vocoder's three
kernels, inverse STFT, row copy, and for the pitch shift the resampler and its row copy).  Every line is printed and appended
to --out.

The per-kernel split comes from runs of their own under the profiler, one configuration each:
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_timestretch.py --once --case stretch:0.8:1000
makes `--calls` untimed calls of that configuration and nothing else; then
    python tools/bench_timestretch.py --split DIR/NAME_results.db --case stretch:0.8:1000
sums the trace per kernel and appends one "kernels" line: launches and ms per call, and per stage its bytes over its time.

    python tools/bench_timestretch.py [--clips 1000] [--seconds 30] [--iters 5] [--scratch-gb G] [--out profiles/timestretch_mi355x.txt]
                                      [--case kind:arg:clips] [--once [--calls 3]] [--split DB]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref", "libaudioflux_ref.so")
EXP, HOP, RATE_HZ = 12, 1024, 44100
CASES = (("stretch", 0.8), ("stretch", 1.25), ("shift", 4))


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


def reference_seconds(kind, arg, x):
    """one clip through the compiled reference on this thread: seconds (best of two), or None without the library"""
    if not os.path.exists(REF):
        return None
    import numpy as np
    from tests import timestretch_cases as tc
    lib = tc.ref_lib()
    c = dict(exp=EXP, hop=HOP)
    st, obj = tc.new(lib, c, "timeStretch" if kind == "stretch" else "pitchShift")
    best = None
    for _ in range(2):
        if kind == "stretch":
            out = np.zeros(lib.timeStretchObj_calDataCapacity(obj, C.c_float(arg), len(x)), np.float32)
            t0 = time.perf_counter()
            lib.timeStretchObj_timeStretch(obj, C.c_float(arg), tc.ptr(x), len(x), tc.ptr(out))
        else:
            out = np.zeros(len(x) + 8, np.float32)
            t0 = time.perf_counter()
            lib.pitchShiftObj_pitchShift(obj, RATE_HZ, arg, tc.ptr(x), len(x), tc.ptr(out))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    (lib.timeStretchObj_free if kind == "stretch" else lib.pitchShiftObj__free)(obj)
    return best


def stage_mb(p, n, clips, resampled=None):
    """MB each stage of one call reads + writes, from the shapes alone (every word counted once per kernel that touches it;
    the phase kernel's two angle reads per output frame mostly hit the L2)"""
    N = p.fftLength
    F = N // 2 + 1
    f = 4e-6 * clips
    d = {"stft": f * (n + 2 * p.T1 * F), "polar": f * 4 * p.T1 * F, "phase": f * (2 * p.T2 * F + p.T2 * F),
         "synthesis": f * (2 * p.T2 * F + p.T2 * F + 2 * p.T2 * N), "istft": f * (2 * p.T2 * N + 2 * p.istftLength),
         "rows": f * (min(p.istftLength, p.returnLength) + p.returnLength)}
    if resampled is not None:
        d["resample"] = f * (p.returnLength + resampled)
        d["rows_out"] = f * 2 * min(n, resampled)
    return {k: round(v, 1) for k, v in d.items()}


# kernel name -> the stage of stage_mb whose bytes it moves
STAGE_OF = (("k_stft", "stft"), ("k_pv_polar", "polar"), ("k_pv_phase", "phase"), ("k_pv_synthesis", "synthesis"), ("k_istft", "istft"),
            ("k_rows_fit", "rows"), ("k_resample", "resample"), ("fillBuffer", "memset"), ("copyBuffer", "copies"))


def split(db, calls, mb):
    """per stage of one call, from a kernel trace of `calls` calls: launches, ms, and the stage's MB over its ms"""
    import sqlite3
    con = sqlite3.connect(db)
    acc = {}
    for name, dur in con.execute("select name, duration from kernels"):
        stage = next((s for key, s in STAGE_OF if key in name), None)
        if stage is None:
            continue  # (the framework's own kernels: filling the input)
        a = acc.setdefault(stage, [0, 0.0])
        a[0] += 1
        a[1] += dur * 1e-6
    if "rows_out" in mb:  # the pitch shift's second row copy runs the same kernel
        mb = dict(mb, rows=mb["rows"] + mb["rows_out"])
    out = {}
    for stage, (launches, ms) in acc.items():
        out[stage] = {"launches": round(launches / calls, 1), "ms": round(ms / calls, 3)}
        if stage in mb and ms > 0:
            out[stage]["mb"] = mb[stage]
            out[stage]["gb_per_s"] = round(mb[stage] / (ms / calls), 1)
    return out, round(sum(v["ms"] for v in out.values()), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--calls", type=int, default=3, help="calls of a --once run")
    ap.add_argument("--case", default=None, help="kind:arg:clips, e.g. stretch:0.8:1000 or shift:4:1: this configuration alone")
    ap.add_argument("--split", default=None, help="kernel-trace database of a --once run of --case: append its per-kernel line")
    ap.add_argument("--scratch-gb", type=float, default=0.0, help="scratch limit of the objects (0: the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timestretch_mi355x.txt"))
    a = ap.parse_args()
    if not a.split:
        import torch  # (before the library: the package shares torch's HIP runtime)

    import audioflux_amd as af
    from tests import timestretch_cases as tc
    if not a.split:
        af.get_lib()
    lib = tc.bind(C.CDLL(af.LIB_PATH))
    out = None if a.once else open(a.out, "a")
    only = None
    if a.case:
        kind, arg, clips = a.case.split(":")
        only = (kind, float(arg) if kind == "stretch" else int(arg), int(clips))

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n = int(RATE_HZ * a.seconds)
    if a.split:  # no device: the trace, and the bytes from the shapes
        assert only, "--split needs --case"
        kind, arg, clips = only
        rate = arg if kind == "stretch" else float(tc.semitone_rate(arg))
        p = tc.Plan()
        assert lib.afx_timestretch_plan(EXP, HOP, C.c_float(rate), n, clips, int(a.scratch_gb * 2 ** 30), C.byref(p), None, None) == 0
        resampled = None if kind == "stretch" else int(math.floor(np.float32(p.returnLength) * np.float32(rate)))
        stages, total = split(a.split, a.calls, stage_mb(p, n, clips, resampled))
        emit({"kind": "kernels", "of": kind, "rate" if kind == "stretch" else "semitones": arg, "clips": clips, "calls_traced": a.calls,
              "kernel_ms_per_call": total, "stages": stages})
        return
    assert torch.cuda.is_available(), "needs an MI355X"
    for clips in sorted({a.clips, 1} if not only else {only[2]}, reverse=True):
        g = torch.Generator(device="cuda").manual_seed(0)
        x = 0.5 * torch.randn((clips, n), device="cuda", generator=g)
        for kind, arg in (CASES if not only else (only[:2],)):
            rate = arg if kind == "stretch" else float(tc.semitone_rate(arg))
            p = tc.Plan()
            assert lib.afx_timestretch_plan(EXP, HOP, C.c_float(rate), n, clips, int(a.scratch_gb * 2 ** 30), C.byref(p), None, None) == 0
            if kind == "stretch":
                o = af.TimeStretch(EXP, HOP)
                o.set_scratch_limit(int(a.scratch_gb * 2 ** 30))
                y = torch.empty((clips, p.returnLength), dtype=torch.float32, device="cuda")
                fn = lambda: o.time_stretch_batch_device(x, arg, out=y)  # noqa: E731
                written, resampled = p.returnLength, None
            else:
                o = af.PitchShift(EXP, HOP)
                o.set_scratch_limit(int(a.scratch_gb * 2 ** 30))
                y = torch.empty((clips, n), dtype=torch.float32, device="cuda")
                fn = lambda: o.pitch_shift_batch_device(x, arg, out=y)  # noqa: E731
                written = resampled = fn().shape[1]  # (a call of its own: a --once run counts it)
            if a.once:
                for _ in range(a.calls - (kind == "shift")):
                    fn()
                torch.cuda.synchronize()
                emit({"kind": kind, "arg": arg, "clips": clips, "once": True})
                continue
            med, best = timed(fn, a.iters)
            d = {"kind": kind, "rate" if kind == "stretch" else "semitones": arg, "clips": clips, "clip_seconds": a.seconds, "samples_in": n,
                 "samples_out": written, "frames_in": p.T1, "frames_out": p.T2, "call_ms": round(med, 3), "best_ms": round(best, 3),
                 "clip_seconds_per_s": round(clips * a.seconds / med * 1e3), "scratch_limit_gb": a.scratch_gb or 4.0, "scratch_mb_per_clip": round(p.scratchBytes / 1e6, 1),
                 "clips_per_chunk": p.clipsPerChunk, "chunks": -(-clips // p.clipsPerChunk), "stage_mb": stage_mb(p, n, clips, resampled)}
            d["moved_gb_per_s"] = round(sum(d["stage_mb"].values()) / med, 1)
            ref = reference_seconds(kind, arg, x[0].cpu().numpy())
            if ref is not None:
                d["reference_cpu_s_per_clip"] = round(ref, 3)
                d["speedup_vs_one_cpu_thread"] = round(ref * clips / (med * 1e-3))
            emit(d)
            del y, o
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
