#!/usr/bin/env python3
"""The packed band plan in k_stft_mel_v2 as emulated device code (tests/test_mel_pack_emulated.py), through the plan layer itself
(afxk_melfused_create / _run); the packed plan's output against the plan as it came (AFX_MEL_NOPACK=1 at plan creation), bit
for bit.

  * 3 clips x 37 frames at hop 512: mel-128 + MFCC-13 in one launch, complex results and the temporal instantiation, with the
    grid sized for one CU and for the whole device.  111 frames are fewer than the 16 x 12 = 192 a workgroup needs before a wave
    claims a 16-frame run (claim_length, afx_melfused2.hip): every run has four frames or fewer, starts inside a clip or crosses
    a clip boundary, and its cepstra come from the tail call of the cepstrum block.
  * 3 clips x 301 frames, mel-128 + MFCC-13 on one CU: one workgroup owns all 903 frames, its waves claim runs of 32 and 16
    frames while 192 or more are left -- whole 16-row cepstrum blocks from the call site between the band stage and the row
    stores, where the packed form keeps a third sum alive -- then 4-frame runs and a clamped last one.  The run lengths are
    worked out below with the launcher's and the kernel's own arithmetic and asserted.
  * a packed plan with one continuation flag flipped changes exactly the row concerned.

AFX_LIB = the library tests/test_emulated_kernels.py builds."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import restate  # noqa: E402
from tests import cases  # noqa: E402
from tests.test_bandplan import Band  # noqa: E402

lib = C.CDLL(os.environ["AFX_LIB"])
vp, fp = C.c_void_p, C.POINTER(C.c_float)
lib.afx_emulated_launches.restype = C.c_int
lib.afx_emulated_launches.argtypes = [C.c_char_p]
lib.afxk_melfused_pack.restype = C.c_int
lib.afxk_melfused_pack.argtypes = [vp]


class Args(C.Structure):  # AfxMelFusedArgs, audioflux_amd/csrc/hip/afx_device.h
    _fields_ = [("x", vp), ("clipStride", C.c_longlong), ("batch", C.c_int), ("dataLength", C.c_int), ("timeLength", C.c_int),
                ("hop", C.c_int), ("specMap", C.c_int), ("postPow", C.c_int), ("normValue", C.c_float), ("out", vp), ("outIm", vp),
                ("dct", vp), ("ccNum", C.c_int), ("ccRectify", C.c_int), ("cc", vp), ("energy", vp), ("rms", vp), ("zcr", vp)]


class Plan(C.Structure):  # AfxMelPlan, audioflux_amd/csrc/hip/afx_melplan.h (which points here: keep the two alike)
    _fields_ = [("radix2Exp", C.c_int), ("variant", C.c_int), ("num", C.c_int), ("split", C.c_int), ("pack", C.c_int),
                ("dTab", fp), ("dMeta", C.POINTER(C.c_int))]


HOP, NUM, CC, CLIPS, WAVES = 512, 128, 13, 3, 12


def clips(frames, seed):
    n = 2048 + (frames - 1) * HOP
    return np.ascontiguousarray(np.stack([cases.noise(seed + i, n) for i in range(CLIPS)]))


window = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2048) / 2048)).astype(np.float32)
bank, _, _ = restate.mel_bank(NUM, 2048, 16000, 0.0, 8000.0)
k = np.arange(NUM)
dct = (np.sqrt(2.0 / NUM) * np.cos(np.pi * np.outer(k, k + 0.5) / NUM))
dct[0] /= np.sqrt(2.0)
dct = np.ascontiguousarray(dct.astype(np.float32))
stream = C.cast((C.c_char * 8)(), vp)
band = Band()
assert lib.afx_bandplan_build(bank.ctypes.data_as(fp), NUM, 1025, C.byref(band)) == 0


def create(nopack):
    if nopack:
        os.environ["AFX_MEL_NOPACK"] = "1"
    else:
        os.environ.pop("AFX_MEL_NOPACK", None)
    plan = vp()
    assert lib.afxk_melfused_create(C.byref(plan), 11, window.ctypes.data_as(fp), C.byref(band), stream) == 0
    os.environ.pop("AFX_MEL_NOPACK", None)
    return plan


def ptr(a):
    return a.ctypes.data_as(vp)


def run(plan, route, xs):
    """every output of the route, NaN-filled first"""
    n = xs.shape[1]
    frames = (n - 2048) // HOP + 1
    a = Args()
    a.x, a.clipStride, a.batch, a.dataLength, a.timeLength, a.hop = ptr(xs), n, CLIPS, n, frames, HOP
    a.normValue = 1.0
    rows = lambda *shape: np.full((CLIPS * frames,) + shape, np.nan, np.float32)  # noqa: E731
    out = {"mel": rows(NUM)}
    a.out = ptr(out["mel"])
    if route == "mfcc":
        out["cc"] = rows(CC)
        a.dct, a.ccNum, a.cc = ptr(dct), CC, ptr(out["cc"])
    elif route == "complex":
        out["im"] = rows(NUM)
        a.specMap, a.outIm = 3, ptr(out["im"])
    elif route == "temporal":
        for name in ("energy", "rms", "zcr"):
            out[name] = rows()
        a.energy, a.rms, a.zcr = ptr(out["energy"]), ptr(out["rms"]), ptr(out["zcr"])
    st = lib.afxk_melfused_run(plan, C.byref(a), stream)
    assert st == 0, (route, st)
    for name, v in out.items():
        assert np.isfinite(v).all(), f"{route}: {name} has values that no wave wrote"
    return out


def same(a, b):
    return all(np.array_equal(a[name], b[name]) for name in a)


def set_cus(cus):
    if cus:
        os.environ["AFX_MEL_CUS"] = cus
    else:
        os.environ.pop("AFX_MEL_CUS", None)


def claimed_runs(total, cus):
    """run lengths of the first workgroup, claims taken one after the other: afx_frame_split (afx_device.h) with one round,
    wg_ranges and claim_length (afx_melfused2.hip).  (A claim's length comes from a read of the counter that may be stale, which
    can only make a run longer than listed; every claim made while 192 or more frames are left is a multiple of 16 either way.)"""
    one_round = cus * WAVES
    fpw = -(-total // one_round)
    if fpw < 16:
        fpw = min(-(-total // one_round), 16)
    wg_n = min(fpw * WAVES, total)
    min_run = 4 if wg_n >= 4 * WAVES else -(-wg_n // WAVES) if wg_n > WAVES else 1
    runs, done = [], 0
    while done < wg_n:
        left = wg_n - done
        g = left // (2 * WAVES)
        if left >= 16 * WAVES:
            ln = g & ~15 if g >= 16 else 16
        else:
            ln = g & ~3 if (g & ~3) > min_run else min_run
        runs.append(min(ln, left))
        done += ln
    return wg_n, runs


packed, plain = create(False), create(True)
assert lib.afxk_melfused_pack(packed) == 1 and lib.afxk_melfused_pack(plain) == 0
assert C.cast(packed, C.POINTER(Plan)).contents.pack == 1 and C.cast(plain, C.POINTER(Plan)).contents.pack == 0
assert lib.afxk_melfused_kind(packed) == 1 and lib.afxk_melfused_kind(plain) == 1
before = lib.afx_emulated_launches(b"k_stft_mel_v2")
xs = clips(37, 7300)
for cus in ("1", None):
    set_cus(cus)
    if cus:
        wg_n, runs = claimed_runs(3 * 37, 1)
        assert wg_n == 111 and max(runs) == 4, runs
    for route in ("mfcc", "complex", "temporal"):
        got, want = run(packed, route, xs), run(plain, route, xs)
        assert same(got, want), f"{route} at {cus or 'all'} CUs: the packed plan's bits differ"
        print(f"{route} at {cus or 'all'} CUs: packed equals unpacked, {', '.join(got)}")
assert lib.afx_emulated_launches(b"k_stft_mel_v2") == before + 12

# against float64, clip 0 (the plan layer's own window)
frames = np.stack([xs[0, i * HOP:i * HOP + 2048].astype(np.float64) * window for i in range(37)])
want = (np.abs(np.fft.rfft(frames)) ** 2) @ bank.astype(np.float64).T
err = np.abs(got["mel"][:37] - want).max() / np.abs(want).max()
print(f"clip 0 against float64: mel {err:.2e}")
assert err <= 1e-5

# whole 16-row cepstrum blocks: 3 x 301 frames in one workgroup
set_cus("1")
wg_n, runs = claimed_runs(3 * 301, 1)
assert wg_n == 903 and runs[0] == 32 and 16 in runs and 4 in runs and sum(runs) == 903, runs
assert all(r % 16 == 0 for r, left in zip(runs, np.cumsum([0] + runs[:-1])) if 903 - left >= 192), runs
long_xs = clips(301, 7400)
got, want = run(packed, "mfcc", long_xs), run(plain, "mfcc", long_xs)
assert same(got, want), "3 x 301 frames on one CU: the packed plan's bits differ"
print(f"16-row blocks: 903 frames in one workgroup, runs {sorted(set(runs), reverse=True)}: packed equals unpacked")
set_cus(None)

# a plan corrupted on purpose: one continuation flag flipped (meta row 6: "b continues a") on a lane that stores a row from b
meta = C.cast(packed, C.POINTER(Plan)).contents.dMeta
lane = next(l for l in range(64) if meta[192 + 64 + l] >= 0)
meta[384 + lane] ^= 1
bad = run(packed, "mfcc", xs)
good = run(plain, "mfcc", xs)
assert not same(bad, good), "a flipped continuation flag went unnoticed"
diff = np.argwhere((bad["mel"] != good["mel"]).any(axis=0)).ravel()
assert list(diff) == [meta[192 + 64 + lane]], diff  # exactly that lane's row
meta[384 + lane] ^= 1
assert same(run(packed, "mfcc", xs), good)
print(f"a flipped continuation flag (lane {lane}) changes row {diff[0]} and is caught")
lib.afxk_melfused_destroy(packed)
lib.afxk_melfused_destroy(plain)
lib.afx_bandplan_free(C.byref(band))
print("OK")
