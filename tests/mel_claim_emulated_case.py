#!/usr/bin/env python3
"""The claim path of k_stft_mel_v2 as emulated device code (tests/test_mel_claim_emulated.py): 3 clips x 301 frames at hop 512,
mel-128 + MFCC-13 in ONE launch with the grid sized for one CU (AFX_MEL_CUS=1: one workgroup owns all 903 frames, its twelve
waves claim 16-frame runs, then 4-frame runs), against the same clips one per call (312-frame ranges: other runs) -- equal bits.
AFX_LIB = the library tests/test_emulated_kernels.py builds."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import restate  # noqa: E402
from tests import cases  # noqa: E402

assert os.environ.get("AFX_MEL_CUS") == "1"
lib = C.CDLL(os.environ["AFX_LIB"])
vp, fp = C.c_void_p, C.POINTER(C.c_float)
lib.bftObj_calTimeLength.restype = C.c_int
lib.afx_bftXxccOneLaunchCount.restype = C.c_longlong
lib.afx_emulated_launches.restype = C.c_int
lib.afx_emulated_launches.argtypes = [C.c_char_p]


def I(v):
    return C.byref(C.c_int(v))


def F(v):
    return C.byref(C.c_float(v))


FRAMES, HOP, NUM, CC = 301, 512, 128, 13
n = 2048 + (FRAMES - 1) * HOP
xs = np.stack([cases.noise(900 + HOP + i, n) for i in range(3)])
h, xx = vp(), vp()
assert lib.bftObj_new(C.byref(h), NUM, 11, I(16000), F(0.0), F(8000.0), None, I(1), I(HOP), I(2), I(0), I(0), I(0), None, None) == 0
assert lib.xxccObj_new(C.byref(xx), NUM) == 0
lib.bftObj_setResultType(h, 1)
assert lib.bftObj_calTimeLength(h, n) == FRAMES
stream = C.cast((C.c_char * 8)(), vp)


def run(x):
    b = x.shape[0]
    mel, cc = np.full((b, FRAMES, NUM), np.nan, np.float32), np.full((b, FRAMES, CC), np.nan, np.float32)
    before = lib.afx_bftXxccOneLaunchCount()
    st = lib.afx_bftXxccBatchDevice(h, xx, x.ctypes.data_as(fp), b, n, C.c_longlong(n), CC, None, mel.ctypes.data_as(fp), cc.ctypes.data_as(fp), stream)
    assert st == 0 and lib.afx_bftXxccOneLaunchCount() == before + 1, st
    assert np.isfinite(mel).all() and np.isfinite(cc).all(), "rows that no wave wrote"
    return mel, cc


mel, cc = run(xs)
for i in range(3):
    m1, c1 = run(xs[i:i + 1])
    assert np.array_equal(mel[i], m1[0]) and np.array_equal(cc[i], c1[0]), f"clip {i}: a frame's values depend on its run"
bank, _, _ = restate.mel_bank(NUM, 2048, 16000, 0.0, 8000.0)
want = restate.bft(xs[0], bank, 2048, HOP)
err = np.abs(mel[0] - want).max() / np.abs(want).max()
errc = np.abs(cc[0] - restate.xxcc(want, CC, "log")).max() / np.abs(restate.xxcc(want, CC, "log")).max()
print(f"3 x {FRAMES} frames in one workgroup equal the per-clip calls; clip 0 against float64: mel {err:.2e} mfcc {errc:.2e}")
assert err <= 1e-5 and errc <= 1e-5
assert lib.afx_emulated_launches(b"k_stft_mel_v2") == 4
lib.xxccObj_free(xx)
lib.bftObj_free(h)
print("OK")
