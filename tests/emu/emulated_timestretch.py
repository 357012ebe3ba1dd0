#!/usr/bin/env python3
"""afx_phasevocoder.hip as emulated device code through afx_phase_vocoder_device: the reference's own STFT of cases of
tests/timestretch_cases.py (half spectra, and full spectra with pitch N) against the reference's phase_vocoder at the case's
recorded L2 bar, the mirror bins exact conjugates, two clips in one call bitwise the single calls, refusals; and the plan
function's k / alpha table against the same arithmetic in numpy.
AFX_LIB = the library tests/test_timestretch_emulated.py builds.  Arguments: case names (default: SMALL)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import timestretch_cases as tc  # noqa: E402

lib = tc.bind(C.CDLL(os.environ["AFX_LIB"]))


def vocoder(re, im, c, rate, batch=1):
    """afx_phase_vocoder_device on [batch * T1, pitch] planes: (status, re2, im2 [batch * T2, N] in guarded buffers)"""
    N = 1 << c["exp"]
    T1 = re.shape[0] // batch
    T2 = int(np.ceil(np.float32(T1) / np.float32(rate)))
    re2, im2 = np.full((batch * T2 + 1, N), 7.5, np.float32), np.full((batch * T2 + 1, N), 7.5, np.float32)
    st = lib.afx_phase_vocoder_device(tc.ptr(re), tc.ptr(im), batch, T1, c["exp"], re.shape[1], c["hop"], C.c_float(rate), tc.ptr(re2),
                                      tc.ptr(im2), None)
    assert (re2[-1] == 7.5).all() and (im2[-1] == 7.5).all(), "the row behind the output was written"
    return st, re2[:-1], im2[:-1]


def case(name):
    c = tc.CASES[name]
    N = 1 << c["exp"]
    F = N // 2 + 1
    re, im, wr, wi = tc.expected_vocoder(name)
    keep = re.copy()
    st, re2, im2 = vocoder(re, im, c, c["rate"])
    assert st == 0 and np.array_equal(re, keep), (name, st)
    got = np.concatenate([re2[:, :F], im2[:, :F]]).astype(np.float64)
    want = np.concatenate([wr, wi]).astype(np.float64)
    l2 = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    bar = tc.bar(name)[1]
    assert l2 <= bar, (name, l2, bar)
    j = np.arange(1, N // 2)
    assert tc.same_bits(re2[:, N - j], re2[:, j]) and tc.same_bits(im2[:, N - j], -im2[:, j]), name
    # full spectra with pitch N, two clips: bitwise the single call
    full = np.zeros((2 * re.shape[0], N), np.float32)
    fim = np.full_like(full, np.nan)
    full[:re.shape[0], :F], fim[:re.shape[0], :F] = re, im
    full[re.shape[0]:, :F], fim[re.shape[0]:, :F] = re[::-1], im[::-1]
    full[:, F:] = np.nan  # (bins above N / 2 are not read)
    st, b2, bi2 = vocoder(full, fim, c, c["rate"], batch=2)
    assert st == 0 and tc.same_bits(b2[:re2.shape[0]], re2) and tc.same_bits(bi2[:re2.shape[0]], im2), name
    assert np.isfinite(b2).all() and np.isfinite(bi2).all()
    print(f"vocoder {name}: {re.shape[0]} -> {re2.shape[0]} frames of {N}, l2-rel {l2:.2e} (bar {bar:.1e})", flush=True)


def extras():
    c = tc.CASES["256_64_r0.8"]
    re = np.ones((4, 129), np.float32)
    out = np.zeros((8, 256), np.float32)
    f = lib.afx_phase_vocoder_device
    args = lambda **k: [k.get("re", tc.ptr(re)), tc.ptr(re), k.get("batch", 1), k.get("T1", 4), k.get("exp", 8), k.get("pitch", 129),  # noqa: E731
                        k.get("hop", 64), C.c_float(k.get("rate", 0.8)), tc.ptr(out), k.get("out", tc.ptr(out)), None]
    assert f(*args()) == 0
    for bad in (dict(re=None), dict(out=None), dict(batch=0), dict(T1=0), dict(exp=0), dict(exp=15), dict(pitch=128), dict(hop=0),
                dict(rate=0.0), dict(rate=-1.0), dict(rate=float("nan")), dict(rate=float("inf"))):
        assert f(*args(**bad)) == -6, bad
    # the plan's table against the float32 statement
    for rate in (0.5, 0.8, 1.7, 2.0):
        p = tc.Plan()
        k, a = np.zeros(4096, np.int32), np.zeros(4096, np.float32)
        assert lib.afx_timestretch_plan(c["exp"], c["hop"], C.c_float(rate), 3000, 1, 0, C.byref(p), tc.ptr(k), tc.ptr(a)) == 0
        t = np.arange(p.T2, dtype=np.float32) * np.float32(rate)
        assert np.array_equal(k[:p.T2], np.floor(t).astype(np.int32)) and np.array_equal(a[:p.T2], t - np.floor(t)), rate
    print("vocoder: refusals, the plan's k / alpha table", flush=True)


def main(argv):
    for name in [a for a in argv if a != "extras"] or (list(tc.SMALL) if not argv else []):
        case(name)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
