"""A float64 statement of the reference's PEF pitch tracker per frame (src/mir/_pitch_pef.c:258-426), independent of the
library and of either side's transforms: numpy's FFT for the power spectrum, a direct sum for the correlation.  It is driven
by the float32 TABLES (window, lin, lg, bw, h -- the reference's own, or afx_pitch_pef_plan_host's, which
tests/test_pitch_pef_cpu.py holds bit-equal to them), taken to float64.

Per frame a dict:
  curve   [maxIndex + 1] float64 -- R[k] = sum_{n < N} h[n] B[n + k], B[P + m] = y[m] bw[m]
  index   first argmax over minIndex ... maxIndex (an all-equal row gives minIndex)
  scale   S = max_k |R[k]| over 0 ... maxIndex
"""
import numpy as np


def interp_index(lin, lg):
    """the walk of __vinterp_linear (flux_vectorOp.c:580-610): per lg[m] the first i with lg[m] <= lin[i + 1]; N: past the end"""
    return np.searchsorted(lin[1:], lg, side="left")


def frame(xw, tables, N, P, mn, mx):
    """xw: the windowed frame (float64)"""
    lin, lg, bw, h = (tables[k].astype(np.float64) for k in ("lin", "lg", "bw", "h"))
    pw = np.abs(np.fft.rfft(xw, 2 * N)) ** 2  # [N + 1]
    i = interp_index(tables["lin"], tables["lg"])
    inside = i < N
    j = np.minimum(i, N - 1)
    y = np.where(inside, pw[j] + (lg - lin[j]) * (pw[j + 1] - pw[j]) / (lin[j + 1] - lin[j]), pw[N])
    B = np.zeros(4 * N)
    B[P:P + 2 * N] = y * bw
    curve = np.correlate(B[:mx + N], h, "valid")  # [mx + 1]
    cand = curve[mn:mx + 1]
    return {"curve": curve, "index": mn + int(np.argmax(cand)), "scale": float(np.abs(curve).max())}


def pitch(x, tables, r, hop, P, mn, mx):
    """x float32 -> list of frame dicts"""
    N = 1 << r
    w = tables["window"].astype(np.float64)
    x = np.asarray(x, np.float32).astype(np.float64)
    T = 0 if len(x) < N else (len(x) - N) // hop + 1
    return [frame(x[t * hop:t * hop + N] * w, tables, N, P, mn, mx) for t in range(T)]
