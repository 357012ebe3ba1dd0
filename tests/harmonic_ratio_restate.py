"""float64 restatement of the harmonic ratio (include/mir/harmonicRatio_algorithm.h), written from the reference's text
(harmonicRatio_algorithm.c:172-287, flux_util.c:771-780), with numpy's FFT.  With N = 2^radix2_exp and L = 2N:

    frame t   f = x[t hop : t hop + N] * window (the float32 product the reference forms), zero-padded to L
    r         = real(ifft_L(|fft_L(f)|^2)): r[0] is the frame's energy
    c[j]      = cum[N - 2 - j], cum[n] = sum of f[m]^2, m <= n
    own       = j - 1 for the first j in 2 ... maxLength with (r[j] >= 0 and r[j-1] <= 0) or (r[j] <= 0 and r[j-1] >= 0), else None
    minIndex  = own, or what the previous frame of the same call used (0 in front of the first frame)
    g[j]      = r[j] / sqrt(r[0] c[j] + 1e-16) for j = minIndex + 1 ... maxLength - 1, 0 below
    lag       = the first maximum of g over that range (a strict >), -1 when the range is empty
    value     = 0 for an empty range; g[lag] at either end of the range; else with v1, v2, v3 = g[lag - 1 ... lag + 1]
                p = (v3 - v1) / (2 (2 v2 - v3 - v1) + 1e-16), value = v2 - 0.25 (v1 - v3) p

Per frame it also keeps `weight`, the first-order change of each g[j] when every spectrum bin moves by max|X| -- what
tests/harmonic_ratio_check.py prices errors with (derived there) --, and D, that change of any r[n]."""
import numpy as np


def spectrum(xw):
    """xw: the windowed frame (float64, N samples) -> dict(r, c, D): everything that does not depend on minIndex"""
    N = len(xw)
    L = 2 * N
    X = np.fft.fft(np.concatenate([xw, np.zeros(N)]))
    mag = np.abs(X)
    r = np.fft.ifft(X.real * X.real + X.imag * X.imag).real
    cum = np.cumsum(xw * xw)
    c = cum[N - 2 - np.arange(N - 1)]  # c[j], j = 0 ... N - 2
    D = 2.0 / L * float(np.sum(mag)) * float(mag.max())
    return {"r": r, "c": c, "D": D}


def own_crossing(r, max_length):
    for j in range(2, max_length + 1):
        if (r[j] >= 0 and r[j - 1] <= 0) or (r[j] <= 0 and r[j - 1] >= 0):
            return j - 1
    return None


def evaluate(sp, max_length, min_index):
    """the frame with minIndex given -> dict(curve [maxLength], weight [maxLength], lag, value, W)"""
    r, c, D = sp["r"], sp["c"], sp["D"]
    r0 = r[0]
    curve, weight = np.zeros(max_length), np.zeros(max_length)
    js = np.arange(min_index + 1, max_length)
    if len(js):
        den = np.sqrt(r0 * c[js] + 1e-16)
        curve[js] = r[js] / den
        if r0 > 0:
            weight[js] = D / den * (1.0 + np.abs(r[js]) / (2.0 * r0)) + np.abs(curve[js]) / 2.0
    if not len(js):
        return {"curve": curve, "weight": weight, "lag": -1, "value": 0.0, "W": 0.0}
    lag, best = int(js[0]), curve[js[0]]
    for j in js[1:]:
        if best < curve[j]:
            best, lag = curve[j], int(j)
    if lag == js[0] or lag == js[-1]:
        return {"curve": curve, "weight": weight, "lag": lag, "value": float(best), "W": float(weight[lag])}
    v1, v2, v3 = curve[lag - 1], curve[lag], curve[lag + 1]
    p = (v3 - v1) / (2 * (2 * v2 - v3 - v1) + 1e-16)
    return {"curve": curve, "weight": weight, "lag": lag, "value": float(v2 - 0.25 * (v1 - v3) * p),
            "W": float(weight[lag - 1:lag + 2].sum())}


def harmonic_ratio(x, window, r, hop, max_length):
    """x float32 samples, window the float32 table of N entries -> list of frame dicts: spectrum() + evaluate() with the
    restatement's own minIndex chain, plus own (None: inherited) and first (the minIndex used)"""
    N = 1 << r
    T = 0 if len(x) < N else (len(x) - N) // hop + 1
    out, carry = [], 0
    for t in range(T):
        sp = spectrum((x[t * hop:t * hop + N] * window).astype(np.float64))
        own = own_crossing(sp["r"], max_length)
        carry = carry if own is None else own
        sp.update(evaluate(sp, max_length, carry))
        sp.update(own=own, first=carry)
        out.append(sp)
    return out
