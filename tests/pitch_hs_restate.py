"""A float64 statement of the reference's HPS and LHS pitch trackers (src/mir/_pitch_hps.c:415-518, _pitch_lhs.c:416-532),
independent of the library and of the kernel's factorisation: numpy's FFT of the zero-padded frame at M points.

Per frame a dict:
  curve   [maxIndex + 1] float64 -- prod_k |X[j (k + 1)]| or sum_k log |X[j (k + 1)]| (-inf where a bin is 0)
  index   first argmax over minIndex ... maxIndex (an all-equal row gives minIndex)
  margin  curve[index] - the best other candidate (0 for ties, inf when there is no other candidate)
  weight  [maxIndex + 1] -- first-order change of curve[j] when each bin it reads moves by max|X|:
          LHS sum_k max|X| / |X[j (k + 1)]|,  HPS sum_k max|X| prod_{l != k} |X[j (l + 1)]|
  xmax    max |X| over the M bins
"""
import numpy as np

HPS, LHS = 0, 1


def window(wtype, N):
    """window_calFFTWindow for the types the cases use, in float64"""
    n = np.arange(N)
    if wtype == 1:
        return 0.5 - 0.5 * np.cos(2 * np.pi * n / N)
    if wtype == 2:
        return 0.54 - 0.46 * np.cos(2 * np.pi * n / N)
    if wtype == 5:
        return np.bartlett(N)
    if wtype == 0:
        return np.ones(N)
    raise KeyError(wtype)


def frame(kind, xw, M, mn, mx, count):
    """xw: the windowed frame (float64)"""
    mag = np.abs(np.fft.fft(xw, M))
    xmax = float(mag.max())
    j = np.arange(mx + 1)
    bins = mag[j[:, None] * (np.arange(count) + 1)[None, :]]  # [mx + 1, count]
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == LHS:
            curve = np.log(bins).sum(axis=1)
            weight = (xmax / bins).sum(axis=1) if xmax > 0 else np.full(mx + 1, np.inf)
        else:
            curve = bins.prod(axis=1)
            weight = np.zeros(mx + 1)
            for k in range(count):
                weight += xmax * np.delete(bins, k, axis=1).prod(axis=1)
    cand = curve[mn:mx + 1]
    if len(cand) == 0:
        return {"curve": curve, "index": mn, "margin": np.inf, "weight": weight, "xmax": xmax}
    i = int(np.argmax(cand)) if not np.all(np.isneginf(cand)) else 0
    others = np.delete(cand, i)
    with np.errstate(invalid="ignore"):
        margin = float(cand[i] - others.max()) if len(others) else np.inf
    if np.isnan(margin):  # -inf against -inf
        margin = 0.0
    return {"curve": curve, "index": mn + i, "margin": margin, "weight": weight, "xmax": xmax}


def pitch(kind, x, sr, r, hop, wtype, M, mn, mx, count):
    """x float32 -> list of frame dicts"""
    N = 1 << r
    w = window(wtype, N).astype(np.float32).astype(np.float64)
    x = np.asarray(x, np.float32).astype(np.float64)
    T = 0 if len(x) < N else (len(x) - N) // hop + 1
    return [frame(kind, x[t * hop:t * hop + N] * w, M, mn, mx, count) for t in range(T)]


def fre_of(index, sr, M):
    """freArr[i] = (index + 1) * (1.0 * samplate / M), stored as float"""
    return np.float32((index + 1) * (1.0 * sr / M))
