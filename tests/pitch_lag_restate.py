"""float64 restatement of the two lag-domain pitch trackers (include/mir/_pitch_ncf.h, include/mir/_pitch_cep.h), written from
the reference's text (_pitch_ncf.c:380-494, _pitch_cep.c:381-474), with numpy's FFT.  With N = 2^radix2_exp and L = 2N:

    frame t = x[t hop : t hop + N] * window (the float32 table; Rect: no multiply), zero-padded to L
    X = fft_L(frame), P[k] = |X[k]|^2 for all L bins
    NCF   r = real(ifft_L(P)) (normalised by 1 / L);  curve[i] = L^(-1/4) r[i + 1] / sqrt(r[0]) for i = minIndex - 1 ...
          maxIndex - 1, curve[i] = 0 elsewhere in 0 ... maxIndex (curve[maxIndex] included: the reference never computes
          it); a frame with r[0] == 0 has NaN in every computed entry
    CEP   curve[q] = real(ifft_L(ln P))[q], q = 0 ... maxIndex; a frame in which a bin of P is exactly 0 is a row of NaN
    index = first maximum over minIndex ... maxIndex as __vmax picks it (flux_vector.c:1536): a strict >, a NaN in first
            position wins, later NaNs never do
    fre   = samplate / (index + 1), in double, rounded to float32

Per frame it also returns `weight`, the first-order change of each curve entry when every spectrum bin moves by max|X| --
what tests/pitch_lag_check.py prices errors with (derived there)."""
import numpy as np

NCF, CEP = "NCF", "CEP"


def first_max(c, mn, mx):
    """__vmax over c[mn ... mx], + mn"""
    best, at = c[mn], mn
    for j in range(mn + 1, mx + 1):
        if best < c[j]:
            best, at = c[j], j
    return at


def frame(kind, xw, mn, mx):
    """xw: the windowed frame (float64, N samples) -> dict(curve [mx + 1], weight [mx + 1], index)"""
    N = len(xw)
    L = 2 * N
    X = np.fft.fft(np.concatenate([xw, np.zeros(N)]))
    mag = np.abs(X)
    P = X.real * X.real + X.imag * X.imag
    top = float(mag.max())
    curve = np.zeros(mx + 1)
    weight = np.zeros(mx + 1)
    if kind == NCF:
        r = np.fft.ifft(P).real
        lags = np.arange(max(mn - 1, 0), mx)  # entries mn - 1 ... mx - 1
        if r[0] == 0:
            curve[lags] = np.nan
        else:
            K = float(L) ** -0.25
            D = float(np.sum(2.0 * mag * top)) / L  # change of any r[n]
            curve[lags] = K * r[lags + 1] / np.sqrt(r[0])
            weight[lags] = K * D / np.sqrt(r[0]) * (1.0 + np.abs(r[lags + 1]) / (2.0 * r[0]))
    else:
        if (P == 0).any():
            curve[:] = np.nan
        else:
            curve[:] = np.fft.ifft(np.log(P)).real[:mx + 1]
            weight[:] = float(np.sum(2.0 * top / mag)) / L
    return {"curve": curve, "weight": weight, "index": first_max(curve, mn, mx)}


def pitch(kind, x, window, r, hop, mn, mx):
    """x float32 samples, window the float32 table of N entries or None (Rect) -> list of frame dicts"""
    N = 1 << r
    T = 0 if len(x) < N else (len(x) - N) // hop + 1
    out = []
    for t in range(T):
        xw = x[t * hop:t * hop + N]
        if window is not None:
            xw = xw * window  # the float32 product the reference forms
        out.append(frame(kind, xw.astype(np.float64), mn, mx))
    return out


def fre_of(index, sr):
    return np.float32(1.0 * sr / (np.asarray(index) + 1))
