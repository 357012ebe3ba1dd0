"""Float64 numpy statement of harmonic / percussive separation as the reference computes it (src/mir/hpss_algorithm.c:117-327):
the third opinion beside the compiled reference and the library, and the source of the bitwise median check."""
import numpy as np


def window(window_type, n):
    k = np.arange(n)
    if window_type == 2:
        return 0.54 - 0.46 * np.cos(2 * np.pi * k / n)
    if window_type == 1:
        return 0.5 - 0.5 * np.cos(2 * np.pi * k / n)
    assert window_type == 0
    return np.ones(n)


def median_filter(plane, axis, order, frames_per_clip=0):
    """the middle element of the sorted, zero-padded window of odd `order` around every cell along `axis`; axis 0 never reads across
    a clip of frames_per_clip rows.  Pure selection: the result has the dtype and the bits of the input."""
    plane = np.asarray(plane)
    assert order % 2 == 1
    if axis == 0 and frames_per_clip and frames_per_clip < plane.shape[0]:
        return np.concatenate([median_filter(plane[i:i + frames_per_clip], 0, order) for i in range(0, plane.shape[0], frames_per_clip)])
    half = order // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (half, half)
    p = np.pad(plane, pad)
    win = np.lib.stride_tricks.sliding_window_view(p, order, axis=axis)
    return np.sort(win, axis=-1)[..., half].copy()


def frames(x, n_fft, hop):
    t = (len(x) - n_fft) // hop + 1 if len(x) >= n_fft else 0
    return np.stack([x[i * hop:i * hop + n_fft] for i in range(t)]) if t else np.zeros((0, n_fft))


def istft_wola(spec_half, n_fft, hop, w, init):
    """stftObj_istft type 0 (stft_algorithm.c:304-409): (init + sum frames x w) / clamp(sum w^2, 1e-6 -> 1)"""
    t = spec_half.shape[0]
    fr = np.fft.irfft(spec_half, n=n_fft, axis=1) * w
    n = (t - 1) * hop + n_fft
    acc = np.asarray(init, np.float64)[:n].copy()
    nrm = np.zeros(n)
    for i in range(t):
        acc[i * hop:i * hop + n_fft] += fr[i]
        nrm[i * hop:i * hop + n_fft] += w * w
    return acc / np.where(nrm < 1e-6, 1.0, nrm)


def spectra(x, radix2_exp, window_type, h_order, p_order):
    """-> (complex half spectrum, mag, H, P) of one clip, [T, N/2 + 1]"""
    n_fft = 1 << radix2_exp
    hop = n_fft // 4
    w = window(window_type, n_fft)
    s = np.fft.rfft(frames(np.asarray(x, np.float64), n_fft, hop) * w, axis=1)
    mag = np.abs(s)
    h = median_filter(mag, 0, h_order)  # (order 1: the identity -- the library's documented deviation)
    p = median_filter(mag, 1, p_order)
    den = np.maximum(h * h + p * p, 1e-16)
    return s, mag, h * h / den * mag, p * p / den * mag


def hpss(x, radix2_exp, window_type, h_order, p_order, init_h=None, init_p=None):
    n_fft = 1 << radix2_exp
    hop = n_fft // 4
    w = window(window_type, n_fft)
    s, mag, hm, pm = spectra(x, radix2_exp, window_type, h_order, p_order)
    t = s.shape[0]
    if t == 0:
        return np.zeros(0), np.zeros(0)
    n = (t - 1) * hop + n_fft
    unit = s / np.maximum(mag, 1e-16)
    zero = np.zeros(n)
    return (istft_wola(unit * hm, n_fft, hop, w, zero if init_h is None else init_h),
            istft_wola(unit * pm, n_fft, hop, w, zero if init_p is None else init_p))


def condition(radix2_exp, window_type, t):
    """per output sample: sum of w over the frames that cover it / clamp(sum of w^2): how much the float32 rounding of a frame's
    inverse transform is amplified there (tests/conftest.py::assert_istft_parity)"""
    n_fft = 1 << radix2_exp
    hop = n_fft // 4
    w = window(window_type, n_fft)
    n = (t - 1) * hop + n_fft
    gain, nrm = np.zeros(n), np.zeros(n)
    for i in range(t):
        gain[i * hop:i * hop + n_fft] += np.abs(w)
        nrm[i * hop:i * hop + n_fft] += w * w
    return gain / np.where(nrm < 1e-6, 1.0, nrm)
