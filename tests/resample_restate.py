"""The resampler restated in numpy (src/dsp/resample_algorithm.c of the reference): the table in float64 closed form, and
the tap sums with the reference's float32 phase arithmetic and float64 accumulation.  `exact_phase=True` is the control:
the same sums with the phase i / ratio kept in float64, which is NOT what the reference computes."""
import numpy as np

f32 = np.float32


def _i0(x):
    return np.i0(x)


def window_right_half(win, value, length):
    """float64 right half (centre first) of the symmetric window of 2 (length - 1) + 1 points"""
    m = 2 * (length - 1)            # the window's last index; the centre is at length - 1
    k = np.arange(length, dtype=np.float64) + (length - 1)
    u = k / m                       # 0.5 ... 1
    if win == 1:                    # Hann
        return 0.5 - 0.5 * np.cos(2 * np.pi * u)
    if win == 4:                    # Kaiser, beta = value
        return _i0(value * np.sqrt(1 - (2 * u - 1) ** 2)) / _i0(value)
    if win == 8:                    # Gauss, alpha = value: exp(-0.5 (alpha (k - centre) / (m / 2))^2)
        return np.exp(-0.5 * (2 * value * (k - (length - 1)) / m) ** 2)
    if win == 13:                   # Tukey, alpha = value
        a = value
        w = np.ones(length)
        edge = u >= 1 - a / 2
        w[edge] = 0.5 * (1 + np.cos(2 * np.pi / a * (u[edge] - 1 + a / 2)))
        return w
    raise ValueError(win)


def table(zero_num, nbit, win, value, roll_off):
    """rollOff sinc(rollOff u) on linspace(0, zeroNum) times the window's right half, float64, before any ratio"""
    length = zero_num * (1 << nbit) + 1
    u = np.arange(length, dtype=np.float64) / (1 << nbit)
    return float(f32(roll_off)) * np.sinc(float(f32(roll_off)) * u) * window_right_half(win, float(f32(value)), length)


def resample(x, tab, ratio, bit_length, target_length, scale_out=False, exact_phase=False):
    """x: the samples the call consumes; tab: the object's float32 table as it stands (times ratio when that is < 1); ratio:
    the float32 ratio.  Float32 phase (one float64 division rounded to float32, factor and scale - factor single float32
    roundings), weights and sums in float64."""
    x = np.asarray(x, np.float64)
    tab = np.asarray(tab, f32)
    S, L = len(x), len(tab)
    dtab = np.zeros(L, f32)
    dtab[:-1] = tab[1:] - tab[:-1]  # one float32 subtraction; the last entry is 0
    tab64, dtab64 = tab.astype(np.float64), dtab.astype(np.float64)
    ratio = f32(ratio)
    scale = f32(min(1.0, float(ratio)))
    step = int(np.floor(f32(scale * f32(bit_length))))
    i = np.arange(target_length, dtype=np.float64)
    if exact_phase:
        t = i / float(ratio)
        n = np.floor(t)
        fl = float(scale) * (t - n)
        fr = float(scale) - fl
    else:
        t = (i / float(ratio)).astype(f32)
        n = np.floor(t)
        fl = (scale * (t - n.astype(f32))).astype(f32)
        fr = (scale - fl).astype(f32)
    n = n.astype(np.int64)
    out = np.zeros(target_length, np.float64)
    for f, first, direction, room in ((fl, n, -1, n + 1), (fr, n + 1, 1, S - n - 1)):
        fv = f.astype(np.float64) * bit_length
        off = np.floor(fv).astype(np.int64)
        delta = fv - off
        count = np.minimum(room, (L - off) // step)
        for j in range(int(count.max()) if len(count) else 0):
            m = j < count
            o = off[m] + j * step
            idx = first[m] + direction * j
            ok = idx < S  # samples past the input count as 0
            w = tab64[o] + delta[m] * dtab64[o]
            acc = np.zeros(m.sum())
            acc[ok] = w[ok] * x[idx[ok]]
            out[m] += acc
    if scale_out:
        out /= np.sqrt(float(ratio))
    return out
