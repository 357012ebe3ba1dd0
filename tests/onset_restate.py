"""Restatement of the onset detector (src/mir/onset_algorithm.c, src/flux_spectral.c, __vmaxfilter of
src/vector/flux_vector.c) in numpy: the max filter, the eleven novelty functions and the normalisation in float64 on the
float32 inputs, and the pick rule in float64 and in float32 (the float32 form is the reference's arithmetic operation for
operation: the window's maximum by comparison, the mean as a float32 sum in index order divided by the count)."""
import numpy as np

from tests.onset_cases import BROADBAND, CD, FLUX, HFC, MKL, NWPD, PD, RCD, SD, SF, WPD

DEFAULT_PARAM = (1, 1.0, 1, 0, 0, 0.0, 0, 1.0)


def pick_params(sr, hop):
    """onset_algorithm.c:123-133: the products in double, floored as float"""
    sr = 32000 if sr <= 0 else sr
    hop = 512 if hop < 1 else hop
    f = lambda v: int(np.floor(np.float32(v)))  # noqa: E731
    return [f(0.03 * sr / hop), f(0.0 * sr / hop + 1), f(0.1 * sr / hop), f(0.1 * sr / hop + 1), f(0.03 * sr / hop)], np.float32(0.07)


def max_filter(x, order):
    """flux_vector.c:3063-3081 along the last axis: window j - order // 2 ... j - 1 + order - order // 2, cut at the ends"""
    x = np.asarray(x)
    if order < 2:
        return x.copy()
    M = x.shape[-1]
    left, right = order // 2, order - order // 2
    out = np.empty_like(x)
    for j in range(M):
        out[..., j] = x[..., max(j - left, 0):min(j - 1 + right, M - 1) + 1].max(axis=-1)
    return out


def effective_param(param):
    step, p, pos, is_exp, typ, thr = (DEFAULT_PARAM if param is None else param)[:6]
    return (step if step > 0 else 1), (p if p != 0 else 1.0), pos, is_exp, typ, thr


def novelty64(spec, phase, kind, param=None, index=None):
    """the raw novelty curve [T] in float64 of float32 rows [T, M] (onset_algorithm.c:318-377); entries the reference
    leaves to the caller's array (or counts onto it) are those of a zeroed array"""
    s = np.asarray(spec, np.float64)
    T, M = s.shape
    idx = np.arange(M) if index is None else np.asarray(index, np.int64)
    step, p, pos, is_exp, typ, thr = effective_param(param)
    p = float(np.float32(p))
    thr = float(np.float32(thr))
    x = s[:, idx]
    out = np.zeros(T)
    if kind == HFC:
        return (x * idx[None, :]).sum(axis=1)
    if kind in (SD, SF) or kind not in (MKL, PD, WPD, NWPD, CD, RCD, BROADBAND):
        d = x[step:] - x[:-step] if step < T else np.zeros((0, len(idx)))
        d = np.maximum(d, 0) if pos else np.abs(d)
        if kind == SD:
            v = d.sum(axis=1)
        elif kind == SF:
            v = (d * d).sum(axis=1)
        else:  # flux, and every value that is no named kind
            v = (d ** p).sum(axis=1)
            if typ:
                v = v / len(idx)
            if is_exp:
                v = v ** (1.0 / p)
        out[step:] = v
        return out
    if kind == MKL:
        v = np.log(1 + x[1:] / (x[:-1] + 1e-16)).sum(axis=1)
        out[1:] = v / len(idx) if typ else v
        return out
    if kind == BROADBAND:
        with np.errstate(divide="ignore", invalid="ignore"):
            out[1:] = (10 * np.log10(x[1:] / x[:-1]) > thr).sum(axis=1)
        return out
    ph = np.asarray(phase, np.float64)[:, idx]
    if kind in (PD, WPD, NWPD):
        v = np.abs(ph[2:] - 2 * ph[1:-1] + ph[:-2])
        if kind != PD:
            v = v * x[2:]
        v = v.sum(axis=1) / len(idx)
        if kind == NWPD:
            v = v / (x[2:].sum(axis=1) / len(idx) + 1e-16)
        out[2:] = v
        return out
    # cd / rcd
    re, im = x * np.cos(ph), x * np.sin(ph)
    for i in range(1, T):
        r, q = re[i].copy(), im[i].copy()
        if i > 1:
            a = 2 * ph[i - 1] - ph[i - 2]
            r -= x[i - 1] * np.cos(a)
            q -= x[i - 1] * np.sin(a)
        v = np.sqrt(r * r + q * q)
        if kind == RCD:
            v = np.where(x[i] <= x[i - 1], 0.0, v)
        out[i] = v.sum()
    return out


def normalise(raw, dtype=np.float64):
    """onset_algorithm.c:379-385 in `dtype`: v - min over ALL entries, then / max when that is > 0"""
    e = np.asarray(raw, dtype)
    e = e - e.min()
    mx = e.max()
    return (e / mx).astype(dtype) if mx > 0 else e


def envelope64(spec, phase, kind, order=1, param=None, index=None):
    return normalise(novelty64(max_filter(np.asarray(spec, np.float32), order), phase, kind, param, index))


def windows(i, n, pre, post):
    return max(i - pre, 0), (i - 1 + post if i + post < n else n - 1)


def mean32(e, a, b):
    """__vmean (flux_vector.c:1651-1660): a float32 sum in index order, divided by the count"""
    s = np.float32(0)
    for v in e[a:b + 1]:
        s = np.float32(s + v)
    return np.float32(s / np.float32(b - a + 1))


def pick(e, params, delta, dtype=np.float32):
    """__peakPick (onset_algorithm.c:423-460) in `dtype` -> the points"""
    pre_max, post_max, pre_avg, post_avg, wait = params
    e = np.asarray(e, dtype)
    n = len(e)
    delta = dtype(delta)
    pts, pre = [], -wait - 1
    for i in range(n):
        a, b = windows(i, n, pre_max, post_max)
        if e[i] != e[a:b + 1].max():
            continue
        a, b = windows(i, n, pre_avg, post_avg)
        mean = mean32(e, a, b) if dtype == np.float32 else e[a:b + 1].sum() / (b - a + 1)
        if e[i] >= dtype(mean + delta) and i - pre > wait:
            pts.append(i)
            pre = i
    return np.array(pts, np.int32)


def margins64(e64, params, delta):
    """per frame the two decision margins of the float64 restatement: e[i] - max of the REST of its window (inf when the
    window holds nothing else), and e[i] - mean - delta"""
    pre_max, post_max, pre_avg, post_avg, _ = params
    e = np.asarray(e64, np.float64)
    n = len(e)
    m1, m2 = np.full(n, np.inf), np.zeros(n)
    for i in range(n):
        a, b = windows(i, n, pre_max, post_max)
        rest = np.delete(e[a:b + 1], i - a)
        if len(rest):
            m1[i] = e[i] - rest.max()
        a, b = windows(i, n, pre_avg, post_avg)
        m2[i] = e[i] - e[a:b + 1].sum() / (b - a + 1) - float(np.float32(delta))
    return m1, m2
