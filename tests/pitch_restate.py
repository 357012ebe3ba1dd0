"""A float64 statement of the reference's YIN tracker (src/mir/_pitch_yin.c), independent of the library and of the kernel's
formulation: direct sums instead of transforms, every decision with the MARGINS of the comparisons that made it."""
import numpy as np

SNAP = 1e-6


def _snap(v):  # _pitch_yin.c:371-380, :398-404: values below 1e-6 in magnitude become 0
    return np.where(np.abs(v) >= SNAP, v, 0.0)


def frame_curve(x, auto, min_index, max_index):
    """one frame (float64 array of fftLength samples) -> (yin[yinLength], snap_margin, cond): the relative distance of the
    closest correlation / energy value to the 1e-6 snap, and per lag the condition of yin = d / mean:
    (m[L] + |yin| mean(m[1 .. L])) / |mean[L]| with m = e[0] + e + 2 |r|, the size of the terms that cancel in d -- in the
    numerator and, for signals whose d changes sign (autoLength near 0), in the running mean as well"""
    N = len(x)
    D = N - auto
    # _pitch_yin.c:358-369: r[j] = sum_{m = 0 .. auto} x[m] x[m + j], auto + 1 products
    r = np.array([np.dot(x[:auto + 1], x[j:j + auto + 1]) for j in range(max_index + 1)])
    # :383-405: E inclusive prefix of x^2; e[j] = E[auto + j] - E[j]: auto squares from x[j + 1] on
    E = np.cumsum(x * x)
    e = E[auto:auto + max_index + 1] - E[:max_index + 1]
    assert max_index <= D - 1
    both = np.concatenate([r, e])
    nz = both[both != 0.0]
    snap_margin = float(np.min(np.abs(np.abs(nz) - SNAP)) / SNAP) if len(nz) else 1.0
    r, e = _snap(r), _snap(e)
    d = e[0] + e - 2.0 * r  # :408-410
    # :414-448: running mean from lag 1 on; yin[k] = d[L] / (mean[L] + 1e-16), L = min_index + k
    run = np.concatenate([[0.0], np.cumsum(d[1:])])
    L = np.arange(min_index, max_index + 1)
    mean = run[L] / L
    y = d[L] / (mean + 1e-16)
    mag = abs(e[0]) + np.abs(e) + 2.0 * np.abs(r)  # the terms that cancel in d
    mag_run = np.concatenate([[0.0], np.cumsum(mag[1:])])
    cond = (mag[L] + np.abs(y) * mag_run[L] / L) / (np.abs(mean) + 1e-16)
    return y, snap_margin, cond


def offset(y, k):
    """:462-503: vertex of the parabola through k - 1, k, k + 1; 0 at the borders and when it leaves (-1, 1); also the curvature"""
    if k < 1 or k > len(y) - 2:
        return 0.0, 0.0
    num = (y[k + 1] - y[k - 1]) / 2
    den = (y[k - 1] + y[k + 1] - 2 * y[k]) / 2
    off = -num / (2 * den + 1e-16)
    return (off if abs(off) <= 1 else 0.0), den


def troughs(y, thresh):
    """:505-603: indices k <= len - 2 below thresh that are troughs, and per index the distance by which the curve would have
    to move to change its status"""
    n = len(y)
    hits, flip = [], np.empty(n - 1)
    for k in range(n - 1):
        c = [(thresh - y[k], True)]                      # y[k] < thresh
        c.append((y[k + 1] - y[k], k == 0))               # k == 0: strictly below the right neighbour; else <=
        if k > 0:
            c.append((y[k - 1] - y[k], True))             # strictly below the left neighbour
        ok = [(v > 0) if strict else (v >= 0) for v, strict in c]
        if all(ok):
            hits.append(k)
            flip[k] = min(abs(v) for v, _ in c)
        else:
            flip[k] = max(abs(v) for (v, _), o in zip(c, ok) if not o)
    return hits, flip


def frame_decision(y, thresh, samplate, min_index):
    hits, flip = troughs(y, thresh)
    out = {"hits": hits, "min": float(np.min(y)), "margin_all": float(np.min(flip))}
    if hits:
        k = hits[0]
        off, den = offset(y, k)
        out.update(found=True, k=k, fre=samplate / (min_index + k + off), value=float(y[k]), den=den,
                   margin_first=float(np.min(flip[:k + 1])))
    else:
        out.update(found=False, k=-1, fre=0.0, value=0.0, den=0.0, margin_first=float(np.min(flip)))
    out["cand_fre"] = [samplate / (min_index + k + offset(y, k)[0]) for k in hits]
    out["cand_val"] = [float(y[k]) for k in hits]
    return out


def pitch(x, samplate, r, hop, auto, min_index, max_index, thresh):
    """whole clip -> list of per-frame dicts (curve under "yin", "snap_margin", "cond", and frame_decision's entries)"""
    N = 1 << r
    x = np.asarray(x, np.float64)
    res = []
    for t in range(0 if len(x) < N else (len(x) - N) // hop + 1):
        y, sm, cond = frame_curve(x[t * hop:t * hop + N], auto, min_index, max_index)
        dct = frame_decision(y, thresh, samplate, min_index)
        dct["yin"], dct["snap_margin"], dct["cond"] = y, sm, cond
        res.append(dct)
    return res
