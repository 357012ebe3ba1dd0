"""float64 numpy restatement of the spectral descriptors -- the third opinion beside the compiled reference and the
kernels.  Lines cited are src/flux_spectral.c (fs) and src/feature/spectral_algorithm.c (sa) of the reference.
restate(kind, iarg, farg, spec, phase, fre, idx, num) -> list of [T] float64 arrays; margin(...) -> per frame, how close
(relative) the deciding quantity of a discrete descriptor is to its threshold."""
import numpy as np


def _diff(x, step):
    return x[step:] - x[:-step]


def restate(kind, iarg, farg, spec, phase, fre, idx, num, is_power=False):
    i, f = list(iarg) + [0] * 4, list(farg) + [0.0] * 2
    idx = np.asarray(idx)
    x = np.asarray(spec, np.float64)[:, idx]
    fr = np.asarray(fre, np.float64)[idx]
    T, n = x.shape
    S = x.sum(1)
    with np.errstate(all="ignore"):
        def guard(a, b):
            return np.where(b != 0, a / np.where(b != 0, b, 1), 0.0)
        c = guard((fr * x).sum(1), S)
        d = fr[None, :] - c[:, None]
        c2 = np.where(S != 0, np.sqrt((d * d * x).sum(1) / np.where(S != 0, S, 1)), 0.0)

        def entropy(norm):
            v = x / S[:, None]
            e = -(v * np.log2(v + 1e-16)).sum(1)
            return e / np.log2(n) if norm and np.log2(n) else (e * 0 if norm else e)
        out = np.zeros(T)
        if kind == "flatness":  # fs:21-57
            return [guard(np.exp(np.log(x + 2e-16).mean(1)), S / n)]
        if kind == "rolloff":  # fs:106-145
            cs = np.cumsum(np.abs(x), 1)
            hit = cs >= (S * f[0])[:, None]
            pos = np.where(hit.any(1), hit.argmax(1), n - 1)
            return [fr[pos]]
        if kind == "centroid":
            return [c]
        if kind == "spread":
            return [c2]
        if kind == "skewness":  # fs:203-232
            return [guard((d ** 3 * x).sum(1), c2 ** 3 * S)]
        if kind == "kurtosis":
            return [guard((d ** 4 * x).sum(1), c2 ** 4 * S)]
        if kind == "entropy":  # fs:265-294
            return [entropy(i[0])]
        if kind == "crest":
            return [guard(x.max(1), S / n)]
        if kind == "slope":  # fs:326-364
            df = fr - fr.mean()
            return [guard((df[None, :] * (x - x.mean(1)[:, None])).sum(1), (df * df).sum())]
        if kind == "decrease":  # fs:366-397: the absolute bin divides
            return [guard(((x[:, 1:] - x[:, :1]) / idx[None, 1:]).sum(1), S - x[:, 0])]
        if kind == "bandwidth":  # fs:399-432
            p = f[0]
            v = (x * d ** p).sum(1)
            return [v if p == 1 else v ** (1 / p)]
        if kind == "rms":  # fs:434-459
            w = np.where((idx == 0) | ((num % 2 == 0) & (idx == num - 1)), 0.5, 1.0)
            return [np.sqrt(2 * (x * x * w).sum(1) / (num * num))]
        if kind == "energy":  # fs:804-832
            v = x if is_power else x * x
            if i[0]:
                v = np.log(1 + (f[0] if f[0] > 0 else 10.0) * v)
            return [v.mean(1)]
        if kind == "hfc":
            return [(x * idx[None, :]).sum(1)]
        if kind in ("eef", "eer"):  # sa:781-853
            e, ent = (x * x).mean(1), entropy(i[0])
            return [np.sqrt(1 + np.abs(e * ent))] if kind == "eef" else [np.sqrt(1 + np.abs(np.log(1 + e * f[0]) / ent))]
        if kind == "max":  # sa:855-891
            return [x.max(1), fr[x.argmax(1)]]
        if kind == "mean":
            return [x.mean(1), np.full(T, fr.mean())]
        if kind == "var":
            return [((x.mean(1)[:, None] - x) ** 2).sum(1) / (n - 1), np.full(T, ((fr.mean() - fr) ** 2).sum() / (n - 1))]
        # ---- frame differences
        if kind in ("flux", "sd", "sf"):  # fs:60-104, :486-556
            step = max(i[0], 1)
            v = _diff(x, step)
            v = np.maximum(v, 0) if i[1] else np.abs(v)
            if kind == "flux":
                p = f[0]
                s = (v ** p).sum(1)
                if i[3]:
                    s = s / n
                if i[2]:
                    s = s ** (1 / p)
            else:
                s = (v * v if kind == "sf" else v).sum(1)
            out[step:] = s
            return [out]
        if kind == "mkl":  # fs:558-587
            s = np.log(1 + x[1:] / (x[:-1] + 1e-16)).sum(1)
            out[1:] = s / n if i[0] else s
            return [out]
        if kind == "broadband":  # fs:759-778
            out[1:] = (10 * np.log10(x[1:] / x[:-1]) > f[0]).sum(1)
            return [out]
        if kind == "novelty":  # fs:780-802
            step = max(i[0], 1)
            v = novelty_terms(x, step, i[1])
            hit = v > f[0]
            out[step:] = hit.sum(1) if i[2] else np.where(hit, v, 0).sum(1)
            return [out]
        ph = np.asarray(phase, np.float64)[:, idx]
        if kind in ("pd", "wpd", "nwpd"):  # fs:589-677
            v = np.abs(ph[2:] - 2 * ph[1:-1] + ph[:-2])
            if kind != "pd":
                v = v * x[2:]
            s = v.mean(1)
            if kind == "nwpd":
                s = s / (x[2:].mean(1) + 1e-16)
            out[2:] = s
            return [out]
        if kind in ("cd", "rcd"):  # fs:679-757
            z = x * np.exp(1j * ph)
            pred = np.zeros_like(z)
            pred[2:] = x[1:-1] * np.exp(1j * (2 * ph[1:-1] - ph[:-2]))
            v = np.abs(z - pred)[1:]
            if kind == "rcd":
                v = np.where(x[1:] <= x[:-1], 0, v)
            out[1:] = v.sum(1)
            return [out]
    raise ValueError(kind)


def novelty_terms(x, step, method):
    cur, pre = x[step:], x[:-step]
    with np.errstate(all="ignore"):
        if method == 0:
            return cur - pre
        r = cur / (pre + 1e-16)
        if method == 1:
            return np.log(r)
        if method == 2:
            return cur * np.log(r)
        return r - np.log(r) - 1


def margin(kind, iarg, farg, spec, idx):
    """per frame: the smallest relative distance of a deciding quantity from its threshold (inf where nothing is decided)"""
    i, f = list(iarg) + [0] * 4, list(farg) + [0.0] * 2
    x = np.asarray(spec, np.float64)[:, np.asarray(idx)]
    T = x.shape[0]
    m = np.full(T, np.inf)
    with np.errstate(all="ignore"):
        if kind == "rolloff":
            cs, thr = np.cumsum(np.abs(x), 1), (x.sum(1) * f[0])[:, None]
            m = (np.abs(cs - thr) / np.maximum(np.abs(thr), 1e-300)).min(1)
        elif kind == "broadband":
            r = x[1:] / x[:-1]
            m[1:] = np.abs(r / 10 ** (f[0] / 10) - 1).min(1)
        elif kind == "novelty":
            step = max(i[0], 1)
            v = novelty_terms(x, step, i[1])
            scale = np.maximum(np.abs(x[step:]), np.abs(x[:-step])) if i[1] in (0, 2) else 1.0
            m[step:] = (np.abs(v - f[0]) / np.maximum(scale, 1e-300)).min(1)
    return m
