"""The acceptance rule of the HPS / LHS results, in one place (GPU tests, emulated kernel, fixture generator and self-check).

Per frame, against the float64 restatement (tests/pitch_hs_restate.py), with the compiled reference's own distance from it
as the yardstick.  The reference's spectrum is not handed out; its curve rows are, so

    eps = max(1e-5, 4 * max_j |curve_ref[j] - curve64[j]| / weight[j])          (reference_eps)

weight[j] being the restatement's first-order change of curve[j] when each bin it reads moves by max|X|: a spectrum error
of delta * max|X| per bin moves curve[j] by at most delta * weight[j], so eps is four times (a lower bound of) the
reference's relative spectrum error.  The fixture stores eps per frame.
 1. curve: |got[j] - curve64[j]| <= eps * weight[j].  A spectral null makes a log-sum ill-conditioned for any float32
    evaluation; that is what the weight prices.  Entries that are -inf / 0 in the restatement (silent frames) must be equal.
 2. a frame whose index equals the reference's: fre is bit-equal (an integer times a constant).
 3. a frame whose index differs is accepted only when the restatement's difference between the two candidates is within
    eps * (weight[a] + weight[b]) -- each of the two values may be off by its own bar, so that is where a float32
    evaluation can order them either way ("explained"); at most 1 % of a case's frames (at least one frame); anything
    else fails.
Returns the worst figures for the parity log: worst_curve as a fraction of its bar, and the explained frames."""
import numpy as np

FLOOR = 1e-5


def reference_eps(f, ref_curve):
    """ref_curve: the reference's float32 row (NaN where its peak pick overwrote it)"""
    c, w = f["curve"], f["weight"]
    ok = np.isfinite(ref_curve) & np.isfinite(c) & np.isfinite(w) & (w > 0)
    if not ok.any():
        return FLOOR
    return max(FLOOR, 4.0 * float(np.max(np.abs(ref_curve[ok].astype(np.float64) - c[ok]) / w[ok])))


def index_of(fre, sr, M):
    return int(round(float(fre) / (1.0 * sr / M))) - 1


def check_curve(name, t, f, eps, got):
    """-> the worst error as a fraction of its bar"""
    c, w = f["curve"], f["weight"]
    got = np.asarray(got, np.float64)
    assert got.shape == c.shape, (name, t, got.shape, c.shape)
    exact = ~np.isfinite(c) | (w == 0)
    assert np.array_equal(got[exact], c[exact]), f"{name} frame {t}: entries that are 0 / -inf in the restatement differ"
    lax = ~exact & ~np.isfinite(w)  # a bin of exactly 0 beside finite ones: no bar
    m = ~exact & ~lax
    if not m.any():
        return 0.0
    over = np.abs(got[m] - c[m]) / (eps * w[m])
    k = int(np.argmax(over))
    assert over[k] <= 1.0, (f"{name} frame {t}: curve[{np.flatnonzero(m)[k]}] off by {abs(got[m][k] - c[m][k]):.3e}: "
                            f"{over[k]:.2f} of its bar (eps {eps:.2e}, weight {w[m][k]:.3e})")
    return float(over[k])


def check_case(name, frames64, eps, ref_fre, got_fre, sr, M, curves=None):
    """frames64: pitch_hs_restate.pitch(...); eps [T]; ref_fre / got_fre [T] float32; curves: optional [T, maxIndex + 1]"""
    T = len(frames64)
    assert len(got_fre) == T and len(ref_fre) == T, (name, T, len(got_fre), len(ref_fre))
    explained, worst_curve = [], 0.0
    for t, f in enumerate(frames64):
        e = float(eps[t])
        if curves is not None:
            worst_curve = max(worst_curve, check_curve(name, t, f, e, curves[t]))
        gb, rb = np.float32(got_fre[t]).view(np.uint32), np.float32(ref_fre[t]).view(np.uint32)
        if gb == rb:
            continue
        a, b = index_of(got_fre[t], sr, M), index_of(ref_fre[t], sr, M)
        n = len(f["curve"])
        assert 0 <= a < n and 0 <= b < n and a != b, f"{name} frame {t}: fre {got_fre[t]} is no candidate's (reference {ref_fre[t]})"
        with np.errstate(invalid="ignore"):
            gap = abs(f["curve"][a] - f["curve"][b])
        bar = e * (f["weight"][a] + f["weight"][b])
        assert gap <= bar, (f"{name} frame {t}: index {a} where the reference has {b}; the restatement separates them by "
                            f"{gap:.3e}, bar {bar:.3e}")
        explained.append(t)
    assert len(explained) <= max(1, T // 100), f"{name}: {len(explained)} of {T} frames differ: {explained[:8]}"
    return {"frames": T, "explained": len(explained), "worst_curve": worst_curve}
