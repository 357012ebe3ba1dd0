"""The acceptance rule of the NCF / cepstrum results, in one place (GPU tests, emulated kernel, fixture generator and
self-check); the structure is that of tests/pitch_hs_check.py.

Per frame, against the float64 restatement (tests/pitch_lag_restate.py), with the compiled reference's own distance from it
as the yardstick.  The reference's spectrum is not handed out; its curve rows (mCorrArr / mCepArr) are, so

    eps = max(1e-5, 4 * max_j |row_ref[j] - curve64[j]| / weight[j])          (reference_eps)

over the entries the reference's peak pick did not turn into NaN; the fixture stores eps per frame.  The floor and the
factor are this module's own; nothing is measured against the code under test.

weight[j] is the restatement's first-order change of curve[j] when every one of the L = 2N spectrum bins moves by max|X|, so
a spectrum error of delta * max|X| per bin moves curve[j] by at most delta * weight[j], and eps is four times (a lower bound
of) the reference's relative spectrum error:
  CEP  c[q] = (1 / L) sum_k ln|X_k|^2 e^{...}.  d ln|X_k|^2 = 2 d|X_k| / |X_k|, so |dc[q]| <= (1 / L) sum_k 2 max|X| / |X_k|
       -- the same for every q.  A weak bin makes the log ill-conditioned for any float32 evaluation: the weight prices it.
  NCF  r[n] = (1 / L) sum_k |X_k|^2 e^{...}.  d|X_k|^2 = 2 |X_k| d|X_k|, so |dr[n]| <= D = (1 / L) sum_k 2 |X_k| max|X| for
       every n, r[0] included.  c[i] = K r[i + 1] / sqrt(r[0]), K = L^(-1/4):
       |dc[i]| <= K (|dr[i + 1]| / sqrt(r[0]) + |r[i + 1]| |dr[0]| / (2 r[0]^(3/2))) <= K D / sqrt(r[0]) (1 + |r[i + 1]| / (2 r[0])).
       The entries the reference never computes (below minIndex - 1, and maxIndex) are exact zeros: weight 0.

 1. curve: |got[j] - curve64[j]| <= eps * weight[j].  Entries that are 0 or NaN in the restatement must be equal, NaN
    counting as equal to NaN.
 2. a frame whose fre equals the reference's is bit-equal (samplate / (index + 1), rounded once).
 3. a frame whose index differs is accepted only when the restatement's difference between the two candidates is within
    eps * (weight[a] + weight[b]) -- each of the two values may be off by its own bar, so that is where a float32 evaluation
    can order them either way ("explained"); at most 1 % of a case's frames (at least one frame); anything else fails.
Returns the worst figures for the parity log: worst_curve as a fraction of its bar, and the explained frames."""
import numpy as np

FLOOR = 1e-5
FACTOR = 4.0


def reference_eps(f, ref_row):
    """ref_row: the reference's float32 row (NaN where its peak pick overwrote it)"""
    c, w = f["curve"], f["weight"]
    ok = np.isfinite(ref_row) & np.isfinite(c) & np.isfinite(w) & (w > 0)
    if not ok.any():
        return FLOOR
    return max(FLOOR, FACTOR * float(np.max(np.abs(ref_row[ok].astype(np.float64) - c[ok]) / w[ok])))


def index_of(fre, sr):
    return int(round(float(sr) / float(fre))) - 1


def check_curve(name, t, f, eps, got):
    """-> the worst error as a fraction of its bar"""
    c, w = f["curve"], f["weight"]
    got = np.asarray(got, np.float64)
    assert got.shape == c.shape, (name, t, got.shape, c.shape)
    exact = np.isnan(c) | (w == 0)
    assert np.array_equal(got[exact], c[exact], equal_nan=True), f"{name} frame {t}: entries that are 0 / NaN in the restatement differ"
    m = ~exact
    if not m.any():
        return 0.0
    over = np.abs(got[m] - c[m]) / (eps * w[m])
    over = np.where(np.isnan(over), np.inf, over)  # a NaN where the restatement has a number
    k = int(np.argmax(over))
    assert over[k] <= 1.0, (f"{name} frame {t}: curve[{np.flatnonzero(m)[k]}] off by {abs(got[m][k] - c[m][k]):.3e}: "
                            f"{over[k]:.2f} of its bar (eps {eps:.2e}, weight {w[m][k]:.3e})")
    return float(over[k])


def check_case(name, frames64, eps, ref_fre, got_fre, sr, curves=None):
    """frames64: pitch_lag_restate.pitch(...); eps [T]; ref_fre / got_fre [T] float32; curves: optional [T, maxIndex + 1]"""
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
        assert np.isfinite(got_fre[t]) and got_fre[t] > 0, f"{name} frame {t}: fre {got_fre[t]}"
        a, b = index_of(got_fre[t], sr), index_of(ref_fre[t], sr)
        n = len(f["curve"])
        assert 0 <= a < n and 0 <= b < n and a != b, f"{name} frame {t}: fre {got_fre[t]} is no candidate's (reference {ref_fre[t]})"
        assert np.float32(1.0 * sr / (a + 1)).view(np.uint32) == gb, f"{name} frame {t}: fre {got_fre[t]} is not samplate / {a + 1}"
        gap = abs(f["curve"][a] - f["curve"][b])
        bar = e * (f["weight"][a] + f["weight"][b])
        assert gap <= bar, (f"{name} frame {t}: index {a} where the reference has {b}; the restatement separates them by "
                            f"{gap:.3e}, bar {bar:.3e}")  # (a NaN gap fails)
        explained.append(t)
    assert len(explained) <= max(1, T // 100), f"{name}: {len(explained)} of {T} frames differ: {explained[:8]}"
    return {"frames": T, "explained": len(explained), "worst_curve": worst_curve}
