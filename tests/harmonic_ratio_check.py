"""The acceptance rule of the harmonic-ratio results, in one place (GPU tests, emulated kernel, fixture generator and
self-check); the structure is that of tests/pitch_lag_check.py.

Per frame, against the float64 restatement (tests/harmonic_ratio_restate.py), with the compiled reference's own distance from
it as the yardstick.  The reference hands out one value per frame, so

    eps = max(1e-5, 4 * |value_ref - value64| / W)                                  (reference_eps)

and the fixture stores eps per frame.  1e-5 is the project's spectrum-relative parity figure, 4 the factor of the lag check;
nothing is measured against the code under test.

weight[j] is the restatement's first-order change of g[j] when every one of the L = 2N spectrum bins moves by max|X|, so a
spectrum error of delta * max|X| per bin moves g[j] by at most delta * weight[j]:
    r[n] = (1 / L) sum_k |X_k|^2 e^{...}; d|X_k|^2 = 2 |X_k| d|X_k|, so |dr[n]| <= D = (2 / L) sum_k |X_k| max|X| for every n.
    g[j] = r[j] / s, s = sqrt(r[0] c[j] + 1e-16): |dg| <= |dr[j]| / s + |r[j]| c[j] |dr[0]| / (2 s^3)
         <= D / s (1 + |r[j]| / (2 r[0]))                                          (c[j] / s^2 <= 1 / r[0]),
    plus |g[j]| / 2 for a relative error delta of c[j] itself (the running sum is a tree on the device).
    Where the frame starts in silence c[j] is about 0 and s about 1e-8: the weight is then 1e8 D -- the reference's own
    ill-conditioning, priced, not excused.
W, the value's weight, is the sum of weight over the one or three entries the value is formed from.

 1. curve: |got[j] - g64[j]| <= eps * weight[j]; entries that are exact zeros in the restatement (at and below minIndex, and a
    silent frame's) must be equal.
 2. a frame whose first (the minIndex it used) and lag equal the restatement's: |value - value64| <= eps * W.  The
    restatement is evaluated with the minIndex the frame inherits from the chain of the results under test, so one accepted
    difference does not count again in every frame that inherits it.
 3. a frame where either differs is "explained" only when
      lag:   the restatement separates the two candidates by at most eps * (weight[a] + weight[b]);
      first: |r[j]| or |r[j - 1]| is at most eps * D at a disputed crossing j (the one claimed and, if the restatement has
             one of its own, that one): only there can a float32 evaluation see another sign;
    at most `cap` frames of a case (1 % of its frames, at least one; tests/harmonic_ratio_cases.cap), anything else fails.
 4. silent frames and empty ranges are exact zeros (W = 0); no output is NaN or Inf where the restatement's is finite.
Without lag / first (the host-pointer call and the reference return values only) the restatement's own decisions are taken
and rule 2 applies.  Returns the worst figures for the parity log."""
import numpy as np

from tests import harmonic_ratio_restate as hr

FLOOR = 1e-5
FACTOR = 4.0


def reference_eps(f, ref_value):
    if not (f["W"] > 0 and np.isfinite(ref_value)):
        return FLOOR
    return max(FLOOR, FACTOR * abs(float(ref_value) - f["value"]) / f["W"])


def check_curve(name, t, f, eps, got):
    """-> the worst error as a fraction of its bar"""
    c, w = f["curve"], f["weight"]
    got = np.asarray(got, np.float64)
    assert got.shape == c.shape, (name, t, got.shape, c.shape)
    assert np.isfinite(got).all(), f"{name} frame {t}: the curve has NaN / Inf"
    exact = w == 0
    assert np.array_equal(got[exact], c[exact]), f"{name} frame {t}: entries that are exact zeros in the restatement differ"
    m = ~exact
    if not m.any():
        return 0.0
    over = np.abs(got[m] - c[m]) / (eps * w[m])
    k = int(np.argmax(over))
    assert over[k] <= 1.0, (f"{name} frame {t}: curve[{np.flatnonzero(m)[k]}] off by {abs(got[m][k] - c[m][k]):.3e}: "
                            f"{over[k]:.2f} of its bar (eps {eps:.2e}, weight {w[m][k]:.3e})")
    return float(over[k])


def _near_zero(f, j, max_length, eps):
    r = f["r"]
    return 2 <= j <= max_length and min(abs(r[j]), abs(r[j - 1])) <= eps * f["D"]


def check_case(name, frames64, eps, value, max_length, lag=None, first=None, curves=None, cap=1):
    """frames64: harmonic_ratio_restate.harmonic_ratio(...); eps [T]; value [T] float32; lag / first [T] int or None;
    curves: optional [T, maxLength]"""
    T = len(frames64)
    assert len(value) == T and len(eps) == T, (name, T, len(value), len(eps))
    explained, worst_curve, worst_value, carry = [], 0.0, 0.0, 0
    for t, f in enumerate(frames64):
        e = float(eps[t])
        assert np.isfinite(value[t]), f"{name} frame {t}: value {value[t]}"
        ev, why = f, None
        if first is not None:
            own = f["own"]
            want, got = (carry if own is None else own), int(first[t])
            assert 0 <= got <= max_length - 1, (name, t, got)
            if got != want:
                disputed = [got + 1] + ([] if own is None else [own + 1])
                assert any(_near_zero(f, j, max_length, e) for j in disputed), \
                    (f"{name} frame {t}: minIndex {got} where the restatement has {want}; |r| at the disputed crossings "
                     f"{[(j, min(abs(f['r'][j]), abs(f['r'][j - 1]))) for j in disputed if 2 <= j <= max_length]}, bar {e * f['D']:.3e}")
                why = "first"
            if got != f["first"]:
                ev = dict(f, **hr.evaluate(f, max_length, got))
            carry = got
        if curves is not None:
            worst_curve = max(worst_curve, check_curve(name, t, ev, e, curves[t]))
        if lag is not None and int(lag[t]) != ev["lag"]:
            a, b = int(lag[t]), ev["lag"]
            lo = (carry if first is not None else f["first"]) + 1
            assert lo <= a < max_length and b >= 0, f"{name} frame {t}: lag {a} is no candidate's (restatement {b})"
            gap, bar = abs(ev["curve"][a] - ev["curve"][b]), e * (ev["weight"][a] + ev["weight"][b])
            assert gap <= bar, (f"{name} frame {t}: lag {a} where the restatement has {b}; it separates them by {gap:.3e}, "
                                f"bar {bar:.3e}")
            why = "lag"
        elif why is None or lag is not None:
            err, bar = abs(float(value[t]) - ev["value"]), e * ev["W"]
            assert err <= bar, (f"{name} frame {t}: value {value[t]} where the restatement has {ev['value']}: off by {err:.3e}, "
                                f"bar {bar:.3e} (eps {e:.2e}, W {ev['W']:.3e})")
            if bar > 0:
                worst_value = max(worst_value, err / bar)
        if why:
            explained.append(t)
    assert len(explained) <= cap, f"{name}: {len(explained)} of {T} frames differ: {explained[:8]}"
    return {"frames": T, "explained": len(explained), "worst_curve": worst_curve, "worst_value": worst_value}
