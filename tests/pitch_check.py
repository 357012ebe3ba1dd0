"""The acceptance rule of the YIN results, in one place (GPU tests, emulated kernel, fixture self-check).

Per frame, against the float64 restatement (tests/pitch_restate.py) with the compiled reference's own distance from it as
the yardstick: eps = max(1e-5, 4 |reference min - f64 min|) -- curve values are O(1).
 1. min(yin) and, when given, the curve: |got[k] - f64[k]| <= max(eps, 8 * 2^-23 * cond[k]) (min: k = argmin).  cond[k] is the
    restatement's condition number of yin[k] = d[L] / mean[L]: the size of the float32 terms e[0], e[L], 2 r[L] that cancel
    in d[L] -- and, weighted by |yin|, in the d's that make up the running mean -- over |mean[L]|.  At lags far below the
    period d[L] is a small difference of large sums, so the plain bar cannot hold there for ANY float32 evaluation
    (measured: a 55 Hz tone at n_fft 4096, lag 16: cond 380, error 9.4e-5 on a value of 3.0).  Around the troughs, where
    decisions are made, cond is small and eps rules.
 2. a frame whose chosen lag equals the fixture's: fre within max(1e-5, 4 eps / (|2 den| lag)) relative, den the parabola's
    curvature in the restatement (flat troughs of low pitches make the vertex ill-conditioned).
 3. a frame whose decision differs (lag, found / not found, candidate count) is accepted only when the restatement shows a
    deciding comparison with margin <= eps ("explained"); at most 1 % of a case's frames (at least one frame); anything else fails.
Frames where a correlation / energy value lies within 1e-4 (relative) of the 1e-6 snap are fragile in the same sense: a
float32 rounding flips the snap; they count as explained differences when they miss rule 1.
Returns a dict of the worst figures (worst_curve: as a fraction of its bar) for the parity log."""
import numpy as np

FLOOR = 1e-5


def value_bar(f, k, eps):
    """what a curve value at lag index k of restated frame f may be off by"""
    return max(eps, 8.0 * 2.0 ** -23 * float(f["cond"][k]))


def check_candidates(name, t, f, samplate, min_index, eps, got_fre, got_val, ref_fre, ref_val):
    """candidate lists of one frame that agree in count: the same lags, values within twice the curve's bar (both sides are float32)"""
    for gf, gv, rf, rv in zip(got_fre, got_val, ref_fre, ref_val):
        assert abs(samplate / gf - samplate / rf) < 0.75, (name, t, gf, rf)
        k = min(max(int(round(samplate / rf)) - min_index, 0), len(f["yin"]) - 1)
        assert abs(gv - rv) <= 2 * value_bar(f, k, eps), (name, t, k, gv, rv)


def check_case(name, frames64, ref, got, samplate, min_index, curve=None):
    """frames64: pitch_restate.pitch(...); ref / got: dicts with fre (0 or NaN = not found), trough, min, len (candidate counts)"""
    T = len(frames64)
    assert all(len(got[k]) == T for k in ("fre", "min")), (name, T, len(got["fre"]))
    explained, worst_min, worst_curve, worst_fre = [], 0.0, 0.0, 0.0
    for t, f in enumerate(frames64):
        ref_found = bool(np.isfinite(ref["fre"][t]) and ref["fre"][t] != 0)
        eps = max(FLOOR, 4.0 * abs(float(ref["min"][t]) - f["min"]))
        fragile = f["snap_margin"] < 1e-4
        bad = []
        e_min = abs(float(got["min"][t]) - f["min"])
        eps_min = value_bar(f, int(np.argmin(f["yin"])), eps)
        if e_min > eps_min:
            bad.append(f"min {got['min'][t]} vs {f['min']} (bar {eps_min:.2e})")
        if curve is not None:
            err = np.abs(curve[t].astype(np.float64) - f["yin"])
            over = err / np.maximum(eps, 8.0 * 2.0 ** -23 * f["cond"])
            if np.max(over) > 1.0:
                k = int(np.argmax(over))
                bad.append(f"curve[{k}] off by {err[k]:.2e} ({over[k]:.2f} of its bar, eps {eps:.2e}, cond {f['cond'][k]:.1f})")
            elif not fragile:
                worst_curve = max(worst_curve, float(np.max(over)))
        if bad:
            assert fragile, f"{name} frame {t}: " + "; ".join(bad)
            explained.append((t, "snap"))
            continue
        worst_min = max(worst_min, e_min)
        got_found = bool(got["fre"][t] != 0 and np.isfinite(got["fre"][t]))
        same = got_found == ref_found
        if same and got_found:
            lag_ref, lag_got = samplate / float(ref["fre"][t]), samplate / float(got["fre"][t])
            same = abs(lag_ref - lag_got) < 0.75 and round(lag_ref) - min_index >= 0
        if same and "len" in got and "len" in ref:
            same = int(got["len"][t]) == int(ref["len"][t])
        if not same:
            margin = f["margin_all"]
            assert margin <= eps or fragile, (f"{name} frame {t}: decision differs (got {got['fre'][t]}, reference {ref['fre'][t]}) "
                                              f"and no comparison is within {eps:.2e} (closest {margin:.2e})")
            explained.append((t, "margin"))
            continue
        if got_found:
            lag = samplate / float(ref["fre"][t])
            k = int(round(lag)) - min_index
            den = abs(2.0 * f["den"]) if f["found"] and f["k"] == k else 0.0
            bar = max(FLOOR, 4.0 * eps / (den * lag)) if den > 0 else 1e-3
            rel = abs(float(got["fre"][t]) - float(ref["fre"][t])) / float(ref["fre"][t])
            assert rel <= bar, f"{name} frame {t}: fre {got['fre'][t]} vs {ref['fre'][t]}: {rel:.2e} > {bar:.2e}"
            worst_fre = max(worst_fre, rel)
            if got.get("trough") is not None:
                kk = min(max(k, 0), len(f["yin"]) - 1)
                assert abs(float(got["trough"][t]) - float(ref["trough"][t])) <= 2 * value_bar(f, kk, eps), (name, t, got["trough"][t], ref["trough"][t])
    assert len(explained) <= max(1, T // 100), f"{name}: {len(explained)} of {T} frames differ: {explained[:8]}"
    return {"frames": T, "explained": len(explained), "worst_min": worst_min, "worst_curve": worst_curve, "worst_fre": worst_fre}
