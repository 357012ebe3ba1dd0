"""The acceptance rule of the PEF results, in one place (GPU tests, emulated kernel, fixture generator and self-check).

Per frame, against the float64 restatement (tests/pitch_pef_restate.py): S = max_k |R64[k]| over 0 ... maxIndex, and the
yardstick

    eps = max(1e-5, 4 * max_k |R_ref[k] - R64[k]| / S)                            (reference_eps)

measured from the COMPILED REFERENCE's own curve (the head of its mXcorrArr row), never from the code under test; the
fixture stores it per frame.
 1. curve (when asked for): |got[k] - R64[k]| <= eps * S for every k.
 2. a frame whose index equals the reference's: fre is bit-equal (an entry of the log-frequency table).
 3. a frame whose index differs is accepted only when |R64[a] - R64[b]| <= 2 * eps * S -- each of the two values may be
    off by eps * S, so that is where a float32 evaluation can order them either way ("explained"); at most 1 % of a case's
    frames (at least one frame); anything else fails.
 4. frames with S = 0 come out as lg[minIndex] and a zero curve exactly.
Returns the worst figures for the parity log: worst_curve as a fraction of its bar, and the explained frames."""
import numpy as np

FLOOR = 1e-5


def reference_eps(f, ref_curve):
    """ref_curve: the reference's float32 row [maxIndex + 1]"""
    if f["scale"] == 0:
        return FLOOR
    return max(FLOOR, 4.0 * float(np.max(np.abs(ref_curve.astype(np.float64) - f["curve"]))) / f["scale"])


def check_curve(name, t, f, eps, got):
    """-> the worst error as a fraction of its bar"""
    c, S = f["curve"], f["scale"]
    got = np.asarray(got, np.float64)
    assert got.shape == c.shape, (name, t, got.shape, c.shape)
    if S == 0:
        assert not got.any(), f"{name} frame {t}: a silent frame's curve is not zero"
        return 0.0
    err = np.abs(got - c)
    k = int(np.argmax(err)) if np.isfinite(err).all() else int(np.flatnonzero(~np.isfinite(err))[0])
    over = err[k] / (eps * S)
    assert over <= 1.0, f"{name} frame {t}: curve[{k}] off by {err[k]:.3e}: {over:.2f} of its bar (eps {eps:.2e}, S {S:.3e})"
    return float(over)


def check_case(name, frames64, eps, ref_fre, got_fre, lg, mn, curves=None):
    """frames64: pitch_pef_restate.pitch(...); eps [T]; ref_fre / got_fre [T] float32; lg: the float32 log-frequency table;
    curves: optional [T, maxIndex + 1]"""
    T = len(frames64)
    assert len(got_fre) == T and len(ref_fre) == T, (name, T, len(got_fre), len(ref_fre))
    bits = {int(v): i for i, v in reversed(list(enumerate(lg.view(np.uint32))))}
    explained, worst_curve = [], 0.0
    for t, f in enumerate(frames64):
        e, S = float(eps[t]), f["scale"]
        if curves is not None:
            worst_curve = max(worst_curve, check_curve(name, t, f, e, curves[t]))
        gb, rb = int(np.float32(got_fre[t]).view(np.uint32)), int(np.float32(ref_fre[t]).view(np.uint32))
        if S == 0:
            assert gb == int(lg[mn].view(np.uint32)), f"{name} frame {t}: a silent frame gives {got_fre[t]}, not lg[minIndex]"
        if gb == rb:
            continue
        assert gb in bits and rb in bits, f"{name} frame {t}: fre {got_fre[t]} is no entry of the table (reference {ref_fre[t]})"
        a, b = bits[gb], bits[rb]
        n = len(f["curve"])
        assert mn <= a < n and mn <= b < n and a != b, f"{name} frame {t}: index {a} is no candidate (reference {b})"
        gap, bar = abs(f["curve"][a] - f["curve"][b]), 2 * e * S
        assert gap <= bar, (f"{name} frame {t}: index {a} where the reference has {b}; the restatement separates them by "
                            f"{gap:.3e}, bar {bar:.3e}")
        explained.append(t)
    assert len(explained) <= max(1, T // 100), f"{name}: {len(explained)} of {T} frames differ: {explained[:8]}"
    return {"frames": T, "explained": len(explained), "worst_curve": worst_curve}
