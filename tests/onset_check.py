"""The one acceptance rule of the onset tests (GPU, emulated kernels, drop-in) and of the fixture's generator.

Yardstick per case: eps = max(1e-5, 4 x the compiled reference's own largest distance from the float64 envelope) -- measured
from the reference, never from the code under test; the factor 4 is this project's convention (tests/pitch_pef_check.py).
  (a) envelope: |got - e64| <= eps for every frame;
  (b) points: the list is EXACTLY the float32 pick rule (tests/onset_restate.py: pick) applied to the envelope that came with
      it -- no tolerance;
  (c) the list equals the reference's.  A frame on which they differ is accepted only when the float64 restatement shows a
      decision within 2 eps -- e[i] against the rest of its window, or e[i] - mean - delta, where the other of the two
      conditions does not already rule the frame out by more than 2 eps -- at a frame i with
      i <= frame <= i + wait (what a changed point suppresses or releases downstream); at most max(1, 1 %) of the case's
      frames may be explained this way.
The generator demands zero marginal decisions of the reference itself and reference points == float64 points."""
import numpy as np

from tests import onset_restate as rs

FLOOR = 1e-5
FACTOR = 4.0


def reference_eps(e64, ref_evn):
    return max(FLOOR, FACTOR * float(np.abs(np.asarray(ref_evn, np.float64) - e64).max()))


def marginal_frames(e64, params, delta, eps):
    m1, m2 = rs.margins64(e64, params, delta)
    # a frame is a candidate when BOTH conditions hold: a condition within 2 eps of its threshold decides the frame only
    # where the other one holds or is itself within 2 eps (a run of equal values far below the mean decides nothing)
    t = 2 * eps
    return np.flatnonzero(((np.abs(m1) <= t) & (m2 >= -t)) | ((np.abs(m2) <= t) & (m1 >= -t)))


def check_case(name, e64, eps, ref_points, got_evn, got_points, params, delta):
    """-> dict(worst: largest envelope error over eps, explained: frames accepted by rule (c))"""
    got_evn = np.asarray(got_evn, np.float32)
    got_points = np.asarray(got_points, np.int64)
    err = np.abs(got_evn.astype(np.float64) - e64)
    worst = float(err.max() / eps)
    print(f"{name}: envelope error {err.max():.3e} against eps {eps:.3e}; {len(got_points)} points, reference {len(ref_points)}")
    assert np.isfinite(got_evn).all() and worst <= 1.0, f"{name}: (a) envelope {err.max():.3e} > eps {eps:.3e} at frame {err.argmax()}"
    own = rs.pick(got_evn, params, delta, np.float32)
    assert np.array_equal(own, got_points), f"{name}: (b) points {got_points.tolist()} != float32 rule on the own envelope {own.tolist()}"
    diff = sorted(set(got_points.tolist()) ^ set(np.asarray(ref_points).tolist()))
    if diff:
        marg = marginal_frames(e64, params, delta, eps)
        wait = params[4]
        for j in diff:
            assert any(i <= j <= i + wait for i in marg), f"{name}: (c) frame {j} differs from the reference with no marginal decision"
        assert len(diff) <= max(1, len(e64) // 100), f"{name}: (c) {len(diff)} frames explained"
    return {"worst": worst, "explained": len(diff)}
