"""The acceptance rule of the HPSS parity tests (GPU, emulated): 1e-5 peak- and L2-relative AGAINST THE PEAK OF THE INPUT CLIP --
an output that is legitimately almost empty (the percussive part of a chord) must not be judged against its own tiny peak.
Where the weighted overlap-add divides by a window sum near its clamp (the first and last samples under a Hann window) the
float32 rounding of one inverse transform is amplified by the condition number sum w / sum w^2: the bar there is 3e-7 x that
number, the rule of tests/conftest.py::assert_istft_parity."""
import numpy as np

from tests.conftest import HOSTSTUB, parity_log
from tests.hpss_restate import condition


def check_waveform(what, got, want, x_peak, radix2_exp, window_type, tol=1e-5):
    assert np.shape(got) == np.shape(want), f"{what}: shape {np.shape(got)} vs {np.shape(want)}"
    if HOSTSTUB:
        return 0.0
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    scale = max(float(x_peak), 1e-30)
    n_fft = 1 << radix2_exp
    t = (len(want) - n_fft) // (n_fft // 4) + 1
    cond = condition(radix2_exp, window_type, t)
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / scale
    bar = np.maximum(tol, 3e-7 * cond)
    inner = cond <= 30
    l2 = float(np.sqrt((d[inner] ** 2).sum() / max(1, inner.sum())))
    worst = float((d / bar).max()) * tol
    parity_log(what, worst, tol, "hpss: worst error / its bar over the input peak, scaled to 1e-5")
    assert (d <= bar).all(), f"{what}: {int((d > bar).sum())} samples over the bar, worst {d.max():.3e} of the input peak"
    assert l2 <= tol, f"{what}: rms error {l2:.3e} of the input peak"
    assert inner.mean() > 0.9 or len(cond) < 8 * n_fft, f"{what}: the bar is relaxed on too many samples"
    return float(d[inner].max()) if inner.any() else 0.0
