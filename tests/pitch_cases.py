"""Inputs and parameter sets of the YIN fixture (tests/golden/pitch_yin.npz), generated from seeds so that only the
reference's outputs are stored.  A case: name -> (samplate, low_fre, high_fre, radix2_exp, slide_length, auto_length, thresh,
signal kind, samples)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _n(r, hop, frames, extra=0):
    return (1 << r) + hop * (frames - 1) + extra


# name: (samplate, low_fre, high_fre, radix2_exp, slide_length, auto_length, thresh, signal, data_length)
CASES = {
    # signals at the wrapper's sizes
    "tone55_r12": (32000, 27.0, 2000.0, 12, 1024, 2048, 0.1, "tone:55", _n(12, 1024, 4)),
    "tone440_r12": (32000, 27.0, 2000.0, 12, 1024, 2048, 0.1, "tone:440", _n(12, 1024, 4)),
    "tone1900_r11": (32000, 27.0, 2000.0, 11, 512, 1024, 0.1, "tone:1900", _n(11, 512, 6)),
    "tone220_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "tone:220", _n(10, 256, 10)),
    "stack_r11": (32000, 27.0, 2000.0, 11, 512, 1024, 0.1, "stack:196", _n(11, 512, 8)),
    "glide_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "glide", _n(10, 256, 24)),
    "bursts_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "bursts", _n(10, 256, 30)),
    "snr20_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "snr:20", _n(10, 256, 12)),
    "snr5_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "snr:5", _n(10, 256, 12)),
    "snr0_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.3, "snr:0", _n(10, 256, 12)),
    "zero_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "zero", _n(10, 256, 5)),
    "tiny_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "tiny", _n(10, 256, 12)),
    "step_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.1, "step", _n(10, 256, 10)),
    # parameters
    "r8": (16000, 100.0, 2000.0, 8, 64, 128, 0.1, "tone:440", _n(8, 64, 20)),
    "r9": (16000, 60.0, 2000.0, 9, 128, 256, 0.1, "tone:330", _n(9, 128, 16)),
    "r13": (44100, 27.0, 2000.0, 13, 2048, 4096, 0.1, "stack:82", _n(13, 2048, 3)),
    "oddhop_r10": (16000, 27.0, 2000.0, 10, 333, 512, 0.1, "glide", _n(10, 333, 14, 77)),
    "bighop_r8": (16000, 100.0, 2000.0, 8, 300, 128, 0.1, "glide", _n(8, 300, 14, 11)),
    "auto0_r9": (16000, 40.0, 2000.0, 9, 128, 0, 0.1, "tone:330", _n(9, 128, 8)),
    "autobig_r10": (16000, 27.0, 2000.0, 10, 256, 1024 - 60, 0.1, "tone:880", _n(10, 256, 8)),
    "thresh005_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.05, "snr:20", _n(10, 256, 12)),
    "thresh03_r10": (16000, 27.0, 2000.0, 10, 256, 512, 0.3, "stack:196", _n(10, 256, 12)),
    "sr8k_r10": (8000, 27.0, 2000.0, 10, 256, 512, 0.1, "tone:110", _n(10, 256, 8)),
    "sr44k_r11": (44100, 50.0, 1500.0, 11, 512, 1024, 0.1, "tone:261.63", _n(11, 512, 8)),
}


def signal(kind, n, sr, seed=0):
    rng = np.random.default_rng(4000 + seed)
    t = np.arange(n) / float(sr)
    if kind.startswith("tone:"):
        x = 0.5 * np.sin(2 * np.pi * float(kind[5:]) * t + 0.3)
    elif kind.startswith("stack:"):  # harmonics with a weak fundamental
        f0 = float(kind[6:])
        x = sum(a * np.sin(2 * np.pi * f0 * h * t + 0.7 * h) for h, a in ((1, 0.03), (2, 0.3), (3, 0.25), (4, 0.12), (5, 0.08)))
    elif kind == "glide":
        f = 150.0 * (4.0 ** (t / max(t[-1], 1e-9)))
        x = 0.4 * np.sin(2 * np.pi * np.cumsum(f) / sr)
    elif kind == "bursts":  # voiced / unvoiced alternation
        x = 0.4 * np.sin(2 * np.pi * 246.94 * t) + 0.1 * np.sin(2 * np.pi * 493.88 * t)
        noise = 0.3 * rng.standard_normal(n)
        gate = (np.arange(n) // 1500) % 2 == 1
        x = np.where(gate, noise, x)
    elif kind.startswith("snr:"):
        tone = np.sin(2 * np.pi * 311.13 * t)
        x = 0.3 * (tone + rng.standard_normal(n) * np.sqrt(0.5) * 10.0 ** (-float(kind[4:]) / 20.0))
    elif kind == "zero":
        x = np.zeros(n)
    elif kind == "tiny":  # energies around the 1e-6 snap
        x = 1e-4 * np.sin(2 * np.pi * 220.0 * t) + 2e-6 * rng.standard_normal(n)
    elif kind == "step":  # a full-scale stretch next to silence
        x = np.where((np.arange(n) > n // 3) & (np.arange(n) < n // 2), np.sin(2 * np.pi * 523.25 * t), 0.0)
    elif kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def case_input(name):
    sr, lo, hi, r, hop, auto, thresh, kind, n = CASES[name]
    return signal(kind, n, sr, seed=sorted(CASES).index(name))


def plan(sr, lo, hi, r, hop, auto):
    """minIndex, maxIndex, yinLength, mLen of a VALID parameter set (float32 like the constructor)"""
    N = 1 << r
    mn = int(np.floor(np.float32(sr) / np.float32(hi)))
    mx = min(int(np.ceil(np.float32(sr) / np.float32(lo))), N - auto - 1)
    return mn, mx, mx - mn + 1, (mx - mn + 1) // 2 + 1


def frames(n, r, hop):
    N = 1 << r
    return 0 if n < N else (n - N) // hop + 1
