"""Inputs and parameter sets of the HPSS fixture (tests/golden/hpss.npz), generated from seeds so that only the reference's
outputs are stored.  A case: name -> (radix2_exp, window, h_order, p_order, signal kind, samples, which outputs, initial h)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAMM, HANN, RECT = 2, 1, 0  # WindowType values (include/flux_base.h)

# name: (radix2_exp, window_type, h_order, p_order, signal, data_length, outputs "hp" | "h" | "p", non-zero initial arrays)
CASES = {
    "mix_r8": (8, HAMM, 21, 31, "mix", 256 + 64 * 70, "hp", False),
    "mix_r10": (10, HAMM, 21, 31, "mix", 1024 + 256 * 44, "hp", False),
    "mix_r11": (11, HAMM, 21, 31, "mix", 2048 + 512 * 27, "hp", False),
    "mix_r12": (12, HAMM, 21, 31, "mix", 4096 + 1024 * 22, "hp", False),
    "mix_r10_o5_7": (10, HAMM, 5, 7, "mix", 1024 + 256 * 36, "hp", False),
    "mix_r10_o3_63": (10, HAMM, 3, 63, "mix", 1024 + 256 * 36, "hp", False),
    "mix_r10_hann": (10, HANN, 21, 31, "mix", 1024 + 256 * 30, "hp", False),
    "mix_r10_rect": (10, RECT, 21, 31, "mix", 1024 + 256 * 30, "hp", False),
    "chord_r10": (10, HAMM, 21, 31, "chord", 1024 + 256 * 30, "hp", False),
    "clicks_r10": (10, HAMM, 21, 31, "clicks", 1024 + 256 * 30, "hp", False),
    "silence_r10": (10, HAMM, 21, 31, "silence", 1024 + 256 * 10, "hp", False),
    "short_r10": (10, HAMM, 21, 31, "mix", 1024 + 256 * 8, "hp", False),      # 9 frames < hOrder
    "offgrid_r10": (10, HAMM, 21, 31, "mix", 1024 + 256 * 33 + 77, "hp", False),
    "only_h_r10": (10, HAMM, 21, 31, "mix", 1024 + 256 * 25, "h", False),
    "only_p_r10": (10, HAMM, 21, 31, "mix", 1024 + 256 * 25, "p", False),
    "accumulate_r10": (10, HAMM, 21, 31, "mix", 1024 + 256 * 25, "hp", True),
}


def signal(kind, n, seed=0, sr=16000.0):
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / sr
    chord = sum(a * np.sin(2 * np.pi * f * t + ph) for f, a, ph in ((220.0, 0.3, 0.1), (277.18, 0.25, 1.0), (329.63, 0.2, 2.0),
                                                                     (1760.0, 0.1, 0.5)))
    clicks = np.zeros(n)
    for at in range(997, n, 3001):
        m = min(24, n - at)
        clicks[at:at + m] += 0.8 * np.exp(-np.arange(m) / 4.0) * np.where(np.arange(m) % 2, -1.0, 1.0)
    noise = 0.01 * rng.standard_normal(n)
    x = {"mix": chord + clicks + noise, "chord": chord, "clicks": clicks, "silence": np.zeros(n)}[kind]
    return x.astype(np.float32)


def case_input(name):
    r, w, h, p, kind, n, outs, init = CASES[name]
    return signal(kind, n, seed=sorted(CASES).index(name))


def out_length(r, n):
    N, hop = 1 << r, (1 << r) // 4
    return ((n - N) // hop) * hop + N


def initial(name, which):
    """the content of hArr / pArr before the call (zeros unless the case tests the accumulation)"""
    r, w, h, p, kind, n, outs, init = CASES[name]
    m = out_length(r, n)
    if not init:
        return np.zeros(m, np.float32)
    return (0.05 * np.random.default_rng(77 + (which == "p")).standard_normal(m)).astype(np.float32)
