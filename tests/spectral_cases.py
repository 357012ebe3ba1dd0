"""The descriptor cases shared by the fixture generator (tests/golden/make_spectral_golden.py), the emulated-kernel test
and the GPU tests: inputs (by key into the committed golden files), edges, and per descriptor a default and one
non-default parameter set.  A parameter set is (iarg, farg) in the order of AfxSpectralRequest (include/afx_batch.h)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KINDS = ["flatness", "flux", "rolloff", "centroid", "spread", "skewness", "kurtosis", "entropy", "crest", "slope", "decrease",
         "bandwidth", "rms", "energy", "hfc", "sd", "sf", "mkl", "pd", "wpd", "nwpd", "cd", "rcd", "broadband", "novelty",
         "eef", "eer", "max", "mean", "var"]
KIND = {k: i for i, k in enumerate(KINDS)}
PHASE_KINDS = ("pd", "wpd", "nwpd", "cd", "rcd")
TWO_SLOT = ("max", "mean", "var")
FRAME_KINDS = ("flux", "sd", "sf", "mkl", "broadband", "novelty") + PHASE_KINDS
ROW_KINDS = tuple(k for k in KINDS if k not in FRAME_KINDS)
# sums with cancellation (band width: odd p) or long sequential float32 sums in the reference (energy, hfc): where the
# reference itself is furthest from float64 (every sum is judged by max(1e-5, 3 |reference - float64|), the rule of
# tests/test_cepstrogram_gpu.py; these get the wider fixed bars where no reference is at hand)
CANCELLING = ("skewness", "slope", "decrease", "bandwidth", "energy", "hfc")
# outputs decided by a comparison: may differ from the reference on frames where float64 puts the decision on the edge
DISCRETE = ("rolloff", "broadband")

# name -> (kind, iarg, farg)
PARAMS = {
    "flatness": ("flatness", (), ()),
    "flux": ("flux", (1, 0, 0, 0), (1.0,)),                 # step, isPostive, isExp, type / p
    "flux_s2_p2_pos_exp_mean": ("flux", (2, 1, 1, 1), (2.0,)),
    "rolloff": ("rolloff", (), (0.95,)),
    "rolloff_085": ("rolloff", (), (0.85,)),
    "centroid": ("centroid", (), ()),
    "spread": ("spread", (), ()),
    "skewness": ("skewness", (), ()),
    "kurtosis": ("kurtosis", (), ()),
    "entropy": ("entropy", (0,), ()),
    "entropy_norm": ("entropy", (1,), ()),
    "crest": ("crest", (), ()),
    "slope": ("slope", (), ()),
    "decrease": ("decrease", (), ()),
    "bandwidth": ("bandwidth", (), (2.0,)),
    "bandwidth_p3": ("bandwidth", (), (3.0,)),
    "rms": ("rms", (), ()),
    "energy": ("energy", (0,), (10.0,)),
    "energy_log_g5": ("energy", (1,), (5.0,)),
    "hfc": ("hfc", (), ()),
    "sd": ("sd", (1, 0), ()),
    "sd_s2_pos": ("sd", (2, 1), ()),
    "sf": ("sf", (1, 0), ()),
    "sf_s5_pos": ("sf", (5, 1), ()),
    "mkl": ("mkl", (0,), ()),
    "mkl_mean": ("mkl", (1,), ()),
    "pd": ("pd", (), ()),
    "wpd": ("wpd", (), ()),
    "nwpd": ("nwpd", (), ()),
    "cd": ("cd", (), ()),
    "rcd": ("rcd", (), ()),
    "broadband": ("broadband", (), (0.0,)),
    "broadband_3db": ("broadband", (), (3.0,)),
    "novelty": ("novelty", (1, 0, 0), (0.0,)),              # step, methodType, dataType / threshold
    "novelty_s2_kl": ("novelty", (2, 2, 0), (0.1,)),
    "novelty_is": ("novelty", (1, 3, 0), (0.0,)),
    "novelty_entroy_number": ("novelty", (1, 1, 1), (0.05,)),
    "eef": ("eef", (0,), ()),
    "eef_norm": ("eef", (1,), ()),
    "eer": ("eer", (0,), (1.0,)),
    "eer_norm_g10": ("eer", (1,), (10.0,)),
    "max": ("max", (), ()),
    "mean": ("mean", (), ()),
    "var": ("var", (), ()),
}


def request_tuple(name):
    kind, iarg, farg = PARAMS[name]
    return KIND[kind], tuple(iarg) + (0,) * (4 - len(iarg)), tuple(farg) + (0.0,) * (2 - len(farg))


def inputs():
    """name -> (spec [T, num], phase or None, fre [num])"""
    bft = np.load(os.path.join(GOLDEN, "bft.npz"))
    sg = np.load(os.path.join(GOLDEN, "spectrogram.npz"))
    st = np.load(os.path.join(GOLDEN, "stft.npz"))
    re, im = st["pad_center_zero_2048/re"][:, :1025], st["pad_center_zero_2048/im"][:, :1025]
    long_mag = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(np.float32)
    long_ang = np.arctan2(im.astype(np.float64), re.astype(np.float64)).astype(np.float32)
    return {
        "mel128_power": (np.ascontiguousarray(bft["cfg1_mel_power/re"]), None, bft["cfg1_mel_power/fre"].astype(np.float32)),
        "bark64_mag": (np.ascontiguousarray(sg["bark64_mag_norm/spec"]), None, sg["bark64_mag_norm/fre"].astype(np.float32)),
        "linear257": (np.ascontiguousarray(sg["linear_default/spec"]), np.ascontiguousarray(sg["linear_default/phase"]),
                      sg["linear_default/fre"].astype(np.float32)),
        "stft1025": (long_mag, long_ang, (np.arange(1025) * (32000.0 / 2048)).astype(np.float32)),
    }


def edges(num):
    """name -> None (full range) | (start, end) | index list (9 entries, unsorted)"""
    pick = np.array([7, 3, 11, 5, 2, 9, 4, 13, 6]) * (num - 1) // 13
    return {"full": None, "edge": (5, num - 28), "list": [int(v) for v in pick]}


def edge_indices(num, edge):
    if edge is None:
        return np.arange(num)
    if isinstance(edge, tuple):
        return np.arange(edge[0], edge[1] + 1)
    return np.asarray(edge, dtype=np.int64)


def names_for(phase):
    return [n for n, (k, _, _) in PARAMS.items() if phase is not None or k not in PHASE_KINDS]
