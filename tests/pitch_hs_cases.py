"""Inputs and parameter sets of the HPS / LHS pitch fixture (tests/golden/pitch_hs.npz), generated from seeds so that only
outputs are stored.  A case: name -> (kinds, samplate, low_fre, high_fre, radix2_exp, slide_length, window_type,
harmonic_count, signal kind, samples).  Signals are those of tests/pitch_cases.py.  With N = 2^radix2_exp and M =
roundPowerTwo(samplate) the cases cover D = M / N = 1, 2, 8, 16, 32, 64 and 128 (the many-residue loop), M below and above
the samplate, counts 1 / 5 / clamped, the windows, odd and large hops, and both placements of the spectrum slice.
The Hann window goes with noisy signals only: under it a clean synthetic signal has a spectral floor some 1e-10 of its peak,
below float32 rounding, where the reference itself turns bins into exact zeros (-inf for LHS) and is no yardstick --
tests/golden/make_pitch_hs_golden.py refuses such a case."""
import ctypes as C
import os

import numpy as np

from tests.pitch_cases import signal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HPS, LHS = 0, 1
KIND_NAME = {HPS: "HPS", LHS: "LHS"}
RECT, HANN, HAMM, BARTLETT = 0, 1, 2, 5


def _n(r, hop, frames, extra=0):
    return (1 << r) + hop * (frames - 1) + extra


BOTH = (HPS, LHS)
# name: (kinds, samplate, low_fre, high_fre, radix2_exp, slide_length, window, harmonic_count, signal, data_length)
CASES = {
    "d1_sr8k_r13": (BOTH, 8000, 32.0, 2000.0, 13, 2048, HAMM, 3, "tone:220", _n(13, 2048, 3)),
    "d2_sr16k_r13": (BOTH, 16000, 32.0, 2000.0, 13, 2048, HAMM, 5, "stack:196", _n(13, 2048, 3)),
    "d8_default_r12": (BOTH, 32000, 32.0, 2000.0, 12, 1024, HAMM, 5, "stack:110", _n(12, 1024, 4)),  # slice in LDS
    "d16_sr16k_r10": (BOTH, 16000, 32.0, 2000.0, 10, 256, RECT, 5, "glide", _n(10, 256, 12)),
    "d128_sr8k_r6": (BOTH, 8000, 32.0, 2000.0, 6, 16, HAMM, 3, "tone:440", _n(6, 16, 3)),
    "sr44k_r11": (BOTH, 44100, 50.0, 1500.0, 11, 512, HAMM, 5, "tone:261.63", _n(11, 512, 5)),  # M = 32768 < samplate
    "sr48k_r12": (BOTH, 48000, 32.0, 2000.0, 12, 1024, HAMM, 5, "glide", _n(12, 1024, 4)),
    "count1_r10": (BOTH, 16000, 32.0, 2000.0, 10, 256, HAMM, 1, "tone:330", _n(10, 256, 6)),
    "clamp_sr8k_r10": ((LHS,), 8000, 32.0, 3000.0, 10, 256, HAMM, 5, "tone:440", _n(10, 256, 5)),  # LHS: 5 -> 2; HPS refuses
    "window5_r9": (BOTH, 16000, 40.0, 2000.0, 9, 128, BARTLETT, 5, "snr:20", _n(9, 128, 6)),  # HPS: Hamm, LHS: Bartlett
    "oddhop_r10": (BOTH, 16000, 32.0, 2000.0, 10, 333, HANN, 5, "snr:20", _n(10, 333, 8, 77)),
    "bighop_r8": (BOTH, 16000, 60.0, 2000.0, 8, 300, HAMM, 4, "glide", _n(8, 300, 7, 11)),
    "scratch_r12": (BOTH, 32000, 32.0, 15000.0, 12, 1024, HAMM, 2, "noise", _n(12, 1024, 3)),  # slice in device scratch
    "zero_r10": (BOTH, 16000, 32.0, 2000.0, 10, 256, HAMM, 5, "zero", _n(10, 256, 3)),
    "step_r10": (BOTH, 16000, 32.0, 2000.0, 10, 256, HAMM, 5, "step", _n(10, 256, 10)),
    "noise_r11": (BOTH, 32000, 32.0, 2000.0, 11, 512, HAMM, 5, "noise", _n(11, 512, 4)),
}
# the smallest case of each D class and of each slice placement: what the emulated kernel runs
SMALL = ("d1_sr8k_r13", "d2_sr16k_r13", "d8_default_r12", "d16_sr16k_r10", "d128_sr8k_r6", "scratch_r12", "zero_r10")
# cases whose float64 curves are stored in the fixture
CURVES = ("d16_sr16k_r10", "d128_sr8k_r6", "count1_r10", "window5_r9")


def case_input(name):
    n, kind = CASES[name][9], CASES[name][8]
    return signal(kind, n, CASES[name][1], seed=100 + sorted(CASES).index(name))


def pairs():
    """every (case, kind)"""
    return [(name, k) for name, c in CASES.items() for k in c[0]]


def round_pow2(v):
    """util_roundPowerTwo: the nearer power of two, ties up"""
    if v < 1:
        return 1
    lo = 1 << (int(v).bit_length() - 1)
    return lo if lo == v or v - lo < 2 * lo - v else 2 * lo


def plan(kind, sr, lo, hi, r, hop, window, count):
    """what the two constructors decide for a VALID parameter set: M, minIndex, maxIndex, harmonicCount, window type"""
    M = round_pow2(sr)
    mn, mx = int(np.ceil(np.float32(lo))), int(np.floor(np.float32(hi)))
    if kind == LHS:
        k = sr // (mx + 1)
        if count > k:
            count = k or 1
    elif window > HAMM:
        window = HAMM
    return M, mn, mx, count, window


def frames(n, r, hop):
    N = 1 << r
    return 0 if n < N else (n - N) // hop + 1


# ---- ctypes bindings shared by the library under test and the compiled reference (same entry points) ----------------------
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


def bind(lib):
    for k in ("HPS", "LHS"):
        f = getattr(lib, f"pitch{k}Obj_new")
        f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_void_p), ip, fp, fp, ip, ip, ip, ip, ip]
        f = getattr(lib, f"pitch{k}Obj_calTimeLength")
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
        f = getattr(lib, f"pitch{k}Obj_pitch")
        f.restype, f.argtypes = None, [C.c_void_p, fp, C.c_int, fp]
        f = getattr(lib, f"pitch{k}Obj_free")
        f.restype, f.argtypes = None, [C.c_void_p]
    return lib


def bind_device(lib):
    """the additive calls of include/mir/_pitch_hps.h / _pitch_lhs.h"""
    bind(lib)
    ll = C.c_longlong
    for k in ("HPS", "LHS"):
        f = getattr(lib, f"pitch{k}Obj_pitchBatchDevice")
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p, ll, C.c_void_p]
        f = getattr(lib, f"pitch{k}Obj_curveBatchDevice")
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p]
        for g in ("minIndex", "maxIndex", "harmonicCount", "interpLength"):
            f = getattr(lib, f"pitch{k}Obj_{g}")
            f.restype, f.argtypes = C.c_int, [C.c_void_p]
    return lib


def _opt(v, t):
    return None if v is None else C.byref(t(v))


def new(lib, kind, sr=None, lo=None, hi=None, r=None, hop=None, window=None, count=None, cont=None):
    obj = C.c_void_p()
    st = getattr(lib, f"pitch{KIND_NAME[kind]}Obj_new")(C.byref(obj), _opt(sr, C.c_int), _opt(lo, C.c_float), _opt(hi, C.c_float),
                                                        _opt(r, C.c_int), _opt(hop, C.c_int), _opt(window, C.c_int),
                                                        _opt(count, C.c_int), _opt(cont, C.c_int))
    return st, obj


def free(lib, kind, obj):
    getattr(lib, f"pitch{KIND_NAME[kind]}Obj_free")(obj)


def cal_time_length(lib, kind, obj, n):
    return getattr(lib, f"pitch{KIND_NAME[kind]}Obj_calTimeLength")(obj, n)


def call(lib, kind, obj, x, fill=np.nan):
    """one pitch call on an existing object -> fre (entries the call left alone keep `fill`)"""
    x = np.ascontiguousarray(x, np.float32)
    T = cal_time_length(lib, kind, obj, len(x))
    fre = np.full(max(T, 0), fill, np.float32)
    getattr(lib, f"pitch{KIND_NAME[kind]}Obj_pitch")(obj, x.ctypes.data_as(fp), len(x), fre.ctypes.data_as(fp))
    return fre


def run_case(lib, name, kind):
    _, sr, lo, hi, r, hop, window, count, _, _ = CASES[name]
    st, obj = new(lib, kind, sr, lo, hi, r, hop, window, count)
    assert st == 0 and obj, (name, kind, st)
    fre = call(lib, kind, obj, case_input(name))
    free(lib, kind, obj)
    return fre


# ---- the compiled reference only: what its objects hold ------------------------------------------------------------------
# both reference structs start {int isContinue; FFTObj; int fftLength, slideLength, radix2Exp, interpFFTLength, timeLength,
# minIndex, maxIndex, harmonicCount; float *winDataArr; float *plane ...}: plain data the reference wrote while it ran
def ref_fields(obj):
    ints = C.cast(obj, C.POINTER(C.c_int * 12)).contents
    return {"isContinue": ints[0], "fftLength": ints[4], "slideLength": ints[5], "radix2Exp": ints[6], "interpLength": ints[7],
            "timeLength": ints[8], "minIndex": ints[9], "maxIndex": ints[10], "harmonicCount": ints[11]}


def ref_curves(obj, kind):
    """the curve rows [timeLength, maxIndex + 1] the reference kept for its last call (mHpsArr / mSumArr); the peak pick has
    overwritten the winner and its two neighbours with NaN (util_peakPick)"""
    f = ref_fields(obj)
    ptrs = C.cast(obj, C.POINTER(C.c_void_p * 9)).contents
    plane = ptrs[7 if kind == HPS else 8]  # byte 56: mHpsArr | mDbArr, byte 64: mSumArr
    T, M = f["timeLength"], f["interpLength"]
    a = np.ctypeslib.as_array(C.cast(plane, fp), (T, M))
    return a[:, :f["maxIndex"] + 1].copy()
