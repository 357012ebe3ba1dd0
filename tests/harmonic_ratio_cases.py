"""Inputs and parameter sets of the harmonic-ratio fixture (tests/golden/harmonic_ratio.npz), generated from seeds so that only
outputs are stored.  name -> (samplate, low_fre, radix2_exp, slide_length, signal kind, frames); the window argument is
ignored by the object, so there is none.  Signals are those of tests/pitch_cases.py with seed 500 + the row number, plus the
two kinds defined here; n = N + hop (frames - 1) + 5 samples, N = 2^radix2_exp.  The cases cover N = 64 ... 4096 (one at the
wrapper's default size), odd hops and a hop above N, an odd samplate, maxLength capped at N - 1, a range of four lags with an
empty one, frames that inherit minIndex from an earlier frame and a clip in which no frame has a crossing."""
import ctypes as C
import os

import numpy as np

from tests.pitch_cases import signal as _signal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (samplate, low_fre, radix2_exp, slide_length, signal, frames) -- in the row order of the seeds
CASES = {
    "r6_sr8k": (8000, 130.0, 6, 16, "tone:440", 3),
    "r8_stack": (16000, 64.0, 8, 64, "stack:196", 6),
    "r9_oddhop": (16000, 40.0, 9, 133, "snr:20", 8),
    "r10_bighop": (16000, 32.0, 10, 1300, "glide", 5),
    "r11_sr44k": (44100, 50.0, 11, 512, "stack:261.63", 5),
    "r12_default": (32000, 32.7, 12, 1024, "stack:110", 4),
    "noise_r8": (16000, 64.0, 8, 64, "noise", 6),
    "step_r10": (16000, 27.0, 10, 256, "step", 10),
    "zero_r9": (16000, 32.0, 9, 128, "zero", 3),
    "snr5_r9": (16000, 40.0, 9, 128, "snr:5", 6),
    "oddsr_r8": (22051, 90.0, 8, 77, "tone:330", 6),
    "tiny_r10": (16000, 27.0, 10, 256, "tiny", 6),
    "cap_r7": (16000, 20.0, 7, 32, "stack:196", 5),      # maxLength capped at N - 1
    "carry_r8": (16000, 1000.0, 8, 64, "carry", 10),     # frames that inherit minIndex
    "short_r8": (16000, 4000.0, 8, 64, "noise", 6),      # maxLength 4, one empty range
    "dc_r8": (16000, 1000.0, 8, 64, "dc", 6),            # no frame has a crossing: minIndex 0 throughout
}
NAMES = list(CASES)
# the smallest case of each class: what the emulated kernel runs
SMALL = ("r6_sr8k", "r8_stack", "carry_r8", "short_r8", "dc_r8", "zero_r9")
# explained frames a case may have (tests/harmonic_ratio_check.py): 1 % of its frames, at least one; step_r10's frames that
# start in silence are ill-conditioned for the reference itself, which departs from float64 on two of them
CAP = {"step_r10": 3}


def signal(kind, n, sr, seed=0):
    """tests/pitch_cases.signal plus `dc` (an offset larger than the sine on it: the autocorrelation never changes sign) and
    `carry` (noise, then dc, then noise again)"""
    t = np.arange(n) / float(sr)
    dc = 0.4 + 0.3 * np.sin(2 * np.pi * 60.0 * t)
    if kind == "dc":
        return dc.astype(np.float32)
    if kind == "carry":
        a = 0.3 * np.random.default_rng(4000 + seed).standard_normal(n)
        k = np.arange(n)
        x = np.where(k < n // 2 - 40, a, dc)
        return np.where(k > n - 200, a, x).astype(np.float32)
    return _signal(kind, n, sr, seed=seed)


def data_length(name):
    c = CASES[name]
    return (1 << c[2]) + c[3] * (c[5] - 1) + 5


def case_input(name):
    c = CASES[name]
    return signal(c[4], data_length(name), c[0], seed=500 + NAMES.index(name))


def ctor_args(name):
    """(samplate, low_fre, radix2_exp, window_type, slide_length): the constructor's arguments of a case, in its order"""
    c = CASES[name]
    return c[0], c[1], c[2], None, c[3]


def cap(name):
    return CAP.get(name, max(1, CASES[name][5] // 100))


def frames(n, r, hop):
    N = 1 << r
    return 0 if n < N else (n - N) // hop + 1


# ---- ctypes bindings shared by the library under test and the compiled reference (same entry points) ----------------------
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


class Plan(C.Structure):
    """AfxHarmonicRatioPlan (include/mir/harmonicRatio_algorithm.h)"""
    _fields_ = [(n, C.c_int) for n in ("samplate", "radix2Exp", "windowLength", "fftLength", "slideLength")] + \
               [("lowFre", C.c_float), ("maxLength", C.c_int), ("ldsBytes", C.c_longlong), ("window", fp)]


def bind(lib):
    lib.harmonicRatioObj_new.restype = C.c_int
    lib.harmonicRatioObj_new.argtypes = [C.POINTER(C.c_void_p), ip, fp, ip, ip, ip]
    lib.harmonicRatioObj_calTimeLength.restype, lib.harmonicRatioObj_calTimeLength.argtypes = C.c_int, [C.c_void_p, C.c_int]
    lib.harmonicRatioObj_harmonicRatio.restype, lib.harmonicRatioObj_harmonicRatio.argtypes = None, [C.c_void_p, fp, C.c_int, fp]
    lib.harmonicRatioObj_free.restype, lib.harmonicRatioObj_free.argtypes = None, [C.c_void_p]
    return lib


def bind_device(lib):
    """the additive calls of the header"""
    bind(lib)
    ll, vp = C.c_longlong, C.c_void_p
    lib.harmonicRatioObj_harmonicRatioBatchDevice.restype = C.c_int
    lib.harmonicRatioObj_harmonicRatioBatchDevice.argtypes = [vp, vp, C.c_int, C.c_int, ll, vp, vp, vp, ll, vp]
    lib.harmonicRatioObj_curveBatchDevice.restype = C.c_int
    lib.harmonicRatioObj_curveBatchDevice.argtypes = [vp, vp, C.c_int, C.c_int, ll, vp, vp]
    for g in ("maxLength", "windowLength"):
        f = getattr(lib, f"harmonicRatioObj_{g}")
        f.restype, f.argtypes = C.c_int, [vp]
    lib.afx_harmonic_ratio_plan_host.restype = C.c_int
    lib.afx_harmonic_ratio_plan_host.argtypes = [ip, fp, ip, ip, ip, C.POINTER(Plan)]
    lib.afx_harmonic_ratio_plan_free.restype, lib.afx_harmonic_ratio_plan_free.argtypes = None, [C.POINTER(Plan)]
    return lib


def _opt(v, t):
    return None if v is None else C.byref(t(v))


def _args(sr, lo, r, window, hop):
    i, f = C.c_int, C.c_float
    return (_opt(sr, i), _opt(lo, f), _opt(r, i), _opt(window, i), _opt(hop, i))


def new(lib, sr=None, lo=None, r=None, window=None, hop=None):
    obj = C.c_void_p()
    st = lib.harmonicRatioObj_new(C.byref(obj), *_args(sr, lo, r, window, hop))
    return st, obj


def plan(lib, sr=None, lo=None, r=None, window=None, hop=None):
    """afx_harmonic_ratio_plan_host -> status, dict of the scalar fields and a COPY of the window (None after -100)"""
    p = Plan()
    st = lib.afx_harmonic_ratio_plan_host(*_args(sr, lo, r, window, hop), C.byref(p))
    d = {n: getattr(p, n) for n, _ in Plan._fields_[:8]}
    d["window"] = np.ctypeslib.as_array(p.window, (p.windowLength,)).copy() if p.window else None
    lib.afx_harmonic_ratio_plan_free(C.byref(p))
    return st, d


def call(lib, obj, x, fill=np.nan):
    """one call on an existing object -> values (entries the call left alone keep `fill`)"""
    x = np.ascontiguousarray(x, np.float32)
    T = lib.harmonicRatioObj_calTimeLength(obj, len(x))
    out = np.full(max(T, 0), fill, np.float32)
    lib.harmonicRatioObj_harmonicRatio(obj, x.ctypes.data_as(fp), len(x), out.ctypes.data_as(fp))
    return out


def run_case(lib, name):
    st, obj = new(lib, *ctor_args(name))
    assert st == 0 and obj, (name, st)
    out = call(lib, obj, case_input(name))
    lib.harmonicRatioObj_free(obj)
    return out


# ---- the compiled reference only: what its object holds (plain data it wrote while it ran; x86-64 layout of
# struct OpaqueHarmonicRatio: a pointer, seven ints, padding, then the array pointers) ---------------------------------------
def ref_fields(obj):
    ints = C.cast(obj, C.POINTER(C.c_int * 9)).contents
    return {"samplate": ints[2], "fftLength": ints[3], "windowLength": ints[4], "slideLength": ints[5], "maxLength": ints[6]}


def ref_window(obj):
    ptr = C.cast(obj.value + 40, C.POINTER(C.c_void_p)).contents.value
    return np.ctypeslib.as_array(C.cast(ptr, fp), (ref_fields(obj)["windowLength"],)).copy()
