"""Inputs and parameter sets of the PEF pitch fixture (tests/golden/pitch_pef.npz), generated from seeds so that only outputs
are stored.  A case: name -> (samplate, low_fre, high_fre, cut_fre, radix2_exp, slide_length, window_type, alpha, beta,
gamma, signal kind, samples).  Signals are those of tests/pitch_cases.py.  With N = 2^radix2_exp the cases cover N = 64 ...
4096 (one case at the default size), odd hops and hops above N, both branches of the last log frequency (cutFre below and
above samplate / 2), an odd samplate, filterPadNum = 0 (beta 1), 0 < P < N and P = N (alpha + beta < 1), three windows,
narrow and wide candidate ranges, and the signal kinds tone, stack, glide, snr:20, snr:5, noise, step and zero.
The Hann window goes with noisy signals only (tests/pitch_hs_cases.py says why)."""
import ctypes as C
import os

import numpy as np

from tests.pitch_cases import signal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECT, HANN, HAMM, BARTLETT = 0, 1, 2, 5


def _n(r, hop, frames, extra=0):
    return (1 << r) + hop * (frames - 1) + extra


# name: (samplate, low_fre, high_fre, cut_fre, radix2_exp, slide_length, window, alpha, beta, gamma, signal, data_length)
CASES = {
    "r6_sr8k": (8000, 32.0, 2000.0, 4000.0, 6, 16, HAMM, 10.0, 0.5, 1.8, "tone:440", _n(6, 16, 3)),
    "r8_stack": (16000, 60.0, 2000.0, 4000.0, 8, 64, HAMM, 10.0, 0.5, 1.8, "stack:196", _n(8, 64, 6)),
    "r9_oddhop": (16000, 40.0, 2000.0, 4000.0, 9, 133, HANN, 10.0, 0.5, 1.8, "snr:20", _n(9, 133, 8, 77)),
    "r10_bighop": (16000, 32.0, 2000.0, 4000.0, 10, 1300, HAMM, 10.0, 0.5, 1.8, "glide", _n(10, 1300, 5, 11)),
    "r11_sr44k": (44100, 50.0, 1500.0, 30000.0, 11, 512, HAMM, 10.0, 0.5, 1.8, "tone:261.63", _n(11, 512, 5)),  # fre1 = 22049
    "r12_default": (32000, 32.0, 2000.0, 4000.0, 12, 1024, HAMM, 10.0, 0.5, 1.8, "stack:110", _n(12, 1024, 4)),
    "oddsr_r8": (22051, 60.0, 2000.0, 4000.0, 8, 77, HAMM, 10.0, 0.5, 1.8, "tone:330", _n(8, 77, 6, 3)),  # samplate / 2 rounds
    "p0_beta1_r9": (16000, 32.0, 2000.0, 4000.0, 9, 128, HAMM, 10.0, 1.0, 1.8, "tone:330", _n(9, 128, 6)),  # P = 0
    "pN_r8": (16000, 60.0, 2000.0, 4000.0, 8, 64, HAMM, 0.3, 0.5, 1.8, "glide", _n(8, 64, 6)),  # alpha + beta < 1: P = N
    "bartlett_r9": (16000, 40.0, 2000.0, 4000.0, 9, 128, BARTLETT, 10.0, 0.5, 1.8, "snr:5", _n(9, 128, 6)),
    "rect_r8": (16000, 60.0, 2000.0, 4000.0, 8, 64, RECT, 10.0, 0.5, 1.8, "noise", _n(8, 64, 6)),
    "narrow_r10": (16000, 100.0, 400.0, 4000.0, 10, 256, HAMM, 10.0, 0.5, 1.8, "tone:220", _n(10, 256, 5)),
    "wide_cut_r10": (16000, 27.0, 3900.0, 7990.0, 10, 256, HAMM, 10.0, 0.5, 1.3, "step", _n(10, 256, 10)),  # cutFre near samplate / 2
    "zero_r9": (16000, 32.0, 2000.0, 4000.0, 9, 128, HAMM, 10.0, 0.5, 1.8, "zero", _n(9, 128, 3)),
    "noise_r11": (32000, 32.0, 2000.0, 4000.0, 11, 512, HAMM, 10.0, 0.5, 1.8, "noise", _n(11, 512, 4)),
}
# the smallest case of each class: what the emulated kernel runs
SMALL = ("r6_sr8k", "r8_stack", "p0_beta1_r9", "pN_r8", "zero_r9", "r9_oddhop")
# cases whose float64 curves and float32 tables are stored in the fixture
CURVES = ("r6_sr8k", "pN_r8", "p0_beta1_r9", "rect_r8")


def case_input(name):
    c = CASES[name]
    return signal(c[10], c[11], c[0], seed=200 + sorted(CASES).index(name))


def ctor_args(name):
    """the constructor's arguments of a case, in its order"""
    return CASES[name][:10]


def frames(n, r, hop):
    N = 1 << r
    return 0 if n < N else (n - N) // hop + 1


# ---- ctypes bindings shared by the library under test and the compiled reference (same entry points) ----------------------
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


class Plan(C.Structure):
    """AfxPitchPefPlan (include/mir/_pitch_pef.h)"""
    _fields_ = [(n, C.c_int) for n in ("samplate", "radix2Exp", "fftLength", "slideLength", "isContinue", "windowType")] + \
               [(n, C.c_float) for n in ("lowFre", "highFre", "cutFre", "alpha", "beta", "gamma")] + \
               [(n, C.c_int) for n in ("minIndex", "maxIndex", "filterPadNum", "logLength", "refXcorrLength", "corrLength", "pwLength")] + \
               [("ldsBytes", C.c_longlong)] + [(n, fp) for n in ("lg", "bw", "h", "window")]


def bind(lib):
    lib.pitchPEFObj_new.restype = C.c_int
    lib.pitchPEFObj_new.argtypes = [C.POINTER(C.c_void_p), ip, fp, fp, fp, ip, ip, ip, fp, fp, fp, ip]
    lib.pitchPEFObj_calTimeLength.restype, lib.pitchPEFObj_calTimeLength.argtypes = C.c_int, [C.c_void_p, C.c_int]
    lib.pitchPEFObj_setFilterParams.restype = None
    lib.pitchPEFObj_setFilterParams.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
    lib.pitchPEFObj_pitch.restype, lib.pitchPEFObj_pitch.argtypes = None, [C.c_void_p, fp, C.c_int, fp]
    lib.pitchPEFObj_free.restype, lib.pitchPEFObj_free.argtypes = None, [C.c_void_p]
    return lib


def bind_device(lib):
    """the additive calls of include/mir/_pitch_pef.h"""
    bind(lib)
    ll = C.c_longlong
    lib.pitchPEFObj_pitchBatchDevice.restype = C.c_int
    lib.pitchPEFObj_pitchBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p, ll, C.c_void_p]
    lib.pitchPEFObj_curveBatchDevice.restype = C.c_int
    lib.pitchPEFObj_curveBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p]
    for g in ("minIndex", "maxIndex", "filterPadNum", "logLength"):
        f = getattr(lib, f"pitchPEFObj_{g}")
        f.restype, f.argtypes = C.c_int, [C.c_void_p]
    bind_plan(lib)
    return lib


def bind_plan(lib):
    lib.afx_pitch_pef_plan_host.restype = C.c_int
    lib.afx_pitch_pef_plan_host.argtypes = [ip, fp, fp, fp, ip, ip, ip, fp, fp, fp, ip, C.POINTER(Plan)]
    lib.afx_pitch_pef_plan_free.restype, lib.afx_pitch_pef_plan_free.argtypes = None, [C.POINTER(Plan)]
    return lib


def _opt(v, t):
    return None if v is None else C.byref(t(v))


def _args(sr, lo, hi, cut, r, hop, window, alpha, beta, gamma, cont):
    i, f = C.c_int, C.c_float
    return (_opt(sr, i), _opt(lo, f), _opt(hi, f), _opt(cut, f), _opt(r, i), _opt(hop, i), _opt(window, i), _opt(alpha, f),
            _opt(beta, f), _opt(gamma, f), _opt(cont, i))


def new(lib, sr=None, lo=None, hi=None, cut=None, r=None, hop=None, window=None, alpha=None, beta=None, gamma=None, cont=None):
    obj = C.c_void_p()
    st = lib.pitchPEFObj_new(C.byref(obj), *_args(sr, lo, hi, cut, r, hop, window, alpha, beta, gamma, cont))
    return st, obj


def plan(lib, sr=None, lo=None, hi=None, cut=None, r=None, hop=None, window=None, alpha=None, beta=None, gamma=None, cont=None):
    """afx_pitch_pef_plan_host -> status, dict of the scalar fields and COPIES of the four tables (None after -100)"""
    p = Plan()
    st = lib.afx_pitch_pef_plan_host(*_args(sr, lo, hi, cut, r, hop, window, alpha, beta, gamma, cont), C.byref(p))
    d = {n: getattr(p, n) for n, _ in Plan._fields_[:20]}
    N = p.fftLength
    for n, size in (("lg", 2 * N), ("bw", 2 * N), ("h", N), ("window", N)):
        ptr = getattr(p, n)
        d[n] = np.ctypeslib.as_array(ptr, (size,)).copy() if ptr else None
    lib.afx_pitch_pef_plan_free(C.byref(p))
    return st, d


def lin_table(sr, N):
    """__vlinspace(0, samplate / 2, N + 1) in float32: start + i * step"""
    step = np.float32(sr // 2) / np.float32(N)
    return (np.float32(0) + np.arange(N + 1, dtype=np.float32) * step).astype(np.float32)


def call(lib, obj, x, fill=np.nan):
    """one pitch call on an existing object -> fre (entries the call left alone keep `fill`)"""
    x = np.ascontiguousarray(x, np.float32)
    T = lib.pitchPEFObj_calTimeLength(obj, len(x))
    fre = np.full(max(T, 0), fill, np.float32)
    lib.pitchPEFObj_pitch(obj, x.ctypes.data_as(fp), len(x), fre.ctypes.data_as(fp))
    return fre


def run_case(lib, name):
    st, obj = new(lib, *ctor_args(name))
    assert st == 0 and obj, (name, st)
    fre = call(lib, obj, case_input(name))
    lib.pitchPEFObj_free(obj)
    return fre


# ---- the compiled reference only: what its object holds (plain data it wrote while it ran; x86-64 layout of
# struct OpaquePitchPEF) ---------------------------------------------------------------------------------------------------
def ref_fields(obj):
    ints = C.cast(obj, C.POINTER(C.c_int * 29)).contents
    return {"isContinue": ints[0], "fftLength": ints[6], "slideLength": ints[7], "radix2Exp": ints[8], "xcorrFFTLength": ints[9],
            "timeLength": ints[10], "minIndex": ints[11], "maxIndex": ints[12], "filterPadNum": ints[28]}


def _ref_array(obj, byte, n):
    ptr = C.cast(obj.value + byte, C.POINTER(C.c_void_p)).contents.value
    return np.ctypeslib.as_array(C.cast(ptr, fp), (n,))


def ref_tables(obj):
    """window, lin, lg, bw, h as the reference built them (copies)"""
    N = ref_fields(obj)["fftLength"]
    return {"window": _ref_array(obj, 56, N).copy(), "lin": _ref_array(obj, 64, N + 1).copy(), "lg": _ref_array(obj, 72, 2 * N).copy(),
            "bw": _ref_array(obj, 80, 2 * N).copy(), "h": _ref_array(obj, 104, N).copy()}


def ref_curves(obj):
    """mXcorrArr[t, 0 ... maxIndex] of the last call: the peak pick works on a copy, the rows are intact"""
    f = ref_fields(obj)
    T, L = f["timeLength"], f["xcorrFFTLength"]
    return _ref_array(obj, 136, T * L).reshape(T, L)[:, :f["maxIndex"] + 1].copy()
