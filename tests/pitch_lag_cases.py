"""Inputs and parameter sets of the NCF / cepstrum pitch fixture (tests/golden/pitch_lag.npz), generated from seeds so that
only outputs are stored.  Both trackers run every case: name -> (samplate, low_fre, high_fre, radix2_exp, slide_length,
window_type or None for the tracker's default, signal kind, frames).  Signals are those of tests/pitch_cases.py with seed
300 + the row number, n = N + hop (frames - 1) + 5 samples.  With N = 2^radix2_exp the cases cover N = 64 ... 4096 (one case
at the default size), odd hops and a hop above N, an odd samplate, three windows, narrow and wide candidate ranges
(maxIndex <= N - 1 throughout), and the signal kinds tone, stack, glide, snr:20, snr:5, noise, step, zero and tiny.
A pure tone that is periodic in N stays away from the Rect window for CEP: its empty bins are rounding noise under a log
(tests/pitch_hs_cases.py gives the same advice for Hann)."""
import ctypes as C
import os

import numpy as np

from tests.pitch_cases import signal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECT, HANN, HAMM = 0, 1, 2
KINDS = ("NCF", "CEP")
DEFAULT_WINDOW = {"NCF": RECT, "CEP": HAMM}

# name: (samplate, low_fre, high_fre, radix2_exp, slide_length, window, signal, frames) -- in the row order of the seeds
CASES = {
    "r6_sr8k": (8000, 130.0, 2000.0, 6, 16, RECT, "tone:440", 3),
    "r8_stack": (16000, 64.0, 2000.0, 8, 64, HAMM, "stack:196", 6),
    "r9_oddhop": (16000, 40.0, 2000.0, 9, 133, HANN, "snr:20", 8),
    "r10_bighop": (16000, 32.0, 2000.0, 10, 1300, HAMM, "glide", 5),
    "r11_sr44k": (44100, 50.0, 1500.0, 11, 512, HAMM, "stack:261.63", 5),
    "r12_default": (32000, 32.0, 2000.0, 12, 1024, None, "stack:110", 4),
    "rect_r8": (16000, 64.0, 2000.0, 8, 64, RECT, "noise", 6),
    "step_r10": (16000, 27.0, 3900.0, 10, 256, HAMM, "step", 10),
    "zero_r9": (16000, 32.0, 2000.0, 9, 128, HAMM, "zero", 3),
    "snr5_r9": (16000, 40.0, 2000.0, 9, 128, HAMM, "snr:5", 6),
    "oddsr_r8": (22051, 90.0, 2000.0, 8, 77, HAMM, "tone:330", 6),
    "tiny_r10": (16000, 27.0, 2000.0, 10, 256, RECT, "tiny", 6),
}
NAMES = list(CASES)
# the smallest case of each class: what the emulated kernel runs
SMALL = ("r6_sr8k", "r8_stack", "r9_oddhop", "zero_r9", "rect_r8")
# cases whose restated float32 curves and window tables are stored in the fixture
CURVES = ("r6_sr8k", "r8_stack", "rect_r8", "oddsr_r8")


def data_length(name):
    c = CASES[name]
    return (1 << c[3]) + c[4] * (c[7] - 1) + 5


def case_input(name):
    c = CASES[name]
    return signal(c[6], data_length(name), c[0], seed=300 + NAMES.index(name))


def ctor_args(name):
    """the constructor's arguments of a case, in its order"""
    return CASES[name][:6]


def window_of(kind, name):
    w = CASES[name][5]
    return DEFAULT_WINDOW[kind] if w is None else w


def frames(n, r, hop):
    N = 1 << r
    return 0 if n < N else (n - N) // hop + 1


# ---- ctypes bindings shared by the library under test and the compiled reference (same entry points) ----------------------
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


class Plan(C.Structure):
    """AfxPitchLagPlan (include/mir/_pitch_ncf.h, include/mir/_pitch_cep.h)"""
    _fields_ = [(n, C.c_int) for n in ("samplate", "radix2Exp", "fftLength", "slideLength", "isContinue", "windowType")] + \
               [(n, C.c_float) for n in ("lowFre", "highFre")] + [(n, C.c_int) for n in ("minIndex", "maxIndex", "lagLength")] + \
               [("ldsBytes", C.c_longlong), ("window", fp)]


def fn(lib, kind, what):
    return getattr(lib, f"pitch{kind}Obj_{what}")


def bind(lib):
    for k in KINDS:
        fn(lib, k, "new").restype = C.c_int
        fn(lib, k, "new").argtypes = [C.POINTER(C.c_void_p), ip, fp, fp, ip, ip, ip, ip]
        fn(lib, k, "calTimeLength").restype, fn(lib, k, "calTimeLength").argtypes = C.c_int, [C.c_void_p, C.c_int]
        fn(lib, k, "pitch").restype, fn(lib, k, "pitch").argtypes = None, [C.c_void_p, fp, C.c_int, fp]
        fn(lib, k, "enableDebug").restype, fn(lib, k, "enableDebug").argtypes = None, [C.c_void_p, C.c_int]
        fn(lib, k, "free").restype, fn(lib, k, "free").argtypes = None, [C.c_void_p]
    return lib


def bind_plan(lib):
    for k in KINDS:
        f = getattr(lib, f"afx_pitch_{k.lower()}_plan_host")
        f.restype, f.argtypes = C.c_int, [ip, fp, fp, ip, ip, ip, ip, C.POINTER(Plan)]
        g = getattr(lib, f"afx_pitch_{k.lower()}_plan_free")
        g.restype, g.argtypes = None, [C.POINTER(Plan)]
    return lib


def bind_device(lib):
    """the additive calls of the two headers"""
    bind(lib)
    ll = C.c_longlong
    for k in KINDS:
        fn(lib, k, "pitchBatchDevice").restype = C.c_int
        fn(lib, k, "pitchBatchDevice").argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p, ll, C.c_void_p]
        fn(lib, k, "curveBatchDevice").restype = C.c_int
        fn(lib, k, "curveBatchDevice").argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p]
        for g in ("minIndex", "maxIndex"):
            fn(lib, k, g).restype, fn(lib, k, g).argtypes = C.c_int, [C.c_void_p]
    return bind_plan(lib)


def _opt(v, t):
    return None if v is None else C.byref(t(v))


def _args(sr, lo, hi, r, hop, window, cont):
    i, f = C.c_int, C.c_float
    return (_opt(sr, i), _opt(lo, f), _opt(hi, f), _opt(r, i), _opt(hop, i), _opt(window, i), _opt(cont, i))


def new(lib, kind, sr=None, lo=None, hi=None, r=None, hop=None, window=None, cont=None):
    obj = C.c_void_p()
    st = fn(lib, kind, "new")(C.byref(obj), *_args(sr, lo, hi, r, hop, window, cont))
    return st, obj


def plan(lib, kind, sr=None, lo=None, hi=None, r=None, hop=None, window=None, cont=None):
    """afx_pitch_<kind>_plan_host -> status, dict of the scalar fields and a COPY of the window (None after -100)"""
    p = Plan()
    st = getattr(lib, f"afx_pitch_{kind.lower()}_plan_host")(*_args(sr, lo, hi, r, hop, window, cont), C.byref(p))
    d = {n: getattr(p, n) for n, _ in Plan._fields_[:12]}
    d["window"] = np.ctypeslib.as_array(p.window, (p.fftLength,)).copy() if p.window else None
    getattr(lib, f"afx_pitch_{kind.lower()}_plan_free")(C.byref(p))
    return st, d


def restate_window(p):
    """the window argument of pitch_lag_restate.pitch for a plan: None for Rect"""
    return None if p["windowType"] == RECT else p["window"]


def call(lib, kind, obj, x, fill=np.nan):
    """one pitch call on an existing object -> fre (entries the call left alone keep `fill`)"""
    x = np.ascontiguousarray(x, np.float32)
    T = fn(lib, kind, "calTimeLength")(obj, len(x))
    fre = np.full(max(T, 0), fill, np.float32)
    fn(lib, kind, "pitch")(obj, x.ctypes.data_as(fp), len(x), fre.ctypes.data_as(fp))
    return fre


def run_case(lib, kind, name):
    st, obj = new(lib, kind, *ctor_args(name))
    assert st == 0 and obj, (kind, name, st)
    fre = call(lib, kind, obj, case_input(name))
    fn(lib, kind, "free")(obj)
    return fre


# ---- the compiled reference only: what its object holds (plain data it wrote while it ran; x86-64 layout of
# struct OpaquePitchNCF / OpaquePitchCEP, which are laid out alike) ---------------------------------------------------------
def ref_fields(obj):
    ints = C.cast(obj, C.POINTER(C.c_int * 11)).contents
    return {"isContinue": ints[0], "fftLength": ints[4], "slideLength": ints[5], "radix2Exp": ints[6], "lagLength": ints[7],
            "timeLength": ints[8], "minIndex": ints[9], "maxIndex": ints[10]}


def _ref_array(obj, byte, n):
    ptr = C.cast(obj.value + byte, C.POINTER(C.c_void_p)).contents.value
    return np.ctypeslib.as_array(C.cast(ptr, fp), (n,))


def ref_window(obj):
    return _ref_array(obj, 48, ref_fields(obj)["fftLength"]).copy()


def ref_curves(obj):
    """mCorrArr / mCepArr [t, 0 ... maxIndex] of the last call: the peak pick has put NaN around the index it chose"""
    f = ref_fields(obj)
    T, L = f["timeLength"], f["lagLength"]
    return _ref_array(obj, 56, T * L).reshape(T, L)[:, :f["maxIndex"] + 1].copy()
