"""What the resampler tests share (include/dsp/resample_algorithm.h): the case list, the inputs, a ctypes binding of
resampleObj_* that serves this library and the compiled reference alike (oracle/_ref/libaudioflux_ref.so; oracle/ref.py does
not bind the resampler), and the expected outputs -- from the compiled reference where it is present, else from
tests/golden/resample.npz (tests/golden/make_resample_golden.py)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libaudioflux_ref.so")

BEST, MID, FAST = 0, 1, 2
HANN, KAISER, GAUSS, TUKEY = 1, 4, 8, 13

# name -> how the object is made (qual: resampleObj_new; win: resampleObj_newWithWindow's zeroNum, nbit, winType, value,
# rollOff), its rates (src, tgt) or ratio, isScale, and the input samples
CASES = {
    "441_16_best": dict(qual=BEST, rates=(44100, 16000), n=6000),      # 2176 outputs: the case an exact-phase kernel fails
    "441_16_mid": dict(qual=MID, rates=(44100, 16000), n=6000),
    "441_16_fast": dict(qual=FAST, rates=(44100, 16000), n=6000),
    "48_32_best": dict(qual=BEST, rates=(48000, 32000), n=5000),
    "16_441_mid": dict(qual=MID, rates=(16000, 44100), n=4000),        # up-sampling: step = bitLength
    "32_16_fast": dict(qual=FAST, rates=(32000, 16000), n=4001),       # odd length, the exact ratio 1/2 (the birth state)
    "ratio_best": dict(qual=BEST, ratio=0.7123, n=5000),
    "2205_16_best": dict(qual=BEST, rates=(22050, 16000), n=300000),   # t reaches 3e5: float32 phase steps of 1/32; n > 2^18
    "short_best": dict(qual=BEST, rates=(44100, 16000), n=40),         # 176 taps a side: every output is cut at both ends
    "short_up": dict(qual=FAST, rates=(16000, 44100), n=40),
    "one_up": dict(qual=MID, rates=(16000, 44100), n=1),               # 2 outputs of 1 sample
    "one_down": dict(qual=MID, rates=(44100, 16000), n=1),             # 0 outputs
    "441_16_fast_scale": dict(qual=FAST, rates=(44100, 16000), n=6000, scale=1),
    "16_441_mid_scale": dict(qual=MID, rates=(16000, 44100), n=4000, scale=1),
    "hann_16_5": dict(win=(16, 5, HANN, None, 0.945), rates=(44100, 16000), n=3000),   # 513 entries
    "hann_80_9": dict(win=(80, 9, HANN, None, 0.945), rates=(44100, 16000), n=3000),   # 40961 entries: above the LDS limit
    "gauss_24_7": dict(win=(24, 7, GAUSS, 3.0, 0.9), rates=(48000, 16000), n=3000),
    "tukey_24_7": dict(win=(24, 7, TUKEY, 0.4, 0.9), rates=(48000, 44100), n=3000),
}
# the cases whose full output is too large for the fixture: a selection of output indices is kept
LONG = ("2205_16_best",)
# the emulated kernel (one host thread per lane) runs these
SMALL = ("441_16_best", "32_16_fast", "short_best", "one_up", "one_down", "hann_80_9")  # (the last: the table in global memory)
PIECES = (1000, 37, 4411)  # streaming: 44100 -> 16000 with isContinue


def signal(n, seed=0):
    """n float32 samples in -1 ... 1: three tones and hashed noise, from integer arithmetic and sin alone"""
    i = np.arange(n, dtype=np.uint64)
    h = (i + np.uint64(seed * 7919 + 1)) * np.uint64(2654435761) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    noise = h.astype(np.float64) / float(1 << 32) - 0.5
    t = np.arange(n, dtype=np.float64)
    x = 0.4 * np.sin(0.031 * t + seed) + 0.25 * np.sin(0.37 * t) + 0.15 * np.sin(1.9 * t + 0.5 * seed) + 0.3 * noise
    return x.astype(np.float32)


def case_input(name):
    return signal(CASES[name]["n"], seed=sorted(CASES).index(name))


def selection(length):
    """output indices of a LONG case the fixture keeps: both ends, the middle and every 61st"""
    idx = np.concatenate([np.arange(0, 4096), np.arange(length // 2, length // 2 + 4096), np.arange(length - 4096, length),
                          np.arange(0, length, 61)])
    return np.unique(idx[(idx >= 0) & (idx < length)])


class Plan(C.Structure):
    """AfxResamplePlan"""
    _fields_ = [("zeroNum", C.c_int), ("nbit", C.c_int), ("bitLength", C.c_int), ("interpLength", C.c_int), ("winType", C.c_int),
                ("value", C.c_float), ("rollOff", C.c_float), ("isScale", C.c_int), ("isContinue", C.c_int), ("ratio", C.c_float),
                ("p", C.c_int), ("q", C.c_int), ("sourceRate", C.c_int), ("targetRate", C.c_int), ("step", C.c_int), ("taps", C.c_int),
                ("tableInLds", C.c_int), ("group", C.c_int), ("ldsBytes", C.c_longlong), ("table", C.POINTER(C.c_float))]

    def values(self):
        return np.ctypeslib.as_array(self.table, shape=(self.interpLength,)).copy()


def bind(lib, device=True):
    """argument types of resampleObj_* (the reference exports the same names) and, with `device`, of this library's
    additive calls"""
    P, I, F, V = C.POINTER, C.c_int, C.c_float, C.c_void_p
    lib.resampleObj_new.restype, lib.resampleObj_new.argtypes = I, [P(V), P(I), P(I), P(I)]
    lib.resampleObj_newWithWindow.restype = I
    lib.resampleObj_newWithWindow.argtypes = [P(V), P(I), P(I), P(I), P(F), P(F), P(I), P(I)]
    lib.resampleObj_calDataLength.restype, lib.resampleObj_calDataLength.argtypes = I, [V, I]
    lib.resampleObj_setSamplate.restype, lib.resampleObj_setSamplate.argtypes = None, [V, I, I]
    lib.resampleObj_setSamplateRatio.restype, lib.resampleObj_setSamplateRatio.argtypes = None, [V, F]
    lib.resampleObj_enableContinue.restype, lib.resampleObj_enableContinue.argtypes = None, [V, I]
    lib.resampleObj_resample.restype, lib.resampleObj_resample.argtypes = I, [V, V, I, V]
    lib.resampleObj_free.restype, lib.resampleObj_free.argtypes = None, [V]
    if device:
        lib.resampleObj_resampleBatchDevice.restype = I
        lib.resampleObj_resampleBatchDevice.argtypes = [V, V, I, I, C.c_longlong, V, C.c_longlong, V]
        lib.afx_resample_plan_host.restype = I
        lib.afx_resample_plan_host.argtypes = [P(I), P(I), P(I), P(I), P(F), P(F), P(I), P(I), P(Plan)]
        lib.afx_resample_plan_rate.restype, lib.afx_resample_plan_rate.argtypes = I, [P(Plan), I, I, F]
        lib.afx_resample_plan_length.restype, lib.afx_resample_plan_length.argtypes = I, [P(Plan), I]
        lib.afx_resample_plan_free.restype, lib.afx_resample_plan_free.argtypes = None, [P(Plan)]
    return lib


_ref = None


def ref_lib():
    """the compiled reference, or None"""
    global _ref
    if _ref is None and os.path.exists(REF_LIB):
        _ref = bind(C.CDLL(REF_LIB), device=False)
    return _ref


def _opt(ctype, v):
    return None if v is None else C.pointer(ctype(v))


def ctor_args(name, cont=0):
    """(function name, arguments behind the handle) of the case's constructor"""
    c = CASES[name]
    tail = (_opt(C.c_int, c.get("scale", 0)), _opt(C.c_int, cont))
    if "qual" in c:
        return "resampleObj_new", (_opt(C.c_int, c["qual"]),) + tail
    z, nb, wt, val, ro = c["win"]
    return "resampleObj_newWithWindow", (_opt(C.c_int, z), _opt(C.c_int, nb), _opt(C.c_int, wt), _opt(C.c_float, val),
                                         _opt(C.c_float, ro)) + tail


def new(lib, name, cont=0):
    """(status, handle) of the case's object, its rates set"""
    fn, args = ctor_args(name, cont)
    obj = C.c_void_p(None)
    st = getattr(lib, fn)(C.byref(obj), *args)
    if st == 0 and obj:
        set_rates(lib, obj, CASES[name])
    return st, obj


def set_rates(lib, obj, c):
    if "rates" in c:
        lib.resampleObj_setSamplate(obj, *c["rates"])
    else:
        lib.resampleObj_setSamplateRatio(obj, c["ratio"])


def plan(lib, name, cont=0):
    """(status, Plan) of the case, its rates set: afx_resample_plan_free it"""
    fn, args = ctor_args(name, cont)
    p = Plan()
    if fn == "resampleObj_new":
        st = lib.afx_resample_plan_host(args[0], None, None, None, None, None, args[1], args[2], C.byref(p))
    else:
        st = lib.afx_resample_plan_host(None, *args, C.byref(p))
    if st == 0:
        c = CASES[name]
        if "rates" in c:
            lib.afx_resample_plan_rate(C.byref(p), c["rates"][0], c["rates"][1], 0.0)
        else:
            lib.afx_resample_plan_rate(C.byref(p), 0, 0, c["ratio"])
    return st, p


def call(lib, obj, x, fill=0.0):
    """resampleObj_resample of x into a buffer of `fill` (the reference accumulates: give it zeros): the returned values"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.full(5 * len(x) + 8, fill, np.float32)
    n = lib.resampleObj_resample(obj, x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p))
    assert 0 <= n <= len(out) - 8, n
    assert (out[n:] == np.float32(fill)).all(), "values behind the returned length were written"
    return out[:n].copy()


def run_case(lib, name):
    st, obj = new(lib, name)
    assert st == 0 and obj, (name, st)
    try:
        return call(lib, obj, case_input(name))
    finally:
        lib.resampleObj_free(obj)


def run_pieces(lib, name="441_16_best", pieces=PIECES):
    """the pieces of one signal through an isContinue object: the outputs per piece"""
    st, obj = new(lib, name, cont=1)
    assert st == 0 and obj, (name, st)
    x = signal(sum(pieces), seed=77)
    outs, at = [], 0
    for n in pieces:
        outs.append(call(lib, obj, x[at:at + n]))
        at += n
    lib.resampleObj_free(obj)
    return outs


def run_sequence(lib, qual=MID, n=3000):
    """the ratio state machine on ONE object: born at 0.5, then 16000 / 44100, 2.0, 0.7123: the output after every step"""
    x = signal(n, seed=5)
    obj = C.c_void_p(None)
    assert lib.resampleObj_new(C.byref(obj), C.pointer(C.c_int(qual)), None, None) == 0 and obj
    outs = [call(lib, obj, x)]
    for rates in ((44100, 16000), (16000, 32000), 0.7123):
        if isinstance(rates, tuple):
            lib.resampleObj_setSamplate(obj, *rates)
        else:
            lib.resampleObj_setSamplateRatio(obj, rates)
        outs.append(call(lib, obj, x))
    lib.resampleObj_free(obj)
    return outs


_gold = None


def golden():
    global _gold
    if _gold is None:
        _gold = np.load(os.path.join(GOLDEN, "resample.npz"))
    return _gold


def expected(name):
    """the reference's output of the case: (values, indices or None): the compiled reference's where it is present (all
    values), else the fixture's (a selection for the LONG cases)"""
    ref = ref_lib()
    if ref is not None:
        return run_case(ref, name), None
    g = golden()
    if name in LONG:
        return g[name + "/sel"], selection(int(g[name + "/len"]))
    return g[name + "/out"], None


def expected_pieces():
    ref = ref_lib()
    if ref is not None:
        return run_pieces(ref)
    g = golden()
    return [g[f"pieces/{k}"] for k in range(len(PIECES))]


def expected_sequence():
    ref = ref_lib()
    if ref is not None:
        return run_sequence(ref)
    g = golden()
    return [g[f"sequence/{k}"] for k in range(4)]
