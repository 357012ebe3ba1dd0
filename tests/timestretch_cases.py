"""What the time-stretch and pitch-shift tests share (include/mir/timeStretch_algorithm.h, pitchShift_algorithm.h): the case
list, the inputs (signal() of tests/resample_cases.py), a ctypes binding of timeStretchObj_* / pitchShiftObj_* / phase_vocoder
that serves this library and the compiled reference alike (oracle/_ref/libaudioflux_ref.so; oracle/ref.py does not bind
them), and the expected outputs -- from the compiled reference where it is present, else from tests/golden/timestretch.npz.
The parity bars always come from that fixture: tests/golden/make_timestretch_golden.py measures them from the reference alone."""
import ctypes as C
import os

import numpy as np

from tests.resample_cases import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "timestretch.npz")
GOLDEN_VOCODER = os.path.join(ROOT, "tests", "golden", "timestretch_vocoder.npz")  # the planes of the SMALL cases
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libaudioflux_ref.so")
HANN, HAMM = 1, 2

# name -> radix2Exp, hop, samples, rate (window: Hann unless given)
CASES = {
    "128_32_r0.8": dict(exp=7, hop=32, n=1500, rate=0.8),            # generic forward and inverse kernels
    "256_64_r0.5": dict(exp=8, hop=64, n=3000, rate=0.5),            # alpha exactly 0 and 0.5
    "256_64_r0.8": dict(exp=8, hop=64, n=3000, rate=0.8),            # i * rate beside integers in float32
    "256_64_r1.5": dict(exp=8, hop=64, n=3000, rate=1.5),
    "256_64_r2.0": dict(exp=8, hop=64, n=3000, rate=2.0),            # frames skipped
    "256_64_odd": dict(exp=8, hop=64, n=3001, rate=1.7),             # odd length, T2 = 26
    "256_100_r0.8": dict(exp=8, hop=100, n=3000, rate=0.8),          # a hop that is no divisor of N
    "256_256_r1.3": dict(exp=8, hop=256, n=3000, rate=1.3),          # no overlap, 11 frames
    "256_64_hamm": dict(exp=8, hop=64, n=3000, rate=0.8, win=HAMM),  # a window that is not zero at its ends
    "512_128_r1.25": dict(exp=9, hop=128, n=5000, rate=1.25),
    "1024_256_r1.25": dict(exp=10, hop=256, n=12000, rate=1.25),
    "1024_256_r0.6": dict(exp=10, hop=256, n=12000, rate=0.6),
    "2048_512_r0.9": dict(exp=11, hop=512, n=20000, rate=0.9),
    "4096_1024_r0.7": dict(exp=12, hop=1024, n=20000, rate=0.7),     # 16 input frames; the accumulator reaches 5e4 rad
    "4096_1024_r1.5": dict(exp=12, hop=1024, n=20000, rate=1.5),
}
# pitch shift: name -> radix2Exp, hop, samples, semitones
PITCH = {f"ps_256_{n}_{s:+d}": dict(exp=8, hop=64, n=n, semi=s) for n in (3000, 3001) for s in (-12, -5, 3, 12)}
PITCH["ps_1024_12000_+7"] = dict(exp=10, hop=256, n=12000, semi=7)
VOCODER = ("128_32_r0.8", "256_64_r1.5", "256_100_r0.8")  # the vocoder alone on the reference's own STFT
SMALL = tuple(n for n, c in CASES.items() if c["exp"] <= 8)  # the emulated kernels (one host thread per lane): n_fft 128 and 256
SEQUENCE = (0.5, 1.7, 0.8, 0.5)  # rates on one live object, 256 / 64, n = 3000
# the drop-in flows (tests/dropin/flows_timestretch.py): the input of DROPIN_CASE as channel 0, reversed as channel 1
DROPIN_CASE = "256_64_r0.8"
DROPIN_STRETCH = {"stretch_0.8": 0.8, "stretch_0.5": 0.5, "stretch_1.5": 1.5}
DROPIN_SHIFT = {"shift_+3": 3, "shift_-5": -5}


def case_input(name):
    c = CASES.get(name) or PITCH[name]
    return signal(c["n"], seed=sorted(list(CASES) + list(PITCH)).index(name))


def semitone_rate(semi):
    """pitchShift_algorithm.c:63: powf(2, -nSemitone * 1.0 / 12)"""
    return np.float32(np.float32(2.0) ** np.float32(-semi * 1.0 / 12))


class Plan(C.Structure):
    """AfxTimeStretchPlan"""
    _fields_ = [("fftLength", C.c_int), ("slideLength", C.c_int), ("T1", C.c_int), ("T2", C.c_int), ("istftLength", C.c_int),
                ("returnLength", C.c_int), ("capacity", C.c_int), ("scratchBytes", C.c_longlong), ("clipsPerChunk", C.c_int)]


def bind(lib, device=True):
    """argument types of the reference's names and, with `device`, of this library's additive calls"""
    P, I, F, V, LL = C.POINTER, C.c_int, C.c_float, C.c_void_p, C.c_longlong
    lib.timeStretchObj_new.restype, lib.timeStretchObj_new.argtypes = I, [P(V), P(I), P(I), P(I)]
    lib.timeStretchObj_calDataCapacity.restype, lib.timeStretchObj_calDataCapacity.argtypes = I, [V, F, I]
    lib.timeStretchObj_timeStretch.restype, lib.timeStretchObj_timeStretch.argtypes = I, [V, F, V, I, V]
    lib.timeStretchObj_free.restype, lib.timeStretchObj_free.argtypes = None, [V]
    lib.pitchShiftObj_new.restype, lib.pitchShiftObj_new.argtypes = I, [P(V), P(I), P(I), P(I)]
    lib.pitchShiftObj_pitchShift.restype, lib.pitchShiftObj_pitchShift.argtypes = None, [V, I, I, V, I, V]
    lib.pitchShiftObj__free.restype, lib.pitchShiftObj__free.argtypes = None, [V]
    if device:
        lib.timeStretchObj_timeStretchBatchDevice.restype = I
        lib.timeStretchObj_timeStretchBatchDevice.argtypes = [V, F, V, I, I, LL, V, LL, V]
        lib.pitchShiftObj_pitchShiftBatchDevice.restype = I
        lib.pitchShiftObj_pitchShiftBatchDevice.argtypes = [V, I, V, I, I, LL, V, LL, V]
        lib.afx_phase_vocoder_device.restype = I
        lib.afx_phase_vocoder_device.argtypes = [V, V, I, I, I, LL, I, F, V, V, V]
        lib.timeStretchObj_setScratchLimit.restype, lib.timeStretchObj_setScratchLimit.argtypes = None, [V, LL]
        lib.pitchShiftObj_setScratchLimit.restype, lib.pitchShiftObj_setScratchLimit.argtypes = None, [V, LL]
        lib.afx_timestretch_plan.restype = I
        lib.afx_timestretch_plan.argtypes = [I, I, F, I, I, LL, P(Plan), V, V]
        lib.afx_error_count.restype, lib.afx_error_count.argtypes = I, []
    else:
        lib.phase_vocoder.restype, lib.phase_vocoder.argtypes = None, [V, V, I, I, I, F, V, V]
        lib.stftObj_new.restype, lib.stftObj_new.argtypes = I, [P(V), I, P(I), P(I), P(I)]
        lib.stftObj_calTimeLength.restype, lib.stftObj_calTimeLength.argtypes = I, [V, I]
        lib.stftObj_stft.restype, lib.stftObj_stft.argtypes = None, [V, V, I, V, V]
        lib.stftObj_istft.restype, lib.stftObj_istft.argtypes = None, [V, V, V, I, I, V]
        lib.stftObj_free.restype, lib.stftObj_free.argtypes = None, [V]
    return lib


_ref = None


def ref_lib():
    """the compiled reference, or None"""
    global _ref
    if _ref is None and os.path.exists(REF_LIB):
        _ref = bind(C.CDLL(REF_LIB), device=False)
    return _ref


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def new(lib, c, kind="timeStretch"):
    """(status, handle) of the object of case dict c"""
    obj = C.c_void_p(None)
    st = getattr(lib, kind + "Obj_new")(C.byref(obj), C.pointer(C.c_int(c["exp"])), C.pointer(C.c_int(c["hop"])),
                                        C.pointer(C.c_int(c.get("win", HANN))))
    return st, obj


def lengths(c, rate):
    """(T1, T2, inverse transform's samples) of a case at `rate`, in the reference's float32 arithmetic"""
    N = 1 << c["exp"]
    T1 = (c["n"] - N) // c["hop"] + 1
    T2 = int(np.ceil(np.float32(T1) / np.float32(rate)))
    return T1, T2, (T2 - 1) * c["hop"] + N


def stretch(lib, obj, x, rate, fill=0.0):
    """timeStretchObj_timeStretch of x into a capacity-sized buffer of `fill` (the reference accumulates: give it zeros):
    (returned length, capacity, the buffer)"""
    x = np.ascontiguousarray(x, np.float32)
    cap = lib.timeStretchObj_calDataCapacity(obj, C.c_float(rate), len(x))
    out = np.full(cap + 8, fill, np.float32)
    ret = lib.timeStretchObj_timeStretch(obj, C.c_float(rate), ptr(x), len(x), ptr(out))
    assert (out[cap:] == np.float32(fill)).all(), "values behind the capacity were written"
    return ret, cap, out[:cap].copy()


def run_case(lib, name, fill=0.0):
    c = CASES[name]
    st, obj = new(lib, c)
    assert st == 0 and obj, (name, st)
    try:
        return stretch(lib, obj, case_input(name), c["rate"], fill)
    finally:
        lib.timeStretchObj_free(obj)


def shift(lib, obj, x, semi, fill=0.0):
    """pitchShiftObj_pitchShift into len(x) + 8 samples of `fill`: the buffer"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.full(len(x) + 8, fill, np.float32)
    lib.pitchShiftObj_pitchShift(obj, 32000, semi, ptr(x), len(x), ptr(out))
    return out


def run_pitch(lib, name, fill=0.0):
    c = PITCH[name]
    st, obj = new(lib, c, "pitchShift")
    assert st == 0 and obj, (name, st)
    try:
        return shift(lib, obj, case_input(name), c["semi"], fill)
    finally:
        lib.pitchShiftObj__free(obj)


def roundf(n, rate):
    """roundf(n / rate) of timeStretch_algorithm.c:148: the float32 quotient, halves away from zero"""
    return int(np.floor(float(np.float32(n) / np.float32(rate)) + 0.5))


def pitch_length(n, semi):
    """samples a pitch shift writes: min(n, floorf(roundf(n / rate) * rate)) in float32"""
    rate = semitone_rate(semi)
    return min(n, int(np.floor(np.float32(roundf(n, rate)) * rate)))


def ref_stft(ref, c, x):
    """the reference's STFT of x without padding: re, im [T1, N]"""
    N = 1 << c["exp"]
    obj = C.c_void_p(None)
    assert ref.stftObj_new(C.byref(obj), c["exp"], C.pointer(C.c_int(c.get("win", HANN))), C.pointer(C.c_int(c["hop"])), None) == 0
    T1 = ref.stftObj_calTimeLength(obj, len(x))
    re, im = np.zeros((T1, N), np.float32), np.zeros((T1, N), np.float32)
    x = np.ascontiguousarray(x, np.float32)
    ref.stftObj_stft(obj, ptr(x), len(x), ptr(re), ptr(im))
    return obj, re, im


def ref_vocoder(ref, c, re, im, rate):
    """the reference's phase_vocoder on full spectra [T1, N]: re, im [T2, N]"""
    T1, N = re.shape
    T2 = int(np.ceil(np.float32(T1) / np.float32(rate)))
    re2, im2 = np.zeros((T2, N), np.float32), np.zeros((T2, N), np.float32)
    ref.phase_vocoder(ptr(re), ptr(im), T1, N, c["hop"], C.c_float(rate), ptr(re2), ptr(im2))
    return re2, im2


_gold = None


def golden():
    global _gold
    if _gold is None:
        _gold = np.load(GOLDEN)
    return _gold


def bar(name):
    """(peak-relative, L2-relative) bar of a case: twice the distance at which the reference sits from itself when only its
    FFT's rounding changes, never below 1e-5 (tests/golden/make_timestretch_golden.py)"""
    b = golden()[name + "/bar"]
    return float(b[0]), float(b[1])


def expected(name):
    """(returned length, capacity, the inverse transform's samples) of a time-stretch case"""
    ref = ref_lib()
    c = CASES[name]
    L2 = lengths(c, c["rate"])[2]
    if ref is not None:
        ret, cap, out = run_case(ref, name)
        return ret, cap, out[:L2]
    g = golden()
    meta = g[name + "/meta"]
    return int(meta[0]), int(meta[1]), g[name + "/out"]


def expected_pitch(name):
    """the samples the reference writes, cut to the input's length"""
    ref = ref_lib()
    c = PITCH[name]
    m = pitch_length(c["n"], c["semi"])
    if ref is not None:
        x = case_input(name)
        out = np.zeros(len(x) + 8, np.float32)
        st, obj = new(ref, c, "pitchShift")
        assert st == 0
        ref.pitchShiftObj_pitchShift(obj, 32000, c["semi"], ptr(x), len(x), ptr(out))
        ref.pitchShiftObj__free(obj)
        return out[:m].copy()
    return golden()[name + "/out"]


def expected_vocoder(name):
    """(re, im [T1, F] of the reference's STFT, re2, im2 [T2, F] of its phase_vocoder) of a SMALL case"""
    ref = ref_lib()
    c = CASES[name]
    F = (1 << c["exp"]) // 2 + 1
    if ref is not None:
        obj, re, im = ref_stft(ref, c, case_input(name))
        ref.stftObj_free(obj)
        re2, im2 = ref_vocoder(ref, c, re, im, c["rate"])
        return re[:, :F].copy(), im[:, :F].copy(), re2[:, :F].copy(), im2[:, :F].copy()
    global _gold_voc
    if _gold_voc is None:
        _gold_voc = np.load(GOLDEN_VOCODER)
    return tuple(_gold_voc[f"{name}/voc{k}"] for k in range(4))


_gold_voc = None


def expected_sequence():
    """the rates of SEQUENCE on fresh reference objects, 256 / 64, n = 3000: the inverse transforms' samples"""
    ref = ref_lib()
    c = dict(exp=8, hop=64, n=3000)
    if ref is None:
        return [golden()[f"sequence/{k}"] for k in range(len(SEQUENCE))]
    outs = []
    for r in SEQUENCE:
        st, obj = new(ref, c)
        outs.append(stretch(ref, obj, signal(3000, seed=5), r)[2][:lengths(c, r)[2]])
        ref.timeStretchObj_free(obj)
    return outs


def errors(got, want):
    d = got.astype(np.float64) - want
    return float(np.abs(d).max() / np.abs(want).max()), float(np.linalg.norm(d) / np.linalg.norm(want))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
