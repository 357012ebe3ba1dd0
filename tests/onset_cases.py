"""Inputs, parameter sets and ctypes bindings of the onset fixture (tests/golden/onset.npz).  Inputs are generated from seeds so
that only outputs are stored.  A case: name -> dict(T, M, sr, hop, order, kind, param, index): T frames of M bins, the
constructor's samplate / slideLength / filterOrder / NoveltyType, the NoveltyParam as a tuple (None: the C default), an
index table (None: every bin) and the input's seed (None: from the case's place in the list).  The spectrogram is decaying bursts in dB with 5 % multiplicative noise; phase kinds get a
phase plane in -pi ... pi.

FIXTURE: the five shapes whose reference run carries no marginal pick decision (tests/golden/make_onset_golden.py refuses
the others).  KINDS: each of the eleven novelty kinds once at (96, 24).  GRID: the (samplate, slideLength) pairs whose pick
parameters the fixture records from onsetObj_debug -- pairs where a product lands on an integer decide a parameter."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLUX, HFC, SD, SF, MKL, PD, WPD, NWPD, CD, RCD, BROADBAND = range(11)
KIND_NAMES = ("flux", "hfc", "sd", "sf", "mkl", "pd", "wpd", "nwpd", "cd", "rcd", "broadband")


def _case(T, M, sr, hop, order=1, kind=FLUX, param=None, index=None, seed=None):
    return dict(T=T, M=M, sr=sr, hop=hop, order=order, kind=kind, param=param, index=index, seed=seed)


# param: (step, p, isPostive, isExp, type, threshold, isNorm, gamma)
FIXTURE = {
    "flux_default": _case(240, 32, 32000, 512),
    "flux_o3_p2_abs_exp": _case(240, 32, 32000, 512, order=3, param=(1, 2.0, 0, 1, 0, 0.0, 0, 1.0)),
    "flux_step2_mean": _case(400, 128, 16000, 256, param=(2, 1.0, 1, 0, 1, 0.0, 0, 1.0)),
    "flux_o5_p3": _case(130, 40, 44100, 441, order=5, param=(1, 3.0, 1, 0, 0, 0.0, 0, 1.0), seed=403),  # wait = 3 suppresses a candidate
    "flux_o2_hop1024": _case(64, 8, 32000, 1024, order=2),  # preMax = wait = 0
}
KINDS = {"kind_" + KIND_NAMES[k]: _case(96, 24, 32000, 512, kind=k, param=(1, 1.0, 1, 0, 0, 3.0 if k == BROADBAND else 0.0, 0, 1.0))
         for k in range(11)}
CASES = dict(FIXTURE, **KINDS)
# what the emulated kernels run
SMALL = ("flux_o2_hop1024", "flux_o5_p3", "flux_o3_p2_abs_exp", "kind_hfc", "kind_wpd", "kind_rcd")

GRID = [(32000, 512), (32000, 1024), (16000, 256), (44100, 441), (48000, 480), (16000, 160), (22050, 2205), (8000, 240),
        (32000, 320), (32000, 960), (11025, 147), (22050, 512), (44100, 512), (48000, 1024), (96000, 256), (8000, 80),
        (16000, 48), (44100, 1323), (10000, 100), (10000, 300), (7, 3), (32000, 1), (0, 0), (-5, -1), (44100, 4410),
        (12000, 360), (24000, 72), (32000, 96), (50000, 1500), (1000, 10)]


def needs_phase(kind):
    return PD <= kind <= RCD


def power_to_db64(p, mn=-80.0):
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        return np.maximum(10 * np.log10(p / p.max()), mn)


def burst_power(T, M, seed):
    """power plane [T, M]: a floor, bursts that start at random frames over a random band and decay, 5 % multiplicative noise"""
    rng = np.random.default_rng(seed)
    p = np.full((T, M), 1e-6)
    t = np.arange(T)[:, None]
    for _ in range(max(3, T // 18)):
        t0, tau = rng.integers(1, max(2, T - 1)), rng.uniform(2.0, 9.0)
        lo = rng.integers(0, M)
        hi = min(M, lo + rng.integers(1, max(2, M // 2)))
        band = np.zeros(M)
        band[lo:hi] = rng.uniform(0.2, 1.0, hi - lo)
        p += np.where(t >= t0, np.exp(-np.maximum(t - t0, 0) / tau), 0.0) * band[None, :] * rng.uniform(0.1, 1.0)
    return p * (1 + 0.05 * rng.standard_normal((T, M))).clip(0.5, 1.5)


def burst_db(T, M, seed):
    return power_to_db64(burst_power(T, M, seed)).astype(np.float32)


def case_input(name):
    """-> spec [T, M] float32 (dB), phase [T, M] float32 or None"""
    c = CASES[name]
    seed = 300 + sorted(CASES).index(name) if c["seed"] is None else c["seed"]
    spec = burst_db(c["T"], c["M"], seed)
    phase = None
    if name.startswith("kind_"):
        spec = (spec + 81).astype(np.float32)  # magnitudes >= 1: ratios, logarithms and phase weights are defined
    if needs_phase(c["kind"]):
        phase = np.random.default_rng(seed + 1000).uniform(-np.pi, np.pi, spec.shape).astype(np.float32)
    return spec, phase


# ---- ctypes bindings shared by the library under test and the compiled reference (same entry points) ----------------------
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)


class NoveltyParam(C.Structure):
    _fields_ = [("step", C.c_int), ("p", C.c_float), ("isPostive", C.c_int), ("isExp", C.c_int), ("type", C.c_int),
                ("threshold", C.c_float), ("isNorm", C.c_int), ("gamma", C.c_float)]


def bind(lib):
    lib.onsetObj_new.restype = C.c_int
    lib.onsetObj_new.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, ip, ip, ip]
    lib.onsetObj_onset.restype = C.c_int
    lib.onsetObj_onset.argtypes = [C.c_void_p, fp, fp, C.POINTER(NoveltyParam), ip, C.c_int, fp, ip]
    lib.onsetObj_free.restype, lib.onsetObj_free.argtypes = None, [C.c_void_p]
    lib.onsetObj_debug.restype, lib.onsetObj_debug.argtypes = None, [C.c_void_p]
    lib.util_powerToDB.restype, lib.util_powerToDB.argtypes = None, [fp, C.c_int, C.c_float, fp]
    return lib


def bind_device(lib):
    """the additive calls of include/afx_batch.h"""
    bind(lib)
    ll, vp, i, f = C.c_longlong, C.c_void_p, C.c_int, C.c_float
    lib.onsetObj_onsetBatchDevice.restype = i
    lib.onsetObj_onsetBatchDevice.argtypes = [vp, vp, vp, i, C.POINTER(NoveltyParam), ip, i, vp, vp, vp, ll, ll, vp]
    lib.afx_onset_plan_host.restype, lib.afx_onset_plan_host.argtypes = i, [i, i, ip, fp]
    lib.afx_maxFilterDevice.restype, lib.afx_maxFilterDevice.argtypes = i, [vp, ll, i, i, vp, vp]
    lib.afx_peakPickDevice.restype = i
    lib.afx_peakPickDevice.argtypes = [vp, i, i, ll, i, i, i, i, i, f, vp, vp, ll, vp]
    lib.afx_powerToDbDevice.restype, lib.afx_powerToDbDevice.argtypes = i, [vp, i, ll, ll, f, vp, vp]
    return lib


def _opt(v):
    return None if v is None else C.byref(C.c_int(int(v)))


def new(lib, T, M, hop, sr=None, order=None, kind=None):
    obj = C.c_void_p()
    st = lib.onsetObj_new(C.byref(obj), T, M, hop, _opt(sr), _opt(order), _opt(kind))
    return st, obj


def param_of(p):
    return None if p is None else NoveltyParam(*p)


def index_of(index):
    if index is None:
        return None, None, 0
    idx = np.ascontiguousarray(index, np.int32)
    return idx, idx.ctypes.data_as(ip), len(idx)


def call(lib, obj, spec, phase=None, param=None, index=None, fill=0.0):
    """one onsetObj_onset call -> (count or status, evn [T], points [max(count, 0)]); evn starts as `fill`"""
    spec = np.ascontiguousarray(spec, np.float32)
    T = spec.shape[0]
    evn, pts = np.full(T, fill, np.float32), np.full(T, -1, np.int32)
    ph = None if phase is None else np.ascontiguousarray(phase, np.float32)
    par = param_of(param)
    idx, idx_p, idx_n = index_of(index)
    n = lib.onsetObj_onset(obj, spec.ctypes.data_as(fp), None if ph is None else ph.ctypes.data_as(fp),
                           None if par is None else C.byref(par), idx_p, idx_n, evn.ctypes.data_as(fp), pts.ctypes.data_as(ip))
    return n, evn, pts[:max(n, 0)].copy()


def run_case(lib, name, spec=None, phase=None):
    c = CASES[name]
    if spec is None:
        spec, phase = case_input(name)
    st, obj = new(lib, c["T"], c["M"], c["hop"], c["sr"], c["order"], c["kind"])
    assert st == 0 and obj, (name, st)
    n, evn, pts = call(lib, obj, spec, phase, c["param"], c["index"])
    lib.onsetObj_free(obj)
    assert n >= 0, (name, n)
    return evn, pts


def plan(lib, sr, hop):
    """afx_onset_plan_host -> [preMax, postMax, preAvg, postAvg, wait], delta"""
    out, delta = (C.c_int * 5)(), C.c_float()
    assert lib.afx_onset_plan_host(sr, hop, out, C.byref(delta)) == 0
    return list(out), delta.value


_DEBUG_CHILD = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
libc = C.CDLL(None)
lib.onsetObj_new.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.onsetObj_debug.argtypes = lib.onsetObj_free.argtypes = [C.c_void_p]
lib.onsetObj_debug.restype = lib.onsetObj_free.restype = None
for pair in sys.argv[2:]:
    sr, hop = (int(v) for v in pair.split(":"))
    obj = C.c_void_p()
    assert lib.onsetObj_new(C.byref(obj), 4, 4, hop, C.byref(C.c_int(sr)), None, None) == 0
    lib.onsetObj_debug(obj)
    lib.onsetObj_free(obj)
libc.fflush(None)
"""


def debug_params(lib_path, grid):
    """[preMax, postMax, preAvg, postAvg, wait] per (samplate, slideLength) of `grid`, and delta, parsed from what
    onsetObj_debug of the library at lib_path prints -- in a child process, whose stdout is the C library's"""
    import re
    r = subprocess.run([sys.executable, "-c", _DEBUG_CHILD, lib_path] + [f"{sr}:{hop}" for sr, hop in grid], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = re.findall(r"preMax=(-?\d+),postMax=(-?\d+), preAvg=(-?\d+),postAvg=(-?\d+), wait=(-?\d+),delta=([-0-9.]+)", r.stdout)
    assert len(rows) == len(grid), r.stdout[-2000:]
    return np.array([[int(v) for v in row[:5]] for row in rows], np.int32), np.array([float(row[5]) for row in rows], np.float32)
