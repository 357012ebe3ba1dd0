"""The NSGT case table, its inputs, the float64 reference and the comparison shared by tests/test_nsgt_cpu.py, the emulated
run (tests/emu/emulated_nsgt.py), tests/test_nsgt_gpu.py and the generator of tests/golden/nsgt.npz.

Reference: the operation in float64 from the PLAN the library hands out without a device (afx_nsgt_plan_host) --
    X = fft(x);  z[(L - L//2 + j) mod L] = X[clip(o + j, 0, N - 1)] w[j];  cell_i = ifft(z);  row_i = cell_i[colmap_i]
Comparison: for every band i of every chunk, over all its samples, e_i = max|got_i - want_i| / max|want_i|, for the cells and
for the matrix rows.  Bar: max(1e-5, 2 r_i), r_i = the compiled reference's own e_i against the same float64 result (form and
factor of tests/cwt_check.py), against float64 and against the compiled reference's stored results.  No band is left out; a
band whose float64 peak is zero is an error of the table.  Nothing here is taken from what a kernel returns."""
import ctypes as C
import functools
import math
import os
import zlib
from collections import namedtuple

import numpy as np

from tests.conftest import ROOT, parity_log

GOLDEN = os.path.join(ROOT, "tests", "golden", "nsgt.npz")
FLOOR, FACTOR = 1e-5, 2.0
KIND = "nsgt: per band max|got - want| / max|want| over all its samples, bar max(1e-5, 2 x reference-vs-float64)"
MATRIX_LIMIT = 20000  # the fixture stores the compiled reference's matrix where num * maxLength is at most this

EFFICIENT, STANDARD = 0, 1
SCALE = {"Linear": 0, "Linspace": 1, "Mel": 2, "Bark": 3, "Erb": 4, "Octave": 5, "Log": 6}
STYLE = {"Slaney": 0, "ETSI": 1, "Gammatone": 2, "Point": 3, "Rect": 4, "Hann": 5, "Hamm": 6, "Blackman": 7, "Bohman": 8,
         "Kaiser": 9, "Gauss": 10}
NORMAL = {"None": 0, "Area": 1, "BandWidth": 2}

Case = namedtuple("Case", "name num r sr low high bpo min_len bank scale style normal")
C1 = 32.703
CASES = [
    Case("oct84", 84, 15, 32000, C1, None, 12, 3, EFFICIENT, "Octave", "Slaney", "BandWidth"),     # 5 ... 481, 59 distinct lengths
    Case("mel12", 12, 9, 16000, 0.0, None, 12, 3, EFFICIENT, "Mel", "Slaney", "BandWidth"),         # 13 ... 99
    Case("bark12std", 12, 9, 16000, 0.0, None, 12, 3, STANDARD, "Bark", "Blackman", "None"),        # 11 ... 119, even lengths
    Case("oct24min", 24, 12, 32000, C1, None, 12, 3, EFFICIENT, "Octave", "Slaney", "BandWidth"),   # all 3: the clamp
    Case("oct36rect", 36, 13, 32000, C1, None, 6, 1, EFFICIENT, "Octave", "Rect", "None"),          # 3 ... 111
    Case("log20std", 20, 11, 16000, 40.0, None, 12, 3, STANDARD, "Log", "Kaiser", "BandWidth"),     # 4 ... 579
    Case("lin10", 10, 10, 16000, 0.0, None, 12, 3, EFFICIENT, "Linear", "Hamm", "None"),            # all 3, offset 0
    Case("mel40", 40, 13, 32000, 0.0, None, 12, 3, EFFICIENT, "Mel", "Bohman", "BandWidth"),        # 33 ... 637, ends at N/2
    Case("bark2", 2, 10, 16000, 0.0, None, 12, 3, EFFICIENT, "Bark", "Rect", "BandWidth"),          # 203, 725: above N/2
    Case("linspace6", 6, 8, 16000, 100.0, None, 12, 3, EFFICIENT, "Linspace", "Gauss", "BandWidth"),  # 51 ... 53
]
INPUTS = ("noise", "tone", "impulse")


def by_name(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """[3][N] float32: 0.1 N(0,1) | 0.1 sin(2 pi 0.1037 n) + 0.1 N(0,1) | one sample of 1 at N / 3"""
    c = by_name(name)
    N = 1 << c.r
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = np.zeros((3, N), np.float32)
    x[0] = 0.1 * rng.standard_normal(N)
    x[1] = 0.1 * np.sin(2 * np.pi * 0.1037 * c.sr * (np.arange(N) / c.sr)) + 0.1 * rng.standard_normal(N)
    x[2, N // 3] = 1.0
    x.setflags(write=False)
    return x


# ---- ctypes plumbing shared by the library, the emulated library and the compiled reference ---------------------------------
ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)


def _pi(v):
    return None if v is None else C.pointer(C.c_int(int(v)))


def _pf(v):
    return None if v is None else C.pointer(C.c_float(float(v)))


def new_args(c, min_len=None):
    """the optional-pointer arguments of nsgtObj_new / afx_nsgt_plan_host after (obj,) num, radix2Exp"""
    return (_pi(c.sr), _pf(c.low), _pf(c.high), _pi(c.bpo), _pi(c.min_len if min_len is None else min_len), _pi(c.bank),
            _pi(SCALE[c.scale]), _pi(STYLE[c.style]), _pi(NORMAL[c.normal]))


NEW_ARGTYPES = [C.c_int, C.c_int, ip, fp, fp, ip, ip, ip, ip, ip, ip]
Plan = namedtuple("Plan", "len offset bin fre window max total colmap")


def plan_host(lib, c, min_len=None):
    """(status, Plan) from afx_nsgt_plan_host: works without a device"""
    fn = lib.afx_nsgt_plan_host
    fn.restype = C.c_int
    fn.argtypes = NEW_ARGTYPES + [ip, ip, ip, fp, fp, ip, ip, ip]
    mx, tot = C.c_int(0), C.c_int(0)
    a = new_args(c, min_len)
    st = fn(c.num, c.r, *a, None, None, None, None, None, C.byref(mx), C.byref(tot), None)
    if st != 0:
        return st, None
    ln, off, bn = (np.zeros(c.num, np.int32) for _ in range(3))
    fre, win = np.zeros(c.num, np.float32), np.zeros(tot.value, np.float32)
    cm = np.zeros((c.num, mx.value), np.int32)
    st = fn(c.num, c.r, *a, ln.ctypes.data_as(ip), off.ctypes.data_as(ip), bn.ctypes.data_as(ip), fre.ctypes.data_as(fp),
            win.ctypes.data_as(fp), C.byref(mx), C.byref(tot), cm.ctypes.data_as(ip))
    assert st == 0
    return 0, Plan(ln, off, bn, fre, win, mx.value, tot.value, cm)


@functools.lru_cache(maxsize=None)
def product_plan(name, min_len=None):
    import audioflux_amd as af
    st, p = plan_host(af.get_lib(), by_name(name), min_len)
    assert st == 0, (name, st)
    return p


# ---- float32 restatements of the reference's setup (tests/test_nsgt_cpu.py pins them against the compiled reference) --------
f32 = np.float32


def _roundf(v):
    return f32(math.floor(float(v) + 0.5) if v >= 0 else -math.floor(-float(v) + 0.5))


def resolve(c):
    """(low, high) as nsgtObj_new hands them to nsgt_filterBank (nsgt_algorithm.c:151-209) for the rows used here: an explicit
    low >= 0, no high, and never the octave / log default of low == 0"""
    low, high = f32(c.low), f32(c.sr / 2.0)
    assert not (low == 0 and c.scale in ("Octave", "Log"))
    if c.scale == "Linear":
        det = f32(c.sr) / f32(1 << c.r)
        lo = _roundf(low / det)
        low, high = lo * det, f32(lo + f32(c.num) - f32(1)) * det
    elif c.scale == "Octave":
        bpo = f32(c.bpo if 4 <= c.bpo <= 48 else 12)
        lo = _roundf(f32(float(bpo) * math.log2(float(low / f32(440)))))
        hi = f32(lo + f32(c.num) - f32(1))
        low, high = f32(math.pow(2, float(lo / bpo)) * 440), f32(math.pow(2, float(hi / bpo)) * 440)
    return low, high


def linspace32(start, stop, length):
    """__vlinspace (flux_vector.c:2145-2162) in float32"""
    start, stop = f32(start), f32(stop)
    step = f32(f32(stop - start) / f32(length - 1 if length - 1 > 0 else 1))
    return (start + np.arange(length, dtype=np.float32) * step).astype(np.float32)


def colmap_restated(lens, max_len, r, sr):
    """__nsgtObj_dealTime (nsgt_algorithm.c:253-290) and the search of nsgtObj_nsgt (:585-604): column j of row i holds cell
    k - 1, k the first index >= the row's running start with maxTime[j] < time_i[k]"""
    time = f32(1 << r) / f32(sr)
    max_time = linspace32(0, time, max_len + 1)
    out = np.zeros((len(lens), max_len), np.int32)
    for i, L in enumerate(lens):
        cur = f32(L)
        det = f32(cur - f32(2)) if cur - f32(2) >= 0 else f32(0)
        off = f32(time / f32(cur + det))
        t = linspace32(-off, f32(time + off), int(L) + 1)
        start = 0
        for j in range(max_len):
            k = start
            while not (max_time[j] < t[k]):
                k += 1  # (an IndexError here: the reference would leave the column unwritten)
            out[i, j] = k - 1
            start = k
    return out


# ---- the float64 reference -------------------------------------------------------------------------------------------------
def transform64(plan, x):
    """-> (cells complex128 [total], matrix complex128 [num][max]) of one chunk"""
    N = len(x)
    X = np.fft.fft(np.asarray(x, np.float64))
    cells = np.zeros(plan.total, np.complex128)
    mat = np.zeros((len(plan.len), plan.max), np.complex128)
    at = 0
    for i, (L, o) in enumerate(zip(plan.len, plan.offset)):
        L, o = int(L), int(o)
        j = np.arange(L)
        z = np.zeros(L, np.complex128)
        z[(L - L // 2 + j) % L] = X[np.clip(o + j, 0, N - 1)] * plan.window[at:at + L].astype(np.float64)
        cells[at:at + L] = np.fft.ifft(z)
        mat[i] = cells[at:at + L][plan.colmap[i]]
        at += L
    return cells, mat


def per_band_cells(got, want, lens):
    """e_i over the cells of each band; every band is judged"""
    e, at = np.zeros(len(lens)), 0
    for i, L in enumerate(lens):
        L = int(L)
        peak = np.abs(want[at:at + L]).max()
        assert peak > 0, f"band {i} of the float64 reference is zero throughout"
        e[i] = np.abs(got[at:at + L] - want[at:at + L]).max() / peak
        at += L
    return e


def per_band_rows(got, want):
    peak = np.abs(want).max(axis=-1)
    assert np.all(peak > 0), "a row of the float64 reference is zero throughout"
    return np.abs(np.asarray(got) - want).max(axis=-1) / peak


Ref = namedtuple("Ref", "plan cells64 mat64 cells_c mat_c r_cells r_rows")


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 and stored compiled-reference results of the three inputs, and r_i of both outputs ([3][num])"""
    c = by_name(name)
    plan = product_plan(name)
    gold = np.load(GOLDEN)
    x = inputs(name)
    both = [transform64(plan, xc) for xc in x]
    cells64, mat64 = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    cells_c = np.stack([gold[f"{name}/{k}/cells"] for k in INPUTS]).astype(np.complex128)
    assert cells_c.shape == cells64.shape, (name, cells_c.shape, cells64.shape)
    mat_c = None
    if c.num * plan.max <= MATRIX_LIMIT:
        mat_c = np.stack([gold[f"{name}/{k}/matrix"] for k in INPUTS]).astype(np.complex128)
    r_cells = np.stack([per_band_cells(g, w, plan.len) for g, w in zip(cells_c, cells64)])
    # where the matrix is not stored: the matrix only repeats cells, so a row's r is its band's
    r_rows = np.stack([per_band_rows(g, w) for g, w in zip(mat_c, mat64)]) if mat_c is not None else r_cells
    for a in (cells64, mat64, cells_c, mat_c, r_cells, r_rows):
        if a is not None:
            a.setflags(write=False)
    return Ref(plan, cells64, mat64, cells_c, mat_c, r_cells, r_rows)


def judge(name, chunk_inputs, cells, mat, tag=""):
    """cells [chunks][total] complex or None, mat [chunks][num][max] complex; chunk q is input chunk_inputs[q] (an index into
    INPUTS).  Every band of every chunk, cells and rows, against float64 and the stored compiled reference; returns the worst
    error / bar"""
    ref = reference(name)
    worst, fails = 0.0, []
    for q, k in enumerate(chunk_inputs):
        what = f"nsgt {name} {INPUTS[k]}{tag}"
        outs = [("matrix", mat[q], ref.mat64[k], None if ref.mat_c is None else ref.mat_c[k], ref.r_rows[k])]
        if cells is not None:
            outs.append(("cells", cells[q], ref.cells64[k], ref.cells_c[k], ref.r_cells[k]))
        for kind, got, w64, wc, r in outs:
            assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), f"{what} {kind}: non-finite results"
            bar = np.maximum(FLOOR, FACTOR * r)
            for target, want in (("float64", w64), ("compiled reference", wc)):
                if want is None:
                    continue
                e = per_band_cells(got, want, ref.plan.len) if kind == "cells" else per_band_rows(got, want)
                i = int(np.argmax(e / bar))
                print(f"{what} {kind} vs {target}: worst {e[i]:.2e} (band {i}, length {ref.plan.len[i]}; bar {bar[i]:.2e}, "
                      f"reference vs float64 {r[i]:.2e})", flush=True)
                parity_log(f"{what} {kind} vs {target}", e[i], bar[i], KIND,
                           {"case": name, "band": i, "length": int(ref.plan.len[i]), "reference_vs_float64": float(r[i])})
                worst = max(worst, float((e / bar).max()))
                for b in np.nonzero(e > bar)[0]:
                    fails.append(f"{INPUTS[k]} {kind} band {b} (length {ref.plan.len[b]}) vs {target}: {e[b]:.3e} > {bar[b]:.3e}")
    assert not fails, f"nsgt {name}{tag}: {len(fails)} band(s) over their bar: " + "; ".join(fails[:8])
    return worst
