"""The ST case table, its inputs, the float64 reference and the comparison shared by tests/test_st_cpu.py, the emulated run
(tests/emu/emulated_st.py), tests/test_st_gpu.py and the generator of tests/golden/st.npz.

Reference: `f64_st` below, the operation restated in float64 with numpy's FFT.  With X = fft(x) and a row's bin k:
  k != 0: c_k = -factor 2 pi^2 / k^(2 norm) (rounded to float32, as the reference stores it),
          W_k[j] = exp(c_k j^2) + exp(c_k (j - N)^2), row = ifft_j(X[(k + j) mod N] W_k[j]);
  k == 0: the mean of x in every column.
tests/test_st_cpu.py holds it against the compiled reference.
Comparison, per chunk: e = max|got - want| over the requested rows / P, P = max|float64| over those rows.  Bar: max(1e-5, 2 x the
compiled reference's own e against float64, recorded per case and input in the fixture), against float64 (every row) and
against the stored compiled-reference rows (the fixture's selection).  Nothing here is taken from what a kernel returns."""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np

from tests.conftest import ROOT, parity_log

GOLDEN = os.path.join(ROOT, "tests", "golden", "st.npz")
FLOOR, FACTOR = 1e-5, 2.0
KIND = "st: per chunk max|got - want| over the rows / max|float64| over the rows, bar max(1e-5, 2 x reference-vs-float64)"

# lo, hi: the range given to stObj_new; bins: a list given to stObj_useBinArr afterwards, or None; chunks: the inputs used;
# store: positions (in the case's rows) of the reference rows the fixture keeps, or None for all; step: every step-th column
Case = namedtuple("Case", "name r lo hi factor norm bins chunks store step")
CASES = [
    Case("r4full", 4, 0, 8, 1.0, 1.0, None, (0, 1, 2), None, 1),     # N below the lane count; DC row; N/2 row
    Case("r6full", 6, 0, 32, 1.0, 1.0, None, (0, 1, 2), None, 1),
    Case("r9default", 9, 1, 255, 1.0, 1.0, None, (0, 1, 2), (0, 1, 36, 127, 254), 1),  # the wrapper's default range
    Case("r9fn", 9, 1, 256, 2.5, 0.8, None, (0, 1, 2), (0, 63, 255), 1),               # the powf path
    Case("r9list", 9, 1, 255, 1.0, 1.0, (0, 256, 7, 7, 100), (0, 1, 2), None, 1),      # unordered, repeated, both ends
    Case("r12doc", 12, 1, 1024, 1.0, 1.0, None, (1,), (0, 511, 1023), 1),              # the docstring call, 33 MB: the tone
    Case("r14edge", 14, 1, 4, 1.0, 1.0, (1, 2, 3, 4) + tuple(range(8185, 8193)), (0, 1, 2), (0, 3, 4, 11), 8),
]                                                                    # largest LDS; narrowest and widest windows
INPUTS = ("noise", "tone", "impulse")


def by_name(name):
    return next(c for c in CASES if c.name == name)


def rows_of(c):
    """the bin of every output row"""
    return list(c.bins) if c.bins is not None else list(range(c.lo, c.hi + 1))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """[3][N] float32: 0.1 N(0,1) | 0.1 sin(2 pi 0.1037 n) + 0.1 N(0,1) | one sample of 1 at N / 3"""
    c = by_name(name)
    N = 1 << c.r
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = np.zeros((3, N), np.float32)
    x[0] = 0.1 * rng.standard_normal(N)
    x[1] = 0.1 * np.sin(2 * np.pi * 0.1037 * np.arange(N)) + 0.1 * rng.standard_normal(N)
    x[2, N // 3] = 1.0
    x.setflags(write=False)
    return x


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
def coef32(r, factor=1.0, norm=1.0):
    """c_k, k = 0 ... N/2, float32 (entry 0 is 0): the formula in float64, rounded once"""
    k = np.arange(1, (1 << (r - 1)) + 1, dtype=np.float64)
    c = -float(np.float32(factor)) * 2.0 * np.pi * np.pi / k ** (2.0 * float(np.float32(norm)))
    return np.concatenate([[0.0], c]).astype(np.float32)


def f64_st(x, r, bins, factor=1.0, norm=1.0):
    """complex128 [len(bins)][N]"""
    N = 1 << r
    x = np.asarray(x, np.float64)
    X = np.fft.fft(x)
    XX = np.concatenate([X, X])
    c = coef32(r, factor, norm).astype(np.float64)
    j = np.arange(N, dtype=np.float64)
    j2, jn2 = j * j, (j - N) * (j - N)
    out = np.empty((len(bins), N), complex)
    for i, k in enumerate(bins):
        if k == 0:
            out[i] = x.mean()
        else:
            out[i] = np.fft.ifft(XX[k:k + N] * (np.exp(c[k] * j2) + np.exp(c[k] * jn2)))
    return out


Ref = namedtuple("Ref", "f64 peak stored r_ref")


@functools.lru_cache(maxsize=None)
def reference(name):
    """per input k of the case's chunks: float64 rows [rows][N], P, the stored compiled-reference rows [len(store)][N / step],
    the recorded reference-vs-float64 e"""
    c = by_name(name)
    gold = np.load(GOLDEN)
    bins = rows_of(c)
    f64, peak, stored, r_ref = {}, {}, {}, {}
    rr = np.asarray(gold[f"{name}/ref_vs_f64"], np.float64)
    assert rr.shape == (len(c.chunks),)
    for q, k in enumerate(c.chunks):
        f64[k] = f64_st(inputs(name)[k], c.r, bins, c.factor, c.norm)
        f64[k].setflags(write=False)
        peak[k] = float(np.abs(f64[k]).max())
        stored[k] = gold[f"{name}/{INPUTS[k]}/rows"]
        r_ref[k] = float(rr[q])
    return Ref(f64, peak, stored, r_ref)


def select(c, rows):
    """the part of [rows][N] the fixture keeps"""
    sel = list(range(len(rows_of(c)))) if c.store is None else list(c.store)
    return np.ascontiguousarray(np.asarray(rows)[sel][:, ::c.step])


def judge(name, chunk_inputs, got, tag="", pos=None):
    """got [chunks][rows][N] complex64; chunk q is input chunk_inputs[q].  pos: `got` holds only these of the case's rows (a
    subset of the fixture's selection); P is then the peak of those rows, never more than the case's.  -> worst error / bar"""
    c, ref = by_name(name), reference(name)
    worst, fails = 0.0, []
    for q, k in enumerate(chunk_inputs):
        what = f"st {name} {INPUTS[k]}{tag}"
        g = np.asarray(got[q])
        if pos is None:
            want, peak, gs, stored = ref.f64[k], ref.peak[k], select(c, g), ref.stored[k]
        else:
            want = ref.f64[k][list(pos)]
            peak, gs, stored = float(np.abs(want).max()), g[:, ::c.step], ref.stored[k][[c.store.index(p) for p in pos]]
        assert g.shape == want.shape, (what, g.shape)
        assert np.all(np.isfinite(g.real)) and np.all(np.isfinite(g.imag)), f"{what}: non-finite results"
        bar = max(FLOOR, FACTOR * ref.r_ref[k])
        for target, e in (("float64", np.abs(g - want).max() / peak),
                          ("compiled reference", np.abs(gs.astype(np.complex128) - stored).max() / peak)):
            e = float(e)
            print(f"{what} vs {target}: {e:.2e} (bar {bar:.2e}, reference vs float64 {ref.r_ref[k]:.2e})", flush=True)
            parity_log(f"{what} vs {target}", e, bar, KIND, {"case": name, "reference_vs_float64": ref.r_ref[k]})
            if not e <= bar:
                fails.append(f"{what} vs {target}: {e:.3e} > {bar:.3e}")
            worst = max(worst, e / bar)
    assert not fails, "; ".join(fails)
    return worst
