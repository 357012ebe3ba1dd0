"""The FST case table, its inputs, the float64 reference and the comparison shared by tests/test_fst_cpu.py, the emulated run
(tests/emu/emulated_fst.py), tests/test_fst_gpu.py and the generator of tests/golden/fst.npz.

Reference: `f64_fst` below, the operation restated in float64 with numpy's FFT (the whole N x N matrix: small r only), and
`cells64` / `expand`, the same numbers without the matrix: the N/2 + 1 visible cells (bin -1, DC, bin +1, band 2, band 4,
..., band N/4) and the rows requested.  tests/test_fst_cpu.py holds the two against each other and against the compiled
reference.
Comparison, per chunk: e = max|got - want| over the requested rows / P, P = max|float64| over the chunk's whole 0 ... N/2
matrix (= over its cells): the scale the forward FFT's error follows.  Bar: max(1e-5, 2 x the compiled reference's own e
against float64, recorded in the fixture), against float64 and against the stored compiled-reference cells.  Nothing here is
taken from what a kernel returns."""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np

from tests.conftest import ROOT, parity_log

GOLDEN = os.path.join(ROOT, "tests", "golden", "fst.npz")
FLOOR, FACTOR = 1e-5, 2.0
KIND = "fst: per chunk max|got - want| over the rows / max|float64| over the chunk, bar max(1e-5, 2 x reference-vs-float64)"
BAND_FLOOR = 1e-3  # every band's float64 peak is at least this fraction of P for the noise and impulse inputs

Case = namedtuple("Case", "name r ranges chunks matrix")
CASES = [
    Case("r4full", 4, ((0, 8),), (0, 1, 2), True),             # smallest plan; every single and both bands
    Case("r6full", 6, ((0, 32),), (0, 1, 2), True),
    Case("r9default", 9, ((1, 255),), (0, 1, 2), False),       # the wrapper's default range
    Case("r12doc", 12, ((1, 2047),), (1,), False),             # the docstring size, 67 MB: one chunk, the tone
    Case("r14edge", 14, ((4090, 4104), (8185, 8192)), (0, 1, 2), False),  # f = 4096 / 4097; ends at N/2; the 2^12-point band
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
    x[1] = 0.1 * np.sin(2 * np.pi * 0.1037 * np.arange(N)) + 0.1 * rng.standard_normal(N)
    x[2, N // 3] = 1.0
    x.setflags(write=False)
    return x


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
def lens(r):
    return [1] + [2 ** e for e in range(r - 2, 0, -1)] + [1, 1] + [2 ** e for e in range(0, r - 1)]


def f64_fst(x, r, lo, hi):
    """the whole operation, literally: N x N complex128 on the way (r <= 10 or so)"""
    N = 1 << r
    X = np.fft.fftshift(np.fft.fft(np.fft.ifftshift(x.astype(np.float64)))) / np.sqrt(N)
    l = lens(r)
    off = np.concatenate([[0], np.cumsum(l)])
    V = X.copy()
    for i, n in enumerate(l):
        if n >= 2:
            s = X[off[i]:off[i] + n]
            V[off[i]:off[i] + n] = np.fft.fftshift(np.fft.ifft(np.fft.ifftshift(s))) * np.sqrt(n)
    full = np.zeros((N, N), complex)
    for i, n in enumerate(l):
        full[N - off[i + 1]: N - off[i + 1] + n, :] = np.repeat(V[off[i]:off[i] + n], N // n)[None, :]
    return full[[N // 2 - f for f in range(lo, hi + 1)]]


def cells64(x, r):
    """the visible cells of one chunk, complex128 [N/2 + 1]: the partitions r-1 ... 2r-1 of f64_fst, nothing else"""
    N = 1 << r
    X = np.fft.fftshift(np.fft.fft(np.fft.ifftshift(np.asarray(x, np.float64)))) / np.sqrt(N)
    l = lens(r)
    off = np.concatenate([[0], np.cumsum(l)])
    out = []
    for i in range(r - 1, 2 * r):
        n, s = l[i], X[off[i]:off[i] + l[i]]
        out.append(s if n < 2 else np.fft.fftshift(np.fft.ifft(np.fft.ifftshift(s))) * np.sqrt(n))
    return np.concatenate(out)


def row_map(r):
    """(first cell, band length) of every index f = 0 ... N/2: 0, 1, 2 are the singles, n + 1 ... 2n the band of n points"""
    half = 1 << (r - 1)
    cell, ln = np.zeros(half + 1, np.int64), np.ones(half + 1, np.int64)
    cell[:3] = (0, 1, 2)
    n = 2
    while n <= half // 2:
        cell[n + 1:2 * n + 1], ln[n + 1:2 * n + 1] = n + 1, n
        n *= 2
    return cell, ln


def expand(cells, r, lo, hi):
    """rows lo ... hi of the matrix from a chunk's cells: column l of index f holds cell first(f) + l // (N / len(f))"""
    N = 1 << r
    cell, ln = row_map(r)
    out = np.empty((hi - lo + 1, N), cells.dtype)
    for k, f in enumerate(range(lo, hi + 1)):
        out[k] = np.repeat(cells[cell[f]:cell[f] + ln[f]], N // ln[f])
    return out


def decimate(rows, r, lo, hi):
    """the distinct columns of rows lo ... hi, one array per row, and whether every row is exactly their expansion"""
    N = 1 << r
    _, ln = row_map(r)
    out, exact = [], True
    for k, f in enumerate(range(lo, hi + 1)):
        d = rows[k, ::N // ln[f]]
        exact = exact and bool(np.array_equal(np.repeat(d, N // ln[f]).view(np.uint32), np.ascontiguousarray(rows[k]).view(np.uint32)))
        out.append(d)
    return out, exact


def band_peaks(cells, r):
    """max|cell| of the three singles and of every band"""
    peaks = [abs(cells[0]), abs(cells[1]), abs(cells[2])]
    n = 2
    while n <= (1 << r) // 4:
        peaks.append(np.abs(cells[n + 1:2 * n + 1]).max())
        n *= 2
    return np.array(peaks)


Ref = namedtuple("Ref", "cells64 peak cells_c mat_c r_ref")


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 cells [3][N/2 + 1] of the three inputs, P [3], the stored compiled-reference cells, the stored matrices (cases
    with `matrix`), and the recorded reference-vs-float64 e [3]"""
    c = by_name(name)
    gold = np.load(GOLDEN)
    c64 = np.stack([cells64(x, c.r) for x in inputs(name)])
    peak = np.abs(c64).max(axis=1)
    cells_c = np.stack([gold[f"{name}/{k}/cells"] for k in INPUTS]).astype(np.complex128)
    assert cells_c.shape == c64.shape, (name, cells_c.shape, c64.shape)
    mat_c = np.stack([gold[f"{name}/{k}/matrix"] for k in INPUTS]) if c.matrix else None
    r_ref = np.asarray(gold[f"{name}/ref_vs_f64"], np.float64)
    for a in (c64, peak, cells_c, mat_c, r_ref):
        if a is not None:
            a.setflags(write=False)
    return Ref(c64, peak, cells_c, mat_c, r_ref)


def judge_cells(name, chunk_inputs, cells, tag=""):
    """cells [chunks][N/2 + 1] complex; chunk q is input chunk_inputs[q].  -> worst error / bar"""
    ref = reference(name)
    worst, fails = 0.0, []
    for q, k in enumerate(chunk_inputs):
        got = np.asarray(cells[q])
        assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), f"fst {name} {INPUTS[k]}{tag}: non-finite cells"
        bar = max(FLOOR, FACTOR * ref.r_ref[k])
        for target, want in (("float64", ref.cells64[k]), ("compiled reference", ref.cells_c[k])):
            e = float(np.abs(got - want).max() / ref.peak[k])
            worst, fails = _record(f"fst {name} {INPUTS[k]}{tag} cells vs {target}", e, bar, ref.r_ref[k], name, worst, fails)
    assert not fails, "; ".join(fails)
    return worst


def judge_rows(name, chunk_inputs, rows, lo, hi, tag=""):
    """rows [chunks][hi - lo + 1][N] complex64 of indices lo ... hi.  Every row must be bitwise the expansion of its distinct
    columns; those are judged.  -> worst error / bar"""
    c, ref = by_name(name), reference(name)
    cell, ln = row_map(c.r)
    worst, fails = 0.0, []
    for q, k in enumerate(chunk_inputs):
        what = f"fst {name} {INPUTS[k]}{tag} rows {lo}...{hi}"
        got = np.asarray(rows[q])
        assert got.shape == (hi - lo + 1, 1 << c.r), (what, got.shape)
        assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), f"{what}: non-finite results"
        dist, exact = decimate(got, c.r, lo, hi)
        assert exact, f"{what}: a row is not the sample-and-hold of its band's cells"
        bar = max(FLOOR, FACTOR * ref.r_ref[k])
        for target, want in (("float64", ref.cells64[k]), ("compiled reference", ref.cells_c[k])):
            e = max(float(np.abs(d - want[cell[f]:cell[f] + ln[f]]).max()) for d, f in zip(dist, range(lo, hi + 1))) / ref.peak[k]
            worst, fails = _record(f"{what} vs {target}", e, bar, ref.r_ref[k], name, worst, fails)
    assert not fails, "; ".join(fails)
    return worst


def _record(what, e, bar, r_ref, name, worst, fails):
    print(f"{what}: {e:.2e} (bar {bar:.2e}, reference vs float64 {r_ref:.2e})", flush=True)
    parity_log(what, e, bar, KIND, {"case": name, "reference_vs_float64": float(r_ref)})
    if not e <= bar:
        fails.append(f"{what}: {e:.3e} > {bar:.3e}")
    return max(worst, e / bar), fails
