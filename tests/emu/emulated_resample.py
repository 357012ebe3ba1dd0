#!/usr/bin/env python3
"""afx_resample.hip as emulated device code through the C host object resampleObj: cases of tests/resample_cases.py against
the reference's outputs at the bar of the GPU tests (1e-5 peak- and L2-relative) through resample() and
resampleBatchDevice, and "extras": a strided batch of 5 clips bitwise equal to single calls with the padding untouched,
streaming in pieces, refusals.
AFX_LIB = the library tests/test_resample_emulated.py builds.  Arguments: case names (default: SMALL) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resample_cases as rc  # noqa: E402

lib = rc.bind(C.CDLL(os.environ["AFX_LIB"]))
TOL = 1e-5


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def errors(got, want):
    if not len(want):
        return 0.0, 0.0
    d = got.astype(np.float64) - want
    return float(np.abs(d).max() / np.abs(want).max()), float(np.linalg.norm(d) / np.linalg.norm(want))


def batch(obj, xs, n, out_pad=3, sentinel=7.5):
    """resampleBatchDevice over the rows of xs (n valid samples each): (length, the output rows with their padding)"""
    m = lib.resampleObj_calDataLength(obj, n)
    out = np.full((xs.shape[0] + 1, m + out_pad), sentinel, np.float32)
    stride = xs.strides[0] // 4 if xs.shape[0] > 1 else n  # (numpy leaves the stride of a single row unspecified)
    st = lib.resampleObj_resampleBatchDevice(obj, P(xs), xs.shape[0], n, stride, P(out), m + out_pad, None)
    return st, m, out


def case(name):
    x = rc.case_input(name)
    want, sel = rc.expected(name)
    st, obj = rc.new(lib, name)
    assert st == 0 and obj, (name, st)
    got = rc.call(lib, obj, x, fill=3.25)  # overwrite semantics: a non-zero destination
    st, m, out = batch(obj, x[None], len(x))
    lib.resampleObj_free(obj)
    assert st == m == len(got), (name, st, m, len(got))
    assert same_bits(out[0, :m], got) and (out[0, m:] == 7.5).all() and (out[1] == 7.5).all(), name
    if sel is not None:
        got = got[sel]
    assert len(got) == len(want), (name, len(got), len(want))
    p, l2 = errors(got, want)
    assert p <= TOL and l2 <= TOL, (name, p, l2)
    print(f"resample {name}: {len(x)} -> {m} samples, peak-rel {p:.2e}, l2-rel {l2:.2e}", flush=True)


def extras():
    # 5 clips, strides above the lengths, from a misaligned base: bitwise the single calls, the padding untouched
    name, n, clips, stride = "441_16_fast", 1500, 5, 1517
    buf = np.zeros(clips * stride + 1, np.float32)
    xs = buf[1:].reshape(clips, stride)
    for c in range(clips):
        xs[c, :n] = rc.signal(n, seed=40 + c)
    keep = xs.copy()
    st, obj = rc.new(lib, name)
    assert st == 0
    single = [rc.call(lib, obj, xs[c, :n]) for c in range(clips)]
    st, m, out = batch(obj, xs, n)
    assert st == m == len(single[0])
    for c in range(clips):
        assert same_bits(out[c, :m], single[c]), c
    assert (out[:clips, m:] == 7.5).all() and (out[clips] == 7.5).all() and np.array_equal(xs, keep)
    # refusals
    f = lib.resampleObj_resampleBatchDevice
    assert f(obj, P(xs), clips, n, stride, None, m, None) == -6
    assert f(obj, None, clips, n, stride, P(out), m, None) == -6
    assert f(obj, P(xs), clips, n, n - 1, P(out), m, None) == -6
    assert f(obj, P(xs), clips, n, stride, P(out), m - 1, None) == -6
    assert f(obj, P(xs), 0, n, stride, P(out), m, None) == -6
    assert f(obj, P(xs), clips, 0, stride, P(out), m, None) == -6
    assert f(obj, P(xs), clips, 2, stride, P(out), 4, None) == 0 and (out[:, m:] == 7.5).all()  # 2 samples: 0 outputs
    lib.resampleObj_enableContinue(obj, 1)
    assert f(obj, P(xs), clips, n, stride, P(out), m + 3, None) == -4
    lib.resampleObj_enableContinue(obj, 0)
    assert f(obj, P(xs), clips, n, stride, P(out), m + 3, None) == m
    assert lib.resampleObj_resample(obj, None, 5, P(out)) == -6 and lib.resampleObj_resample(None, P(xs), 5, P(out)) == -6
    lib.resampleObj_free(obj)
    # streaming in pieces == the reference fed the same pieces
    got, want = rc.run_pieces(lib), rc.expected_pieces()
    for g, w in zip(got, want):
        assert len(g) == len(w)
        p, l2 = errors(g, w)
        assert p <= TOL and l2 <= TOL, (p, l2)
    print(f"resample: a batch of {clips} strided clips bitwise the single calls, padding untouched; pieces {rc.PIECES} -> "
          f"{[len(g) for g in got]} as the reference; refusals", flush=True)


def main(argv):
    names = [a for a in argv if a != "extras"] or (list(rc.SMALL) if not argv else [])
    for name in names:
        case(name)
    if not argv or "extras" in argv:
        extras()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
