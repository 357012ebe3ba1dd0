"""CPU-only: what the time-stretch and pitch-shift objects decide without a device (afx_timestretch_plan,
include/mir/timeStretch_algorithm.h) against the compiled reference (oracle/_ref when present, else
tests/golden/timestretch.npz): frame counts, returned length and capacity over rates 0.5 ... 2 in steps of 0.05 and a dozen
lengths, the k / alpha table against a numpy float32 statement, chunking under a scratch limit, refusals, the exported names."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from tests import timestretch_cases as tc


@pytest.fixture(scope="module")
def lib():
    return tc.bind(C.CDLL(af.LIB_PATH))


def _plan(lib, exp, hop, rate, n, batch=1, limit=0, table=False):
    p = tc.Plan()
    k, a = (np.full(1 << 16, -7, np.int32), np.full(1 << 16, -7, np.float32)) if table else (None, None)
    st = lib.afx_timestretch_plan(exp, hop, C.c_float(rate), n, batch, limit, C.byref(p), tc.ptr(k) if table else None,
                                  tc.ptr(a) if table else None)
    return (st, p, k, a) if table else (st, p)


def _capacities():
    """rows (exp, hop, n, rate, capacity) of the reference: computed by it where it is present, else the fixture's"""
    rows = tc.golden()["lengths"]
    ref = tc.ref_lib()
    if ref is None:
        return rows
    rows = rows.copy()
    objs = {}
    for r in rows:
        key = (int(r[0]), int(r[1]))
        if key not in objs:
            objs[key] = tc.new(ref, dict(exp=key[0], hop=key[1]))[1]
        r[4] = ref.timeStretchObj_calDataCapacity(objs[key], C.c_float(r[3]), int(r[2]))
    for o in objs.values():
        ref.timeStretchObj_free(o)
    return rows


def test_plan_lengths_are_the_references(lib):
    rows = _capacities()
    assert len(rows) == 3 * 12 * 31 and rows[:, 3].min() == 0.5 and rows[:, 3].max() == 2.0
    for exp, hop, n, rate, cap in rows:
        exp, hop, n, cap = int(exp), int(hop), int(n), int(cap)
        st, p = _plan(lib, exp, hop, rate, n)
        assert st == 0, (exp, n, rate)
        N = 1 << exp
        T1 = (n - N) // hop + 1
        T2 = int(np.ceil(np.float32(T1) / np.float32(rate)))  # phase_vocoder.c:35
        assert (p.fftLength, p.slideLength, p.T1, p.T2, p.istftLength) == (N, hop, T1, T2, (T2 - 1) * hop + N), (exp, n, rate)
        assert p.capacity == cap and p.returnLength == tc.roundf(n, rate), (exp, n, rate, p.capacity, cap)
        assert p.istftLength <= p.capacity
        assert p.scratchBytes >= 4 * (2 * T2 * N + 2 * T1 * (N // 2 + 1) + p.istftLength) and p.clipsPerChunk == 1


def test_case_lengths_are_the_references(lib):
    """the returned length and the capacity of every case, as the reference's object answers them"""
    for name, c in tc.CASES.items():
        ret, cap, out = tc.expected(name)
        st, p = _plan(lib, c["exp"], c["hop"], c["rate"], c["n"])
        assert st == 0 and (p.returnLength, p.capacity, p.istftLength) == (ret, cap, len(out)), name
        assert (p.T1, p.T2) == tc.lengths(c, c["rate"])[:2]


@pytest.mark.parametrize("rate", [0.5, 0.7, 0.8, 1.0, 1.25, 1.3, 1.5, 1.7, 2.0, 0.05, 37.5])
def test_time_table_is_the_float32_statement(rate, lib):
    """k[i] = floorf(i * rate), alpha[i] = i * rate - floorf(i * rate) with the product rounded to float32 (flux_vector.c:2186)"""
    st, p, k, a = _plan(lib, 8, 64, rate, 30000, table=True)
    assert st == 0 and 0 < p.T2 < len(k)
    t = np.arange(p.T2, dtype=np.float32) * np.float32(rate)
    assert t.dtype == np.float32
    assert np.array_equal(k[:p.T2], np.floor(t).astype(np.int32)) and np.array_equal(a[:p.T2], t - np.floor(t))
    assert (k[p.T2:] == -7).all() and (a[p.T2:] == -7).all()
    assert k[p.T2 - 1] <= p.T1 and ((a[:p.T2] >= 0) & (a[:p.T2] < 1)).all()


def test_chunks_follow_the_scratch_limit(lib):
    st, p = _plan(lib, 12, 1024, 0.8, 1323000, batch=1000)  # 30 s at 44.1 kHz: tens of MB a clip
    assert st == 0 and 30e6 < p.scratchBytes < 120e6
    assert p.clipsPerChunk == (4 << 30) // p.scratchBytes >= 32
    assert _plan(lib, 12, 1024, 0.8, 1323000, batch=3)[1].clipsPerChunk == 3
    assert _plan(lib, 12, 1024, 0.8, 1323000, batch=1000, limit=1)[1].clipsPerChunk == 1
    assert _plan(lib, 12, 1024, 0.8, 1323000, batch=1000, limit=5 * p.scratchBytes + 1)[1].clipsPerChunk == 5
    assert _plan(lib, 8, 64, 0.8, 3000, batch=1 << 20, limit=1 << 40)[1].clipsPerChunk == 65535  # (the vocoder's launch limit)


def test_refusals(lib):
    assert lib.afx_timestretch_plan(8, 64, C.c_float(0.8), 3000, 1, 0, None, None, None) == -6
    for exp, hop in ((15, 64), (30, 64), (8, 257), (4, 17)):
        assert _plan(lib, exp, hop, 0.8, 1 << 20)[0] == -4, (exp, hop)
    for rate in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):
        assert _plan(lib, 8, 64, rate, 3000)[0] == -6, rate
    for n in (255, 0, -5):
        assert _plan(lib, 8, 64, 0.8, n)[0] == -6, n
    assert _plan(lib, 8, 64, 1e-6, 3000)[0] == -6   # 43e6 output frames: beyond the sizes a call takes
    assert _plan(lib, 8, 256, 1.0, 256)[0] == 0      # one frame, no overlap
    st, p = _plan(lib, 0, 0, 1.0, 8192)              # the constructor's defaults: 2^12, hop 1024
    assert st == 0 and (p.fftLength, p.slideLength, p.T1) == (4096, 1024, 5)


def test_exported_names(lib):
    for name in ("timeStretchObj_new", "timeStretchObj_calDataCapacity", "timeStretchObj_timeStretch", "timeStretchObj_free",
                 "timeStretchObj_timeStretchBatchDevice", "timeStretchObj_setScratchLimit", "pitchShiftObj_new",
                 "pitchShiftObj_pitchShift", "pitchShiftObj__free", "pitchShiftObj_pitchShiftBatchDevice",
                 "pitchShiftObj_setScratchLimit", "afx_phase_vocoder_device", "afx_timestretch_plan"):
        assert hasattr(lib, name), name
    assert af.TimeStretch is not None and af.PitchShift is not None
