"""The checks of the onset feature that run twice: on the GPU (tests/test_onset_gpu.py, device memory = torch tensors) and
on the emulated kernels (tests/emu/emulated_onset.py, "device" memory = numpy arrays).  `D` is the memory adapter:
D.put(array) -> buffer, D.ptr(buffer, first_element) -> address, D.get(buffer) -> numpy copy (synchronises).  Every check
compares against tests/onset_restate.py by the rule of tests/onset_check.py; bounds that no fixture case carries use the
rule's floor, eps = 1e-5 -- the smallest yardstick the rule ever grants."""
import ctypes as C

import numpy as np

from tests import onset_cases as oc
from tests import onset_restate as rs
from tests.onset_check import FLOOR, check_case

I32 = np.int32
F32 = np.float32


class NumpyDev:
    """host memory: what the generated stand-in of the device layer calls device memory"""

    @staticmethod
    def put(a):
        return np.array(a, copy=True, order="C")

    @staticmethod
    def ptr(buf, first=0):
        return C.c_void_p(buf.ctypes.data + first * buf.itemsize)

    @staticmethod
    def get(buf):
        return buf.copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def batch_call(lib, D, obj, spec, phase=None, param=None, index=None, out_stride=None, point_stride=None, offset=0, points=True,
               counts=True):
    """onsetObj_onsetBatchDevice on spec [B, T, M] -> status, evn [B, out_stride], pts [B, point_stride], cnt [B]; the buffers
    start `offset` floats behind an aligned base and are filled with sentinels (NaN, -7)"""
    B, T, M = spec.shape
    os_ = T if out_stride is None else out_stride
    ps = T if point_stride is None else point_stride
    ds = D.put(np.concatenate([np.full(offset, np.nan, F32), np.ascontiguousarray(spec, F32).reshape(-1)]))
    dp = None if phase is None else D.put(np.ascontiguousarray(phase, F32).reshape(-1))
    de = D.put(np.full(offset + B * os_, np.nan, F32))
    dpt = D.put(np.full(B * max(ps, 0) + 1, -7, I32))
    dc = D.put(np.full(B + 1, -7, I32))
    par = oc.param_of(param)
    idx, idx_p, idx_n = oc.index_of(index)
    st = lib.onsetObj_onsetBatchDevice(obj, D.ptr(ds, offset), None if dp is None else D.ptr(dp), B,
                                       None if par is None else C.byref(par), idx_p, idx_n, D.ptr(de, offset),
                                       D.ptr(dpt) if points else None, D.ptr(dc) if counts else None, os_, ps, None)
    e, p, c = D.get(de), D.get(dpt), D.get(dc)
    assert np.isnan(e[:offset]).all() and p[-1] == -7 and c[-1] == -7
    return st, e[offset:].reshape(B, os_), p[:-1].reshape(B, max(ps, 0)), c[:-1]


def fixture_case(lib, D, name, gold, ref_lib=None):
    """one case through the host-pointer call and as a batch of one: the rule against the reference (live when ref_lib is given,
    else the fixture)"""
    c = oc.CASES[name]
    spec, phase = oc.case_input(name)
    if ref_lib is not None:
        ref_evn, ref_pts = oc.run_case(ref_lib, name, spec, phase)
        assert same_bits(ref_evn, gold[name + "/evn"]) and np.array_equal(ref_pts, gold[name + "/points"]), name
    pick, delta = rs.pick_params(c["sr"], c["hop"])
    assert pick == gold[name + "/pick"].tolist(), name
    e64 = rs.envelope64(spec, phase, c["kind"], c["order"], c["param"], c["index"])
    st, obj = oc.new(lib, c["T"], c["M"], c["hop"], c["sr"], c["order"], c["kind"])
    assert st == 0 and obj, (name, st)
    n, evn, pts = oc.call(lib, obj, spec, phase, c["param"], c["index"], fill=np.nan)
    assert n == len(pts) >= 0, (name, n)
    st, be, bp, bc = batch_call(lib, D, obj, spec[None], None if phase is None else phase[None], c["param"], c["index"])
    lib.onsetObj_free(obj)
    assert st == 0 and same_bits(be[0], evn) and bc[0] == n and np.array_equal(bp[0, :n], pts) and (bp[0, n:] == -7).all(), name
    w = check_case(name, e64, float(gold[name + "/eps"][0]), gold[name + "/points"], evn, pts, pick, delta)
    print(f"onset {name}: T {c['T']}, M {c['M']}, order {c['order']}, kind {c['kind']}: envelope {w['worst']:.3f} of its bar, "
          f"explained {w['explained']}", flush=True)


def free_case(lib, D, T, M, sr, hop, order=1, kind=oc.FLUX, param=None, index=None, seed=1, spec=None, ref_lib=None):
    """a case no fixture carries, by the rule at its floor; against the live reference too when there is one -> evn, points"""
    if spec is None:
        spec = oc.burst_db(T, M, seed)
    pick, delta = rs.pick_params(sr, hop)
    st, obj = oc.new(lib, T, M, hop, sr, order, kind)
    assert st == 0 and obj, st
    n, evn, pts = oc.call(lib, obj, spec, None, param, index, fill=np.nan)
    lib.onsetObj_free(obj)
    assert n == len(pts) >= 0, n
    e64 = rs.envelope64(spec, None, kind, order, param, index)
    ref_pts = rs.pick(e64, pick, delta, np.float64)
    if ref_lib is not None:
        st, robj = oc.new(ref_lib, T, M, hop, sr, order, kind)
        _, _, ref_pts = oc.call(ref_lib, robj, spec, None, param, index)
        ref_lib.onsetObj_free(robj)
    check_case(f"T {T} M {M} order {order} sr {sr} hop {hop}", e64, FLOOR, ref_pts, evn, pts, pick, delta)
    return evn, pts


def edge_lengths(lib, D, ref_lib=None):
    """T = 1, T = step, T = step + 1"""
    for T, step in ((1, 1), (2, 2), (3, 2), (2, 1)):
        evn, pts = free_case(lib, D, T, 8, 32000, 512, param=(step, 1.0, 1, 0, 0, 0.0, 0, 1.0), seed=40 + T, ref_lib=ref_lib)
        if T == step:
            assert (evn == 0).all() and len(pts) == 0, (T, step, evn)
    print("edge lengths: T = 1, T = step, T = step + 1", flush=True)


def index_tables(lib, D, ref_lib=None):
    """a subset, out of order, with a repeat; then no table again on the same object"""
    free_case(lib, D, 70, 33, 32000, 512, index=[20, 3, 3, 31, 7, 0, 32, 12], seed=51, ref_lib=ref_lib)
    free_case(lib, D, 70, 33, 32000, 512, order=2, kind=oc.HFC, index=[5, 4, 4, 30], seed=52, ref_lib=ref_lib)
    spec = oc.burst_db(50, 12, 53)
    st, obj = oc.new(lib, 50, 12, 512)
    a = oc.call(lib, obj, spec, index=[1, 2, 3])[1]
    b = oc.call(lib, obj, spec, index=[3, 4, 5, 6])[1]
    c = oc.call(lib, obj, spec, index=[1, 2, 3])[1]
    d = oc.call(lib, obj, spec)[1]
    lib.onsetObj_free(obj)
    assert same_bits(a, c) and not same_bits(a, b) and not same_bits(a, d)
    print("index tables: subset, out of order, repeat; a table replaced and dropped on one object", flush=True)


def unknown_kind(lib, D):
    spec = oc.burst_db(60, 16, 61)
    outs = []
    for kind in (oc.FLUX, 11, -3, 1000):
        st, obj = oc.new(lib, 60, 16, 512, kind=kind)
        assert st == 0
        outs.append(oc.call(lib, obj, spec, param=(1, 2.0, 1, 1, 1, 0.0, 0, 1.0)))
        lib.onsetObj_free(obj)
    for n, evn, pts in outs[1:]:
        assert n == outs[0][0] and same_bits(evn, outs[0][1]) and np.array_equal(pts, outs[0][2])
    print("an unknown kind equals flux", flush=True)


def max_filter(lib, D):
    """afx_maxFilterDevice against its restatement, exactly (values: -0 equals +0): rows shorter and longer than a tile of the
    LDS path, more than one tile, the global path, even / odd orders and one larger than the row"""
    rng = np.random.default_rng(7)
    for rows, cols in ((900, 5), (130, 33), (37, 129), (5, 1025), (3, 2100), (1, 1)):
        x = rng.standard_normal((rows, cols)).astype(F32)
        x[rng.random(x.shape) < 0.1] = 0.0
        x[0, :2] = -0.0
        for order in (1, 2, 5, cols + 3, 4 * cols):
            dx, dy = D.put(np.concatenate([[np.nan], x.reshape(-1)]).astype(F32)), D.put(np.full(x.size + 2, np.nan, F32))
            assert lib.afx_maxFilterDevice(D.ptr(dx, 1), rows, cols, order, D.ptr(dy, 1), None) == 0
            y = D.get(dy)
            assert np.isnan(y[0]) and np.isnan(y[-1])
            assert np.array_equal(y[1:-1].reshape(rows, cols), rs.max_filter(x, order)), (rows, cols, order)
    print("max filter: exact at M = 5, 33, 129, 1025, 2100, orders 1, 2, 5 and beyond the row", flush=True)


def peak_pick(lib, D):
    """afx_peakPickDevice against the float32 rule, exactly: lengths around the tile of 256 frames, every parameter at 0 and
    above, negative delta (every frame a candidate: the wait rule alone decides), strided batches, sentinels, a short list"""
    rng = np.random.default_rng(9)
    for n in (1, 2, 255, 256, 257, 700):
        for params, delta in (((1, 1, 6, 7, 1), 0.07), ((0, 1, 0, 1, 0), -1.0), ((3, 2, 10, 11, 3), 0.0), ((0, 3, 2, 1, 4), -1.0),
                              ((5000, 5000, 5000, 5000, 2), 0.01)):
            B, stride = 3, n + 5
            e = rng.random((B, stride)).astype(F32)
            e[1, :n] = np.round(e[1, :n] * 4) / 4  # many bit-equal ties
            e[:, n:] = np.nan
            want = [rs.pick(e[b, :n], params, delta, F32) for b in range(B)]
            ps = max(1, max(len(w) for w in want) - 1)  # shorter than the longest list
            de, dp, dc = D.put(e.reshape(-1)), D.put(np.full(B * ps + 1, -7, I32)), D.put(np.full(B + 1, -7, I32))
            assert lib.afx_peakPickDevice(D.ptr(de), B, n, stride, *params, delta, D.ptr(dp), D.ptr(dc), ps, None) == 0
            p, c = D.get(dp), D.get(dc)
            assert p[-1] == -7 and c[-1] == -7
            for b in range(B):
                k = min(len(want[b]), ps)
                assert c[b] == len(want[b]), (n, params, b, c[b], len(want[b]))
                assert np.array_equal(p[b * ps:b * ps + k], want[b][:k]) and (p[b * ps + k:(b + 1) * ps] == -7).all(), (n, params, b)
    # counts alone, points alone
    e = rng.random(300).astype(F32)
    want = rs.pick(e, (1, 1, 6, 7, 1), 0.07, F32)
    de, dp, dc = D.put(e), D.put(np.full(300, -7, I32)), D.put(np.full(1, -7, I32))
    assert lib.afx_peakPickDevice(D.ptr(de), 1, 300, 300, 1, 1, 6, 7, 1, 0.07, None, D.ptr(dc), 0, None) == 0
    assert lib.afx_peakPickDevice(D.ptr(de), 1, 300, 300, 1, 1, 6, 7, 1, 0.07, D.ptr(dp), None, 300, None) == 0
    assert D.get(dc)[0] == len(want) and np.array_equal(D.get(dp)[:len(want)], want)
    for bad in ((-1, 1, 1, 1, 0), (0, 0, 1, 1, 0), (0, 1, -1, 1, 0), (0, 1, 1, 0, 0), (0, 1, 1, 1, -1)):
        assert lib.afx_peakPickDevice(D.ptr(de), 1, 300, 300, *bad, 0.07, D.ptr(dp), D.ptr(dc), 300, None) == -6, bad
    assert lib.afx_peakPickDevice(D.ptr(de), 1, 300, 299, 1, 1, 6, 7, 1, 0.07, D.ptr(dp), D.ptr(dc), 300, None) == -6
    assert lib.afx_peakPickDevice(D.ptr(de), 1, 300, 300, 1, 1, 6, 7, 1, 0.07, None, None, 300, None) == -6
    print("peak pick: exact at lengths 1 ... 700, every parameter, ties, short lists, sentinels, refusals", flush=True)


def ties(lib, D, ref_lib=None):
    """bit-equal ties: an all-equal plane (zero envelope, no division, no points); rows repeated with period 2 at preMax = 3
    put two equal maxima into one window: rule (b) and the wait rule decide"""
    st, obj = oc.new(lib, 40, 9, 512)
    n, evn, pts = oc.call(lib, obj, np.full((40, 9), -3.25, F32), fill=np.nan)
    lib.onsetObj_free(obj)
    assert n == 0 and (evn == 0).all(), (n, evn)
    rng = np.random.default_rng(3)
    rows = rng.uniform(-60, 0, (2, 12)).astype(F32)
    spec = np.tile(rows, (30, 1))
    spec[31:] += 20  # one step up: a frame that stands out, then the period again
    evn, pts = free_case(lib, D, 60, 12, 44100, 441, spec=spec, ref_lib=ref_lib)
    assert same_bits(evn[2:30:2], np.full(14, evn[2], F32)) and evn[2] != evn[3], evn[:8]  # equal maxima two frames apart
    print(f"ties: an all-equal plane, a period of two rows ({len(pts)} points)", flush=True)


def batches(lib, D):
    """a batch of 3 from a misaligned base: bitwise the single calls, sentinels beyond dCount and beyond a row's frames untouched,
    pointStride smaller than the count, the envelope alone"""
    for order, kind in ((1, oc.FLUX), (3, oc.FLUX), (2, oc.CD)):
        T, M, B = 90, 20, 3
        spec = np.stack([oc.burst_db(T, M, 70 + b) for b in range(B)])
        phase = None
        if oc.needs_phase(kind):
            spec = (spec + 81).astype(F32)
            phase = np.random.default_rng(5).uniform(-3, 3, spec.shape).astype(F32)
        st, obj = oc.new(lib, T, M, 441, 44100, order, kind)
        assert st == 0
        single = [oc.call(lib, obj, spec[b], None if phase is None else phase[b]) for b in range(B)]
        st, e, p, c = batch_call(lib, D, obj, spec, phase, out_stride=T + 3, point_stride=T, offset=1)
        assert st == 0
        for b in range(B):
            n, evn, pts = single[b]
            assert n > 2 and c[b] == n and same_bits(e[b, :T], evn) and np.isnan(e[b, T:]).all(), (order, kind, b)
            assert np.array_equal(p[b, :n], pts) and (p[b, n:] == -7).all(), (order, kind, b)
        ps = min(s[0] for s in single) - 1
        st, e2, p2, c2 = batch_call(lib, D, obj, spec, phase, point_stride=ps)
        assert st == 0 and np.array_equal(c2, c) and all(np.array_equal(p2[b], single[b][2][:ps]) for b in range(B))
        st, e3, p3, c3 = batch_call(lib, D, obj, spec, phase, points=False, counts=False)
        assert st == 0 and same_bits(e3, e[:, :T]) and (p3 == -7).all() and (c3 == -7).all()
        lib.onsetObj_free(obj)
    print("batches of 3 from a misaligned base bitwise the single calls; sentinels; short point lists; envelope alone", flush=True)


def lds_bound(lib, D, bound=8192):
    """one length on each side of the picker's LDS bound, M = 8"""
    for T in (bound, bound + 1):
        spec = oc.burst_db(T, 8, 80)
        evn, pts = free_case(lib, D, T, 8, 32000, 512, spec=spec)
        assert len(pts) > 20
    print(f"LDS bound: {bound} and {bound + 1} frames", flush=True)


class SpectralRequest(C.Structure):
    _fields_ = [("kind", C.c_int), ("iarg", C.c_int * 4), ("farg", C.c_float * 2)]


def envelope_is_normalised_descriptor(lib, D):
    """the envelope is bit for bit float32 (raw - min) / max of spectralObj_computeDevice's flux on the same rows"""
    T, M, B = 75, 24, 2
    spec = np.stack([oc.burst_db(T, M, 90 + b) for b in range(B)])
    lib.spectralObj_new.restype, lib.spectralObj_new.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int, oc.fp]
    lib.spectralObj_free.restype, lib.spectralObj_free.argtypes = None, [C.c_void_p]
    lib.spectralObj_computeDevice.restype = C.c_int
    lib.spectralObj_computeDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.POINTER(SpectralRequest),
                                              C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    sp = C.c_void_p()
    fre = np.arange(M, dtype=F32)
    assert lib.spectralObj_new(C.byref(sp), M, fre.ctypes.data_as(oc.fp)) == 0
    req = SpectralRequest(1, (C.c_int * 4)(1, 1, 0, 0), (C.c_float * 2)(1.0, 0.0))  # AFX_SD_FLUX: step, isPostive, isExp, type / p
    ds, dr = D.put(spec.reshape(-1)), D.put(np.zeros(B * T, F32))
    assert lib.spectralObj_computeDevice(sp, D.ptr(ds), None, B * T, T, C.byref(req), 1, D.ptr(dr), B * T, None) == 0
    raw = D.get(dr).reshape(B, T)
    lib.spectralObj_free(sp)
    st, obj = oc.new(lib, T, M, 512)
    st, e, _, _ = batch_call(lib, D, obj, spec)
    lib.onsetObj_free(obj)
    assert st == 0
    for b in range(B):
        assert raw[b].max() > 0 and same_bits(e[b], rs.normalise(raw[b], F32)), b
    print("the envelope is float32 (raw - min) / max of the descriptor call's flux, bit for bit", flush=True)


def power_to_db(lib, D, gold, ref_lib=None):
    """afx_powerToDbDevice and util_powerToDB against the reference at the project's 1e-5 peak-relative bar; one maximum per
    clip; in place; min >= 0 -> -80"""
    p = oc.burst_power(60, 16, 7).astype(F32)
    want = gold["db/out"]
    if ref_lib is not None:
        live = np.zeros(p.size, F32)
        ref_lib.util_powerToDB(p.reshape(-1).ctypes.data_as(oc.fp), p.size, -80.0, live.ctypes.data_as(oc.fp))
        assert same_bits(live.reshape(p.shape), want)
    host = np.full(p.size, np.nan, F32)
    lib.util_powerToDB(p.reshape(-1).ctypes.data_as(oc.fp), p.size, -80.0, host.ctypes.data_as(oc.fp))
    bar = 1e-5 * np.abs(want).max()
    assert np.abs(host.reshape(p.shape) - want).max() <= bar, np.abs(host.reshape(p.shape) - want).max()
    inplace = p.reshape(-1).copy()
    lib.util_powerToDB(inplace.ctypes.data_as(oc.fp), p.size, 5.0, None)  # in place, min >= 0 -> -80
    assert same_bits(inplace, host)
    # three clips of different level behind a misaligned base, a gap of NaN between them
    n, stride = p.size, p.size + 3
    clips = np.full((3, stride), np.nan, F32)
    for b, g in enumerate((1.0, 1e-3, 40.0)):
        clips[b, :n] = p.reshape(-1) * g
    dx, dy = D.put(np.concatenate([[np.nan], clips.reshape(-1)]).astype(F32)), D.put(np.full(3 * stride + 1, np.nan, F32))
    assert lib.afx_powerToDbDevice(D.ptr(dx, 1), 3, n, stride, -80.0, D.ptr(dy, 1), None) == 0
    y = D.get(dy)[1:].reshape(3, stride)
    assert np.isnan(y[:, n:]).all()
    for b in range(3):
        ref = oc.power_to_db64(clips[b, :n].astype(np.float64)).reshape(p.shape)
        assert np.abs(y[b, :n].reshape(p.shape) - ref).max() <= bar, b
    assert np.abs(y[0, :n].reshape(p.shape) - want).max() <= bar
    assert lib.afx_powerToDbDevice(D.ptr(dx, 1), 3, n, stride, -30.0, D.ptr(dx, 1), None) == 0  # in place, another floor
    z = D.get(dx)[1:].reshape(3, stride)
    assert same_bits(z[:, :n], np.maximum(y[:, :n], F32(-30))) and np.isnan(z[:, n:]).all()
    big = np.abs(np.random.default_rng(2).standard_normal(70001)).astype(F32) + F32(1e-3)  # several partial maxima per clip
    dx, dy = D.put(big), D.put(np.zeros_like(big))
    assert lib.afx_powerToDbDevice(D.ptr(dx), 1, big.size, big.size, -80.0, D.ptr(dy), None) == 0
    assert np.abs(D.get(dy) - oc.power_to_db64(big)).max() <= 1e-5 * 80
    for bad in ((None, 1, 5, 5), (1, 0, 5, 5), (1, 1, 0, 5), (1, 2, 5, 4)):
        assert lib.afx_powerToDbDevice(D.ptr(dx) if bad[0] else None, bad[1], bad[2], bad[3], -80.0, D.ptr(dy), None) == -6, bad
    print("power to dB: host and resident calls at 1e-5 of the peak, one maximum per clip, in place, the floor, refusals", flush=True)


def refusals(lib, D):
    T, M = 20, 6
    spec = oc.burst_db(T, M, 95)
    obj = C.c_void_p()
    assert lib.onsetObj_new(None, T, M, 512, None, None, None) == -1
    for t, m in ((0, M), (T, 0), (-1, M)):
        assert lib.onsetObj_new(C.byref(obj), t, m, 512, None, None, None) == -6 and not obj
    lib.onsetObj_free(None)
    st, obj = oc.new(lib, T, M, 512, kind=oc.WPD)
    assert st == 0
    assert oc.call(lib, obj, spec)[0] == -6  # a phase kind without the phase
    st, _, p, c = batch_call(lib, D, obj, spec[None])
    assert st == -6 and (p == -7).all() and (c == -7).all()
    assert oc.call(lib, obj, spec, spec)[0] >= 0
    lib.onsetObj_free(obj)
    st, obj = oc.new(lib, T, M, 512)
    n, evn, _ = oc.call(lib, obj, spec, param=(T + 1, 1.0, 1, 0, 0, 0.0, 0, 1.0), fill=np.nan)
    assert n == -6 and np.isnan(evn).all()  # step > nLength: nothing written
    assert oc.call(lib, obj, spec, param=(T, 1.0, 1, 0, 0, 0.0, 0, 1.0))[0] == 0
    for index in ([0, M], [-1], [2, 3, 1 << 20]):
        assert oc.call(lib, obj, spec, index=index)[0] == -6, index
        assert batch_call(lib, D, obj, spec[None], index=index)[0] == -6, index
    idx = np.array([1, 2], I32)
    evn, pts = np.zeros(T, F32), np.zeros(T, I32)
    assert lib.onsetObj_onset(obj, spec.ctypes.data_as(oc.fp), None, None, idx.ctypes.data_as(oc.ip), 0, evn.ctypes.data_as(oc.fp),
                              pts.ctypes.data_as(oc.ip)) == -6
    assert lib.onsetObj_onset(None, spec.ctypes.data_as(oc.fp), None, None, None, 0, evn.ctypes.data_as(oc.fp),
                              pts.ctypes.data_as(oc.ip)) == -6
    assert batch_call(lib, D, obj, spec[None], out_stride=T - 1)[0] == -6
    assert batch_call(lib, D, obj, spec[None], point_stride=-1)[0] == -6
    assert lib.onsetObj_onsetBatchDevice(obj, None, None, 1, None, None, 0, None, None, None, T, T, None) == -6
    de = D.put(np.zeros(T, F32))
    assert lib.onsetObj_onsetBatchDevice(obj, D.ptr(de), None, 0, None, None, 0, D.ptr(de), None, None, T, T, None) == -6
    lib.onsetObj_free(obj)
    dx = D.put(np.zeros(12, F32))
    for args in ((None, 3, 4, 2, "y"), ("x", 0, 4, 2, "y"), ("x", 3, 0, 2, "y"), ("x", 3, 4, 0, "y"), ("x", 3, 4, 2, "x"), ("x", 3, 4, 2, None)):
        a = [D.ptr(dx) if v == "x" else D.ptr(de) if v == "y" else v for v in args]
        assert lib.afx_maxFilterDevice(a[0], a[1], a[2], a[3], a[4], None) == -6, args
    assert lib.afx_onset_plan_host(32000, 512, None, None) == -6
    print("refusals: constructor, phase, step, index, strides, NULL pointers, in place", flush=True)
