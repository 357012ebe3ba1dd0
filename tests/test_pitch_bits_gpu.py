"""GPU: the pitch trackers give the bits they gave before their kernels' shared pieces moved into afx_pitchparts.h (the row
decode, the thread-local first maximum, the workgroup's first argmax) and their host objects onto afx_pitchkit.h.

The moved device code holds integer operations, comparisons and shuffles only, so the check is exact:
tests/golden/pitch_bits.npz holds what the library of the commit before the change wrote for these seeded inputs on an MI355X
(tests/golden/make_pitch_bits.py), and every array must come back bit for bit.  Through the device-pointer calls into outputs
pre-filled with a marked NaN: every element a call owns must be written, nothing behind it.

Cases: the SMALL lists of HPS / LHS and PEF and every YIN case -- single-wave sizes (N = 64: the cross-wave fold is empty) and
multi-wave ones, the HS slice in LDS and in device scratch, the all-zero rows where every candidate ties and minIndex must
come out --; a PEF launch of more rows than its 2048 workgroups and an HS scratch-slice launch of more rows than its 1024
slices (a workgroup takes a second row); one strided batch per tracker against single-clip calls.  Curves are recorded for
N <= 1024, those above 16 KB as their SHA-256."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import pitch_cases as yc
from tests import pitch_hs_cases as hc
from tests import pitch_pef_cases as pc
from tests.golden.make_pitch_golden import bind as yin_bind
from tests.golden.make_pitch_golden import new as yin_new

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pitch_bits.npz")
MARK = 0x7FC0DEAD  # a NaN no arithmetic produces: what a call did not write
TROUGHS = 4        # candidate slots per frame of the YIN lists
ll = C.c_longlong


def bind(lib):
    hc.bind_device(lib)
    pc.bind_device(lib)
    yin_bind(lib)
    v = C.c_void_p
    lib.pitchYINObj_pitchBatchDevice.restype = C.c_int
    lib.pitchYINObj_pitchBatchDevice.argtypes = [v, v, C.c_int, C.c_int, ll, v, v, v, ll, v]
    lib.pitchYINObj_troughsBatchDevice.restype = C.c_int
    lib.pitchYINObj_troughsBatchDevice.argtypes = [v, v, C.c_int, C.c_int, ll, v, v, v, C.c_int, v]
    lib.pitchYINObj_curveBatchDevice.restype = C.c_int
    lib.pitchYINObj_curveBatchDevice.argtypes = [v, v, C.c_int, C.c_int, ll, v, v]
    return lib


class Torch:
    """arrays the library's device-pointer calls read and write: torch tensors on the GPU"""

    def put(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def marked(self, *shape):
        import torch
        return torch.full(shape, MARK, dtype=torch.int32, device="cuda")

    def ptr(self, a):
        return a.data_ptr()

    def get(self, a, dtype=np.float32):
        import torch
        torch.cuda.synchronize()
        return a.cpu().numpy().view(dtype)


class Host(Torch):
    """the same on the host, for a library whose kernels are the device code compiled for the host (tests/emu)"""

    def put(self, x):
        return np.ascontiguousarray(x)

    def marked(self, *shape):
        return np.full(shape, MARK, np.int32)

    def ptr(self, a):
        return a.ctypes.data

    def get(self, a, dtype=np.float32):
        return a.view(dtype)


def written(*arrays):
    for a in arrays:
        assert not (a.view(np.uint32) == MARK).any(), "elements the call owns and did not write"


def curve_record(c):
    """a curve as the fixture holds it: itself up to 16 KB, its SHA-256 above"""
    written(c)
    return c if c.nbytes <= 16384 else np.frombuffer(hashlib.sha256(np.ascontiguousarray(c).tobytes()).digest(), np.uint8)


def pair_batch(dev, call, xs, n, T, pad=0):
    """(fre, value) of a <tracker>Obj_pitchBatchDevice call over the clips xs[:, :n], rows T + pad apart"""
    b = xs.shape[0]
    xd, f, v = dev.put(xs), dev.marked(b, T + pad), dev.marked(b, T + pad)
    assert call(dev.ptr(xd), b, n, xs.shape[1], dev.ptr(f), dev.ptr(v), T + pad, None) == 0
    f, v = dev.get(f), dev.get(v)
    written(f[:, :T], v[:, :T])
    assert (f[:, T:].view(np.uint32) == MARK).all() and (v[:, T:].view(np.uint32) == MARK).all(), "wrote behind a clip's frames"
    return f[:, :T], v[:, :T]


def curve_batch(dev, call, xs, n, T, width):
    b = xs.shape[0]
    xd, c = dev.put(xs), dev.marked(b, T, width)
    assert call(dev.ptr(xd), b, n, xs.shape[1], dev.ptr(c), None) == 0
    return dev.get(c)


def strided(kinds, n, sr, seed):
    """three clips of n samples, 13 floats of another clip's noise between them"""
    xs = yc.signal("noise", 3 * (n + 13), sr, seed=seed).reshape(3, n + 13)
    for c, kind in enumerate(kinds):
        xs[c, :n] = yc.signal(kind, n, sr, seed=seed + 1 + c)
    return xs


def batch_against_singles(dev, call, xs, n, T, out, key):
    """a batch with clipStride > dataLength and outStride > T: bitwise the single-clip calls"""
    f, v = pair_batch(dev, call, xs, n, T, pad=3)
    for c in range(xs.shape[0]):
        f1, v1 = pair_batch(dev, call, np.ascontiguousarray(xs[c:c + 1, :n]), n, T)
        assert np.array_equal(f1.view(np.uint32), f[c:c + 1].view(np.uint32)), (key, c)
        assert np.array_equal(v1.view(np.uint32), v[c:c + 1].view(np.uint32)), (key, c)
    out[key + "/fre"], out[key + "/value"] = f, v
    return f, v


# ---- HPS / LHS ---------------------------------------------------------------------------------------------------------------
def hs_fn(lib, kind, obj, what):
    f = getattr(lib, f"pitch{hc.KIND_NAME[kind]}Obj_{what}")
    return lambda *a: f(obj, *a)


def hs_case(lib, dev, kind, x, params, curve, out, key):
    sr, lo, hi, r, hop, window, count = params
    st, obj = hc.new(lib, kind, sr, lo, hi, r, hop, window, count)
    assert st == 0 and obj, (key, st)
    xs = np.ascontiguousarray(x)[None]
    T = hc.frames(xs.shape[1], r, hop)
    f, v = pair_batch(dev, hs_fn(lib, kind, obj, "pitchBatchDevice"), xs, xs.shape[1], T)
    out[key + "/fre"], out[key + "/value"] = f[0], v[0]
    if curve:
        width = hs_fn(lib, kind, obj, "maxIndex")() + 1
        out[key + "/curve"] = curve_record(curve_batch(dev, hs_fn(lib, kind, obj, "curveBatchDevice"), xs, xs.shape[1], T, width)[0])
    hc.free(lib, kind, obj)


def hs_outputs(lib, dev, big=True):
    out = {}
    for name in hc.SMALL:
        kinds, sr, lo, hi, r, hop, window, count, _, _ = hc.CASES[name]
        for kind in kinds:
            hs_case(lib, dev, kind, hc.case_input(name), (sr, lo, hi, r, hop, window, count), r <= 10, out,
                    f"hs/{name}/{hc.KIND_NAME[kind]}")
    for kind in hc.BOTH:
        k = hc.KIND_NAME[kind]
        if big:  # 1100 rows on the 1024 scratch slices: the parameters of scratch_r12 at hop 16
            _, sr, lo, hi, r, _, window, count, _, _ = hc.CASES["scratch_r12"]
            x = yc.signal("snr:20", (1 << r) + 16 * 1099, sr, seed=310)
            hs_case(lib, dev, kind, x, (sr, lo, hi, r, 16, window, count), False, out, f"hs/scratch_1100_rows/{k}")
        sr, r, hop, n = 16000, 9, 128, 512 + 128 * 5 + 5
        st, obj = hc.new(lib, kind, sr, 40.0, 2000.0, r, hop, hc.HAMM, 4)
        assert st == 0 and obj
        batch_against_singles(dev, hs_fn(lib, kind, obj, "pitchBatchDevice"), strided(("tone:330", "stack:196", "glide"), n, sr, 320),
                              n, hc.frames(n, r, hop), out, f"hs/batch/{k}")
        hc.free(lib, kind, obj)
    return out


# ---- PEF ---------------------------------------------------------------------------------------------------------------------
def pef_fn(lib, obj, what):
    f = getattr(lib, f"pitchPEFObj_{what}")
    return lambda *a: f(obj, *a)


def pef_outputs(lib, dev, big=True):
    out = {}
    for name in pc.SMALL:
        c = pc.CASES[name]
        st, obj = pc.new(lib, *pc.ctor_args(name))
        assert st == 0 and obj, (name, st)
        xs = pc.case_input(name)[None]
        T = pc.frames(xs.shape[1], c[4], c[5])
        f, v = pair_batch(dev, pef_fn(lib, obj, "pitchBatchDevice"), xs, xs.shape[1], T)
        out[f"pef/{name}/fre"], out[f"pef/{name}/value"] = f[0], v[0]
        width = lib.pitchPEFObj_maxIndex(obj) + 1
        out[f"pef/{name}/curve"] = curve_record(curve_batch(dev, pef_fn(lib, obj, "curveBatchDevice"), xs, xs.shape[1], T, width)[0])
        lib.pitchPEFObj_free(obj)
    st, obj = pc.new(lib, *pc.ctor_args("r6_sr8k"))  # N = 64, hop 16
    assert st == 0 and obj
    call = pef_fn(lib, obj, "pitchBatchDevice")
    if big:  # two clips of 20 000 samples: 2 x 1247 rows on 2048 workgroups
        xs = np.stack([yc.signal(kind, 20000, 8000, seed=330 + i) for i, kind in enumerate(("glide", "snr:5"))])
        T = pc.frames(20000, 6, 16)
        assert 2 * T > 2048
        f, v = pair_batch(dev, call, xs, 20000, T)
        out["pef/2494_rows/fre"], out["pef/2494_rows/value"] = f, v
    n = 64 + 16 * 9 + 5
    batch_against_singles(dev, call, strided(("tone:440", "stack:196", "glide"), n, 8000, 340), n, pc.frames(n, 6, 16), out, "pef/batch")
    lib.pitchPEFObj_free(obj)
    return out


# ---- YIN ---------------------------------------------------------------------------------------------------------------------
def yin_calls(lib, dev, obj, xs, n, T, ylen, pad, curve, out, key):
    b, stride = xs.shape
    xd = dev.put(xs)
    f, v, m = (dev.marked(b, T + pad) for _ in range(3))
    assert lib.pitchYINObj_pitchBatchDevice(obj, dev.ptr(xd), b, n, stride, dev.ptr(f), dev.ptr(v), dev.ptr(m), T + pad, None) == 0
    f, v, m = dev.get(f), dev.get(v), dev.get(m)
    written(f[:, :T], v[:, :T], m[:, :T])
    assert all((a[:, T:].view(np.uint32) == MARK).all() for a in (f, v, m)), "wrote behind a clip's frames"
    cf, cv, cl = dev.marked(b, T, TROUGHS), dev.marked(b, T, TROUGHS), dev.marked(b, T)
    assert lib.pitchYINObj_troughsBatchDevice(obj, dev.ptr(xd), b, n, stride, dev.ptr(cf), dev.ptr(cv), dev.ptr(cl), TROUGHS, None) == 0
    cf, cv, cl = dev.get(cf), dev.get(cv), dev.get(cl, np.int32)
    written(cl)
    stored = np.arange(TROUGHS)[None, None, :] < cl[:, :, None]  # the first min(count, TROUGHS) slots are the call's
    for a in (cf, cv):
        assert np.array_equal(a.view(np.uint32) != MARK, stored), "the candidate slots written are not the first min(count, slots)"
    res = {"fre": f[:, :T], "trough": v[:, :T], "min": m[:, :T], "cand_fre": cf, "cand_val": cv, "cand_len": cl}
    if curve:
        c = dev.marked(b, T, ylen)
        assert lib.pitchYINObj_curveBatchDevice(obj, dev.ptr(xd), b, n, stride, dev.ptr(c), None) == 0
        res["curve"] = curve_record(dev.get(c))
    for k, a in res.items():
        out[f"{key}/{k}"] = a
    return res


def yin_outputs(lib, dev):
    out = {}
    for name, (sr, lo, hi, r, hop, auto, thresh, _, n) in yc.CASES.items():
        st, obj = yin_new(lib, sr, lo, hi, r, hop, auto)
        assert st == 0 and obj, (name, st)
        lib.pitchYINObj_setThresh(obj, thresh)
        ylen = yc.plan(sr, lo, hi, r, hop, auto)[2]
        yin_calls(lib, dev, obj, yc.case_input(name)[None], n, yc.frames(n, r, hop), ylen, 0, r <= 10, out, f"yin/{name}")
        lib.pitchYINObj_free(obj)
    sr, r, hop, auto, n = 16000, 9, 128, 256, 512 + 128 * 9 + 5
    st, obj = yin_new(lib, sr, 60.0, 2000.0, r, hop, auto)
    assert st == 0 and obj
    xs, T = strided(("tone:330", "bursts", "glide"), n, sr, 350), yc.frames(n, r, hop)
    ylen = yc.plan(sr, 60.0, 2000.0, r, hop, auto)[2]
    whole = yin_calls(lib, dev, obj, xs, n, T, ylen, 3, False, out, "yin/batch")
    for c in range(3):
        one = yin_calls(lib, dev, obj, np.ascontiguousarray(xs[c:c + 1, :n]), n, T, ylen, 0, False, {}, "")
        for k, a in one.items():
            assert np.array_equal(a.view(np.uint32), whole[k][c:c + 1].view(np.uint32)), ("yin/batch", c, k)
    lib.pitchYINObj_free(obj)
    return out


# ---- the tests ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import audioflux_amd as af
    return bind(af.get_lib())


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def assert_bits(got, golden, family):
    want = {k: a for k, a in golden.items() if k.startswith(family + "/")}
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    for k, a in got.items():
        w = want[k]
        assert a.shape == w.shape and a.dtype == w.dtype, f"{k}: {a.shape} {a.dtype} vs {w.shape} {w.dtype}"
        u = np.uint32 if a.dtype.itemsize == 4 else a.dtype
        same = np.array_equal(a.view(u), w.view(u))
        if not same:
            d = a.view(u) != w.view(u)
            raise AssertionError(f"{k}: {int(d.sum())} of {d.size} values differ from the parent commit's bits, first at "
                                 f"{tuple(np.argwhere(d)[0])}")


def test_hps_lhs_bits(lib, golden):
    assert_bits(hs_outputs(lib, Torch()), golden, "hs")


def test_pef_bits(lib, golden):
    assert_bits(pef_outputs(lib, Torch()), golden, "pef")


def test_yin_bits(lib, golden):
    assert_bits(yin_outputs(lib, Torch()), golden, "yin")
