"""The device-pointer contract of include/afx_batch.h as a table-driven harness (a plain module: tests/test_device_contract_gpu.py
runs it on the GPU through torch buffers, tests/test_device_contract_emulated.py on the CPU through malloc'ed buffers against the
sanitized emulated kernels).

What a value-parity test cannot see, and this can:
  * extent    -- every output lives in an Arena [guard | payload | guard] pre-filled with a SENTINEL (a quiet-NaN bit pattern no
                 arithmetic produces, compared as integers).  After the call the guards and every word outside the documented
                 extent (row-pitch padding, `capped` tails, whole buffers of a zero-frame call) still hold it, and every word
                 inside a `store` output does not -- so an output the kernel forgot cannot hide behind the previous call's value
                 in a recycled allocation.
  * poison    -- every input word outside [b * stride, b * stride + length) is NaN / +Inf / 3e38 (guards included; the last clip
                 ends on the last payload word): results are bit-equal to the zero-padded baseline, i.e. depend only on the samples.
  * alignment -- buffers at any 4-byte offset from a 256-byte boundary.
  * history   -- a bigger, longer, 100 x louder call on the same object first; results bit-equal to a fresh object's.

A Row names the entry point, builds the object and yields a Case: input buffers, output buffers with their kind, and a closure
making the raw ctypes call from pointers and strides.  A new entry point is covered by adding rows (tests/
test_device_contract_emulated.py::test_registry_covers_every_device_entry_point compares the table with the header)."""
import ctypes as C
import os
import re
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

import audioflux_amd as af
from audioflux_amd import _util
from audioflux_amd.spectral import SpectralRequest, request
from oracle import restate
from tests import hpss_cases as hc
from tests import hpss_restate as hr
from tests import pitch_restate as pr
from tests.conftest import HOSTSTUB, l2_rel, peak_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.uint32(0x7FC5A3E1)
POISONS = {"nan": SENTINEL, "inf": np.uint32(0x7F800000), "3e38": np.float32(3e38).view(np.uint32)}
HELD = np.float32(0.375)  # what a read-modify-write output holds before the call
GPU_GUARD_WORDS = 1 << 18  # 1 MiB on each side: a stray access by a whole tile stays inside the allocation
P, I32 = C.c_void_p, C.c_int
LL = C.c_longlong


# ---------------------------------------------------------------------------------------------------------------- arenas
class Arena:
    """`words` 32-bit words at word offset `offset` from a 256-byte boundary, between two guards.  backend "torch": device
    memory, guards of 1 MiB; "numpy": host memory (the emulated libraries take host pointers), small guards; "tight": host
    memory from malloc with NO guard -- the payload ends on the last byte of the allocation, so under AddressSanitizer a read
    or write one word outside is a report (the start is exact for offset 0; an offset k leaves k words of slack in front)."""

    def __init__(self, backend, words, offset=0, fill=SENTINEL):
        self.backend, self.words, self.offset = backend, int(words), int(offset)
        if backend == "torch":
            import torch
            self.guard = GPU_GUARD_WORDS
            self._t = torch.empty(2 * self.guard + self.offset + self.words + 64, dtype=torch.int32, device="cuda")
            assert self._t.data_ptr() % 256 == 0
            self._base = self._t.data_ptr()
            self._t.fill_(int(np.uint32(fill).view(np.int32)))
            self._lo = self.guard + self.offset
        elif backend == "numpy":
            self.guard = 256
            raw = np.empty(2 * self.guard + self.offset + self.words + 128, np.uint32)
            skip = (-raw.ctypes.data // 4) % 64
            self._a = raw[skip:]
            self._a[:] = fill
            self._base = self._a.ctypes.data
            assert self._base % 256 == 0
            self._lo = self.guard + self.offset
        else:
            assert backend == "tight"
            self.guard = 0
            libc = C.CDLL(None)
            libc.malloc.restype, libc.malloc.argtypes = C.c_void_p, [C.c_size_t]
            libc.free.argtypes = [C.c_void_p]
            n = max(self.offset + self.words, 1)
            self._libc, self._mem = libc, libc.malloc(4 * n)
            assert self._mem
            self._a = np.ctypeslib.as_array((C.c_uint32 * n).from_address(self._mem))
            self._a[:] = fill
            self._base = self._mem
            self._lo = self.offset

    def __del__(self):
        if getattr(self, "_mem", None):
            self._a = None
            self._libc.free(self._mem)
            self._mem = None

    def ptr(self, offset_words=0):
        return self._base + 4 * (self._lo + int(offset_words))

    def _all(self):
        return self._t.cpu().numpy().view(np.uint32) if self.backend == "torch" else np.asarray(self._a)

    def write(self, payload):
        payload = np.ascontiguousarray(payload).view(np.uint32).ravel()
        assert payload.size == self.words
        if self.backend == "torch":
            import torch
            self._t[self._lo:self._lo + self.words] = torch.from_numpy(payload.view(np.int32).copy()).cuda()
        else:
            self._a[self._lo:self._lo + self.words] = payload

    def read(self):
        return self._all()[self._lo:self._lo + self.words].copy()

    def guards_intact(self, fill=SENTINEL):
        a = self._all()
        return bool((a[:self._lo] == fill).all() and (a[self._lo + self.words:] == fill).all())

    @staticmethod
    def mask(rows, length, stride, words):
        """the words of `rows` rows of `length` words, row r at r * stride"""
        m = np.zeros(words, bool)
        for r in range(rows):
            m[r * stride:r * stride + length] = True
        return m

    def unwritten(self, mask):
        """True when every word under the mask still holds the sentinel"""
        return bool((self.read()[mask] == SENTINEL).all())

    def written(self, mask):
        """True when no word under the mask holds the sentinel any more"""
        return bool((self.read()[mask] != SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass
class In:
    data: np.ndarray            # [rows, length], float32 (or int32)
    strided: bool = False       # the API takes this buffer's row stride (clipStride / chunkStride)


@dataclass
class Out:
    rows: int
    length: int
    kind: str = "store"         # store | rmw | capped | untouched (a call that must write nothing) | null (optional, passed NULL)
    strided: bool = False       # the API takes this buffer's row stride (outStride / dataStride)
    count: Optional[str] = None  # capped: the output holding the per-row counts; rows are [frames, pitch]
    bitwise: bool = True        # False: accumulated with float atomics, compared by the fraction-of-cells rule
    gain: Optional[np.ndarray] = None   # rmw: [length], what the buffer held comes back multiplied by (inverse STFT: 1 / sum w^2)


@dataclass
class Case:
    ins: dict
    outs: dict
    call: Callable              # (ptr: dict, stride: dict, stream) -> status
    anchor: Optional[Callable] = None   # (res: dict name -> float32 [rows, length]) asserts the values
    keep: list = field(default_factory=list)
    loose: Optional[float] = None       # peak-rel bar where a different kernel may run for another alignment (documented per row)
    istft_norm: Optional[tuple] = None  # (gain, normaliser) of tests/conftest.py::assert_istft_parity for the loose comparison
    host: Optional[Callable] = None     # the one-clip host call on the same object (history: alternated with the device call)


@dataclass
class Row:
    entry: str                  # the prototype in afx_batch.h
    ident: str
    make: Callable              # () -> object
    case: Callable              # (object, big: bool) -> Case; big = more clips, longer clips, 100 x the amplitude
    doc: str = ""
    emulated: bool = False      # device code of this row exists in the emulated contract library
    env: Optional[dict] = None  # needs its own process with these variables

    def __str__(self):
        return f"{self.entry}[{self.ident}]"


def run(case, backend, stream=None, in_off=0, in_gap=0, poison=None, out_off=0, out_gap=0, sync=None, check=True, held=False):
    """one call of `case` on fresh arenas; returns {output: uint32 [rows, length]} after asserting the extent rules"""
    ptr, stride, arenas = {}, {}, {}
    fill_in = np.uint32(0) if poison is None else POISONS[poison]
    for name, b in case.ins.items():
        d = np.ascontiguousarray(b.data)
        rows, length = d.shape if b.strided else (1, d.size)
        st = length + (in_gap if b.strided else 0)
        words = (rows - 1) * st + length
        a = Arena(backend, words, in_off, fill=fill_in)
        pay = np.full(words, fill_in, np.uint32)
        for r in range(rows):
            pay[r * st:r * st + length] = d.reshape(rows, length)[r].view(np.uint32)
        a.write(pay)
        arenas[name], ptr[name], stride[name] = a, a.ptr(), st
    for name, o in case.outs.items():
        if o.kind == "null":
            ptr[name], stride[name] = None, o.length
            continue
        st = o.length + (out_gap if o.strided else 0)
        words = max((o.rows - 1) * st + o.length + (out_gap if o.strided else 0), 0)
        a = Arena(backend, words, out_off)
        if o.kind == "rmw" and words:
            pay = np.full(words, SENTINEL, np.uint32)
            pay[Arena.mask(o.rows, o.length, st, words)] = HELD.view(np.uint32) if held else np.uint32(0)
            a.write(pay)
        arenas[name], ptr[name], stride[name] = a, a.ptr(), st
    status = case.call(ptr, stride, stream)
    assert status == 0, f"status {status}: {af.last_error()}"
    if sync:
        sync()
    res = {}
    for name, o in case.outs.items():
        if o.kind == "null":
            continue
        a, st = arenas[name], stride[name]
        raw = a.read()
        m = Arena.mask(o.rows, o.length, st, a.words) if o.kind != "untouched" else np.zeros(a.words, bool)
        res[name] = np.stack([raw[r * st:r * st + o.length] for r in range(o.rows)]) if o.rows and o.kind != "untouched" \
            else np.zeros((0, o.length), np.uint32)
        if HOSTSTUB or not check:
            continue
        assert a.guards_intact(), f"{name}: a guard word changed (a store outside the buffer)"
        assert a.unwritten(~m), f"{name}: a word outside the documented extent was written (stride {st}, length {o.length})"
        if o.kind == "store":
            assert a.written(m), f"{name}: {int((raw[m] == SENTINEL).sum())} promised words were not written"
    for name, o in case.outs.items():
        if o.kind == "capped" and not HOSTSTUB and check:
            cnt = np.minimum(res[o.count].view(np.int32).ravel(), o.length)
            lead = np.arange(o.length)[None, :] < cnt[:, None]
            assert (res[name][lead] != SENTINEL).all(), f"{name}: a listed entry was not written"
            assert (res[name][~lead] == SENTINEL).all(), f"{name}: an entry beyond min(dLen, troughPitch) was written"
    for name, a in arenas.items():
        if name in case.ins and not HOSTSTUB and check:
            assert a.guards_intact(fill_in) and (a.read() == _payload_of(case.ins[name], stride[name], fill_in)).all(), \
                f"{name}: the input buffer was modified"
    return res


def _payload_of(b, st, fill):
    d = np.ascontiguousarray(b.data)
    rows, length = d.shape if b.strided else (1, d.size)
    pay = np.full((rows - 1) * st + length, fill, np.uint32)
    for r in range(rows):
        pay[r * st:r * st + length] = d.reshape(rows, length)[r].view(np.uint32)
    return pay


def f32(res, name, shape=None):
    a = res[name].view(np.float32)
    return a.reshape(shape) if shape is not None else a


def same(case, got, want, what):
    """bit equality per output; scatter outputs (float atomics: the order of the additions is not fixed) by the rule of their
    own test files -- at most 0.1 % of the cells further than 1e-5 of the peak apart"""
    if HOSTSTUB:
        return
    for name, o in case.outs.items():
        if o.kind in ("null", "untouched"):
            continue
        if o.bitwise and o.kind != "capped":
            bad = got[name] != want[name]
            assert not bad.any(), f"{what}: {name} differs in {int(bad.sum())} of {bad.size} words (first at {np.argwhere(bad)[0]})"
        elif o.kind == "capped":
            keep = want[name] != SENTINEL
            assert ((got[name] != SENTINEL) == keep).all() and (got[name][keep] == want[name][keep]).all(), f"{what}: {name}"
        else:
            a, b = got[name].view(np.float32).astype(np.float64), want[name].view(np.float32).astype(np.float64)
            far = np.abs(a - b) > 1e-5 * max(np.abs(b).max(), 1e-30)
            assert np.isfinite(a).all() and far.mean() <= 1e-3, f"{what}: {name}: {far.mean():.2e} of the cells differ"


def close(case, got, want, what, tol):
    """the parity bar where another kernel instantiation runs; per row of the output (descriptor slots have their own scales).
    The inverse STFT (case.istft_norm): tests/conftest.py::assert_istft_parity per clip, its conditioning-aware bar"""
    if HOSTSTUB:
        return
    for name, o in case.outs.items():
        if o.kind in ("store", "rmw"):
            a, b = got[name].view(np.float32), want[name].view(np.float32)
            assert np.isfinite(a).all(), f"{what}: {name} is not finite"
            for r in range(a.shape[0]):
                if case.istft_norm is not None:
                    from tests.conftest import assert_istft_parity
                    assert_istft_parity(a[r], b[r].astype(np.float64), case.istft_norm, f"{what}: {name} clip {r}")
                else:
                    assert peak_rel(a[r], b[r]) <= tol, f"{what}: {name} row {r} peak-rel {peak_rel(a[r], b[r]):.3e} > {tol}"


def parity(got, want, what, tol=1e-5):
    if HOSTSTUB:
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    p, l = peak_rel(got, want), l2_rel(got, want)
    assert p <= tol and l <= tol, f"{what}: peak-rel {p:.3e}, l2-rel {l:.3e} > {tol}"


# ---------------------------------------------------------------------------------------------------------------- bindings
_SIG = {
    "bftObj_bftBatchDevice": [P, P, I32, I32, LL, P, P, P],
    "xxccObj_xxccDevice": [P, P, LL, I32, C.POINTER(I32), P, P],
    "afx_bftXxccBatchDevice": [P, P, P, I32, I32, LL, I32, C.POINTER(I32), P, P, P],
    "cwtObj_cwtBatchDevice": [P, P, I32, LL, P, P, P],
    "cwtObj_cwtDetBatchDevice": [P, P, I32, LL, P, P, P],
    "cqtObj_cqtBatchDevice": [P, P, I32, I32, LL, P, P, P],
    "cqtObj_chromaBatchDevice": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32), P, P, LL, P, P],
    "cqtObj_cqtChromaBatchDevice": [P, P, I32, I32, LL, P, P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32), P, P],
    "cepstrogramObj_cepstrogramBatchDevice": [P, I32, P, I32, I32, LL, P, P, P, P],
    "pwtObj_pwtBatchDevice": [P, P, I32, LL, P, P, P],
    "wsstObj_wsstBatchDevice": [P, P, I32, LL, P, P, P, P, P],
    "reassignObj_reassignBatchDevice": [P, P, I32, I32, LL, P, P, P, P, P],
    "spectrogramObj_spectrogramBatchDevice": [P, P, I32, I32, LL, P, P],
    "stftObj_stftBatchDevice": [P, P, I32, I32, LL, P, P, P],
    "stftObj_istftBatchDevice": [P, P, P, I32, I32, I32, P, LL, P],
    "spectralObj_computeDevice": [P, P, P, LL, I32, C.POINTER(SpectralRequest), I32, P, LL, P],
    "hpssObj_hpssBatchDevice": [P, P, I32, I32, LL, P, P, LL, P],
    "hpssObj_spectraBatchDevice": [P, P, I32, I32, LL, P, P, P],
    "afx_medianFilterDevice": [P, LL, I32, I32, I32, I32, P, P],
    "pitchYINObj_pitchBatchDevice": [P, P, I32, I32, LL, P, P, P, LL, P],
    "pitchYINObj_troughsBatchDevice": [P, P, I32, I32, LL, P, P, P, I32, P],
    "pitchYINObj_curveBatchDevice": [P, P, I32, I32, LL, P, P],
}
NOT_COVERED = {"afx_gather"}  # needs a communicator of several ranks: tests/test_dist_gpu.py


def fn(name):
    f = getattr(af.get_lib(), name)
    f.restype, f.argtypes = I32, _SIG[name]
    return f


def header_device_entry_points():
    """the names of every prototype of afx_batch.h that takes device pointers on a stream"""
    src = open(os.path.join(ROOT, "include", "afx_batch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\bint\s+(\w+)\s*\(([^;{]*?void\s*\*\s*hipStream[^;{]*?)\)\s*;", src)
    return {n for n, args in names if n != "afx_clock_probe_start"}


# ---------------------------------------------------------------------------------------------------------------- inputs
def clips(batch, n, seed, amp=0.1):
    """noise + two tones per clip: every bin and every frame carries signal"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = rng.standard_normal((batch, n)) + 2.0 * np.sin(2 * np.pi * 0.013 * t) + np.sin(2 * np.pi * 0.11 * t + 1.0)
    return (amp * x).astype(np.float32)


def _size(big, batch, n, grow):
    """(batch, samples, amplitude) of the row's call, or of the bigger, longer, louder one that goes first in the history check"""
    return (batch + 2, n + grow, 10.0) if big else (batch, n, 0.1)


# ---------------------------------------------------------------------------------------------------------------- rows
ROWS = []


def row(entry, ident, make, doc, **kw):
    def deco(case):
        ROWS.append(Row(entry, ident, make, case, doc, **kw))
        return case
    return deco


def _mel(num, r, hop, sr=16000, rt=1, dt=af.SpectralDataType.POWER, **kw):
    def make():
        o = af.BFT(num, radix2_exp=r, samplate=sr, low_fre=0.0, high_fre=sr / 2.0, slide_length=hop,
                   scale_type=kw.pop("scale", af.SpectralFilterBankScaleType.MEL), data_type=dt, **kw)
        o.set_result_type(rt)
        return o
    return make


def _bft_row(ident, make, r, hop, frames, batch, doc, kind=None, extra=0, anchor_mel=None):
    n = (1 << r) + hop * (frames - 1) + extra

    @row("bftObj_bftBatchDevice", ident, make, doc)
    def case(o, big=False):
        b, m, amp = _size(big, batch, n, 3 * hop + 1)
        if kind is not None:
            assert o.fused_plan_kind() == kind, (ident, o.fused_plan_kind())
        x = clips(b, m, 11, amp)
        t = o.cal_time_length(m)
        outs = {"real": Out(b, t * o.num)}
        outs["imag"] = Out(b, t * o.num) if o.result_type == 0 else Out(0, 0, "null")

        def call(p, s, stream):
            return fn("bftObj_bftBatchDevice")(o._obj, p["x"], b, m, s["x"], p["real"], p["imag"], stream)

        def anchor(res):
            got = f32(res, "real", (b, t, o.num))
            if anchor_mel:
                bank, _, _ = restate.mel_bank(o.num, 1 << r, anchor_mel, 0.0, anchor_mel / 2.0)
                parity(got[0], restate.bft(x[0].astype(np.float64), bank, 1 << r, hop), ident)
            else:
                h = o.bft(x[0], result_type=o.result_type)
                h = h if o.result_type == 1 else h.real
                parity(got[0], np.asarray(h).T, ident)
        return Case({"x": In(x, True)}, outs, call, anchor)


_bft_row("mel128-2048-whole", _mel(128, 11, 512), 11, 512, 17, 3, "k_stft_mel_v2, whole-row plan (kind 1)", 1, 5, 16000)
_bft_row("mel128-2048-T1", _mel(128, 11, 512), 11, 512, 1, 1, "k_stft_mel_v2, one frame", 1, 0, 16000)
_bft_row("mel40-2048-split", _mel(40, 11, 512), 11, 512, 9, 3, "k_stft_mel_v2 with rows cut into segments (kind 2)", 2, 3, 16000)
_bft_row("mel128-512", _mel(128, 9, 160), 9, 160, 33, 3, "afx_melfused512.hip (kind 301), odd clip length", 301, 1, 16000)
_bft_row("mel128-1024", _mel(128, 10, 256), 10, 256, 15, 3, "afx_melfused1k.hip (kind 101)", 101, 7, 16000)
_bft_row("mel128-4096", _mel(128, 12, 1024), 12, 1024, 5, 3, "afx_melfused4k2.hip (kind 201)", 201, 9, 16000)
_bft_row("mel64-256-generic", _mel(64, 8, 64), 8, 64, 31, 3, "size-generic: afx_stft256.hip + bank kernels (kind 0)", 0, 1, 16000)
_bft_row("mel128-8192-generic", _mel(128, 13, 2048), 13, 2048, 3, 1, "size-generic n_fft 8192 (kind 0)", 0, 2, 16000)
_bft_row("linear-2048", _mel(200, 11, 512, scale=af.SpectralFilterBankScaleType.LINEAR, dt=af.SpectralDataType.MAG), 11, 512, 9, 3,
         "linear scale: a bin slice of the STFT rows")
_bft_row("gammatone-2048", _mel(128, 11, 512, scale=af.SpectralFilterBankScaleType.ERB,
                               style_type=af.SpectralFilterBankStyleType.GAMMATONE), 11, 512, 9, 3,
         "dense bank: STFT rows -> pitched scratch -> k_gemm_nt128_bf16x3 / k_gemm_nt128 (kind 0)", 0, 1)
_bft_row("mel128-2048-complex", _mel(128, 11, 512, rt=0), 11, 512, 9, 3, "result type 0: complex filter-bank output")
_bft_row("mel128-2048-temporal", _mel(128, 11, 512, is_temporal=True), 11, 512, 9, 3, "isTemporal: the frame statistics ride along")


def _cc_rows(ident, num, r, hop, frames, cc_num, rectify, want_mel, doc, one_launch=None):
    n = (1 << r) + hop * (frames - 1) + 3

    def make():
        return _mel(num, r, hop)(), af.XXCC(num)

    @row("afx_bftXxccBatchDevice", ident, make, doc)
    def case(o, big=False):
        bft, xx = o
        b, m, amp = _size(big, 3, n, 2 * hop + 1)
        x = clips(b, m, 12, amp)
        t = bft.cal_time_length(m)
        outs = {"mel": Out(b, t * num) if want_mel else Out(0, 0, "null"), "cc": Out(b, t * cc_num)}
        lib = af.get_lib()
        lib.afx_bftXxccOneLaunchCount.restype = LL

        def call(p, s, stream):
            before = lib.afx_bftXxccOneLaunchCount()
            st = fn("afx_bftXxccBatchDevice")(bft._obj, xx._obj, p["x"], b, m, s["x"], cc_num, _util.opt_int(rectify), p["mel"],
                                              p["cc"], stream)
            if one_launch is not None and not HOSTSTUB and st == 0:
                assert lib.afx_bftXxccOneLaunchCount() - before == one_launch, ident
            return st

        def anchor(res):
            bank, _, _ = restate.mel_bank(num, 1 << r, 16000, 0.0, 8000.0)
            mel = restate.bft(x[0].astype(np.float64), bank, 1 << r, hop)
            if want_mel:
                parity(f32(res, "mel", (b, t, num))[0], mel, ident + " mel")
            parity(f32(res, "cc", (b, t, cc_num))[0], restate.xxcc(mel, cc_num, "log" if rectify == 0 else "cubic_root"), ident + " cc")
        return Case({"x": In(x, True)}, outs, call, anchor)


_cc_rows("headline", 128, 11, 512, 17, 13, 0, True, "k_stft_mel_v2 with the cepstra in its epilogue: one launch", 1)
_cc_rows("headline-nomel", 128, 11, 512, 16, 13, 0, False, "the same with dMel == NULL", 1)
_cc_rows("1024-T21", 128, 10, 256, 21, 13, 0, True, "afx_ccblock.h behind afx_melfused1k.hip, T not a multiple of 16", 1)
_cc_rows("cuberoot", 128, 11, 512, 15, 13, 1, True, "cube-root rectification")
_cc_rows("cc20-two-launches", 128, 11, 512, 17, 20, 0, True, "ccNum 20: bank kernel + k_xxcc", 0)


def _xxcc_row(ident, num, rows_, cc_num, rectify, doc):
    @row("xxccObj_xxccDevice", ident, lambda: af.XXCC(num), doc)
    def case(o, big=False):
        rows = rows_ * 3 + 5 if big else rows_
        mel = (np.abs(clips(rows, num, 13, 10.0 if big else 0.1)) + 1e-3).astype(np.float32)

        def call(p, s, stream):
            return fn("xxccObj_xxccDevice")(o._obj, p["m"], rows, cc_num, _util.opt_int(rectify), p["cc"], stream)

        def anchor(res):
            parity(f32(res, "cc", (rows, cc_num)), restate.xxcc(mel.astype(np.float64), cc_num, "log" if rectify == 0 else "cubic_root"), ident)
        # afx_cepstrum.hip:142 takes the 16-byte row loads only for a 16-byte-aligned dIn; other addresses go through k_xxcc,
        # another summation order: the entry point's 1e-5 bar instead of bit equality
        return Case({"m": In(mel)}, {"cc": Out(1, rows * cc_num)}, call, anchor, loose=1e-5)


_xxcc_row("128x13-T17", 128, 17, 13, 0, "afx_cepstrum.hip:142, the 16-row tile + 1")
_xxcc_row("128x13-T16", 128, 16, 13, 0, "afx_cepstrum.hip, exactly one tile")
_xxcc_row("40x20-cuberoot", 40, 15, 20, 1, "afx_xxcc.hip generic, cube root, tile - 1")


def _stft_row(ident, r, hop, frames, batch, doc, extra=1, window=af.WindowType.HANN, emulated=False):
    n = (1 << r) + hop * (frames - 1) + extra
    nf = 1 << r

    @row("stftObj_stftBatchDevice", ident, lambda: af.STFT(radix2_exp=r, window_type=window, slide_length=hop), doc, emulated=emulated)
    def case(o, big=False):
        b, m, amp = _size(big, batch, n, 2 * hop + 1)
        x = clips(b, m, 14, amp)
        t = o.cal_time_length(m)

        def call(p, s, stream):
            return fn("stftObj_stftBatchDevice")(o._obj, p["x"], b, m, s["x"], p["re"], p["im"], stream)

        def anchor(res):
            want = restate.stft(x[0].astype(np.float64), nf, hop, int(window))
            got = f32(res, "re", (b, t, nf))[0] + 1j * f32(res, "im", (b, t, nf))[0]
            parity(got[:, :nf // 2 + 1], want, ident)
            parity(got[:, nf // 2 + 1:], np.conj(want[:, 1:nf // 2][:, ::-1]), ident + " mirrored half")
        return Case({"x": In(x, True)}, {"re": Out(b, t * nf), "im": Out(b, t * nf)}, call, anchor, host=lambda: o.stft_full(100.0 * x[0]))


_stft_row("256-T7-odd", 8, 64, 7, 3, "afx_stft256.hip: frame pairs, odd T (the last frame alone)")
_stft_row("256-T8-even", 8, 64, 8, 1, "afx_stft256.hip: frame pairs, even T")
_stft_row("256-T1", 8, 77, 1, 3, "afx_stft256.hip: one frame")
_stft_row("2048-full", 11, 512, 9, 3, "afx_stft.hip:377 wave kernel, full-spectrum rows (vecOut and its complement)")
_stft_row("2048-oddhop", 11, 333, 6, 3, "afx_stft.hip wave kernel, odd hop: the dword loads")
_stft_row("4096", 12, 1024, 4, 3, "afx_stft.hip wave kernel at 4096")
_stft_row("8192-generic", 13, 2048, 3, 1, "afx_stft.hip size-generic kernels")


def _istft_row(ident, r, hop, frames, batch, doc, emulated=True):
    nf = 1 << r

    @row("stftObj_istftBatchDevice", ident, lambda: af.STFT(radix2_exp=r, window_type=af.WindowType.HANN, slide_length=hop), doc,
         emulated=emulated)
    def case(o, big=False):
        b, t = (batch + 2, frames + 3) if big else (batch, frames)
        m = (t - 1) * hop + nf
        x = clips(b, m, 15, 10.0 if big else 0.1)
        spec = np.stack([restate.stft_full(x[c].astype(np.float64), nf, hop, restate.fft_window(int(af.WindowType.HANN), nf)) for c in range(b)])
        re, im = spec.real.astype(np.float32).reshape(b, -1), spec.imag.astype(np.float32).reshape(b, -1)

        def call(p, s, stream):
            return fn("stftObj_istftBatchDevice")(o._obj, p["re"], p["im"], b, t, 0, p["y"], s["y"], stream)

        def anchor(res):
            got = f32(res, "y", (b, m))
            core = slice(nf, m - nf) if m > 3 * nf else slice(nf // 2, m - nf // 2)
            parity(got[:, core], x[:, core], ident + " (interior: the window sum is well conditioned)", 2e-5)
        # afx_istft.hip:690-695: the fused wave kernels need 8-byte-aligned planes, other addresses take the generic inverse
        # (afxk_istft): the bar of tests/conftest.py::assert_istft_parity instead of bit equality
        gn = restate.istft_norm(t, nf, hop, restate.fft_window(int(af.WindowType.HANN), nf))
        return Case({"re": In(re), "im": In(im)}, {"y": Out(b, m, "rmw", strided=True, gain=1.0 / gn[1])}, call, anchor, loose=1e-5,
                    istft_norm=gn)


_istft_row("256-T9", 8, 64, 9, 3, "afx_istft.hip:690 at n_fft 256 (k_istft_w256: frame pairs, odd T)")
_istft_row("256-T8", 8, 64, 8, 1, "k_istft_w256, even T")
_istft_row("2048-T6", 11, 512, 6, 3, "afx_istft.hip fused wave kernel at 2048")


def _spectrogram_row(ident, make, r, hop, frames, doc):
    n = (1 << r) + hop * (frames - 1) + 5

    @row("spectrogramObj_spectrogramBatchDevice", ident, make, doc)
    def case(o, big=False):
        b, m, amp = _size(big, 3, n, 2 * hop + 1)
        x = clips(b, m, 16, amp)
        t = (m - (1 << r)) // hop + 1

        def call(p, s, stream):
            return fn("spectrogramObj_spectrogramBatchDevice")(o._obj, p["x"], b, m, s["x"], p["out"], stream)

        def anchor(res):
            parity(f32(res, "out", (b, t, o.num))[0], np.asarray(o.spectrogram(x[0])).T, ident + " against the one-clip host call")
        return Case({"x": In(x, True)}, {"out": Out(b, t * o.num)}, call, anchor)


_spectrogram_row("mel-2048", lambda: af.Spectrogram(num=128, samplate=16000, low_fre=0.0, high_fre=8000.0, radix2_exp=11,
                                                    window_type=af.WindowType.HANN, slide_length=512,
                                                    filter_bank_type=af.SpectralFilterBankScaleType.MEL), 11, 512, 9,
                 "banded: the fused STFT -> filter-bank kernel inside a spectrogram object")
_spectrogram_row("linear-1024", lambda: af.Linear(samplate=16000, radix2_exp=10), 10, 256, 9, "linear: the bin slice")
_spectrogram_row("chroma-2048", lambda: af.Chroma(samplate=16000, radix2_exp=11), 11, 512, 9, "chroma: dense 12-row bank")


def _cqt_rows(ident, n, batch, doc, env=None):
    def make():
        return af.CQT(num=84, samplate=32000)

    def shapes(o, big):
        b, m, amp = _size(big, batch, n, 4096 + 77)
        return b, m, clips(b, m, 17, amp), o.cal_time_length(m)

    @row("cqtObj_cqtBatchDevice", ident, make, doc, env=env)
    def cqt_case(o, big=False):
        b, m, x, t = shapes(o, big)

        def call(p, s, stream):
            return fn("cqtObj_cqtBatchDevice")(o._obj, p["x"], b, m, s["x"], p["re"], p["im"], stream)

        def anchor(res):
            got = f32(res, "re", (b, t, 84))[0] + 1j * f32(res, "im", (b, t, 84))[0]
            # (the f16 matrix-core octave kernels: the bar of tests/test_cqt_gpu.py against float64)
            parity(got, restate.cqt(x[0].astype(np.float64), num=84, samplate=32000, min_fre=float(np.float32(32.703)), normal="area"), ident, 1e-4 if m < 4096 else 2e-5)
        return Case({"x": In(x, True)}, {"re": Out(b, t * 84), "im": Out(b, t * 84)}, call, anchor)

    @row("cqtObj_cqtChromaBatchDevice", ident, make, doc + "; chroma-12 folded in", env=env)
    def cc_case(o, big=False):
        b, m, x, t = shapes(o, big)

        def call(p, s, stream):
            return fn("cqtObj_cqtChromaBatchDevice")(o._obj, p["x"], b, m, s["x"], p["re"], p["im"], None, None, None, p["ch"], stream)

        def anchor(res):
            q = restate.cqt(x[0].astype(np.float64), num=84, samplate=32000, min_fre=float(np.float32(32.703)), normal="area")
            parity(f32(res, "ch", (b, t, 12))[0], restate.cqt_chroma(q), ident + " chroma", 1e-4 if m < 4096 else 2e-5)
        return Case({"x": In(x, True)}, {"re": Out(b, t * 84), "im": Out(b, t * 84), "ch": Out(b, t * 12)}, call, anchor)


_cqt_rows("pyramid-T33", 32 * 512 + 300, 3, "k_cqt_pyramid: 33 frames, the clip ends mid-tile")
_cqt_rows("pyramid-T32", 31 * 512 + 1, 1, "k_cqt_pyramid: exactly one tile of 32 frames")
_cqt_rows("pyramid-short", 700, 3, "k_cqt_pyramid: a clip shorter than one window")
_cqt_rows("ladder-T33", 32 * 512 + 300, 3, "AFX_CQT_PYRAMID=0: k_cqt_decimate + k_cqt_octave_f16 per octave", env={"AFX_CQT_PYRAMID": "0"})


def _chroma_row(ident, rows_, chroma_num, doc):
    @row("cqtObj_chromaBatchDevice", ident, lambda: af.CQT(num=84, samplate=32000), doc)
    def case(o, big=False):
        rows = rows_ * 2 + 3 if big else rows_
        q = clips(2, rows * 84, 18, 10.0 if big else 0.1).reshape(2, rows, 84)

        def call(p, s, stream):
            return fn("cqtObj_chromaBatchDevice")(o._obj, _util.opt_int(chroma_num), None, None, p["re"], p["im"], rows, p["ch"], stream)

        def anchor(res):
            parity(f32(res, "ch", (rows, chroma_num)), restate.cqt_chroma(q[0].astype(np.float64) + 1j * q[1], chroma_num), ident)
        return Case({"re": In(q[0].reshape(1, -1)), "im": In(q[1].reshape(1, -1))}, {"ch": Out(1, rows * chroma_num)}, call, anchor)


_chroma_row("12-T33", 33, 12, "k_cqt_chroma, tile + 1")
_chroma_row("12-T1", 1, 12, "k_cqt_chroma, one frame")


def _wavelet_rows(ident, cls, entry, r, doc, stride_extra=0, det=False, **kw):
    n = 1 << r

    def make():
        o = cls(radix2_exp=r, samplate=16000, **kw)
        if det:
            o.enable_det(True)
        return o

    @row(entry, ident, make, doc)
    def case(o, big=False):
        b, amp = (4, 10.0) if big else (2, 0.1)
        x = clips(b, n + stride_extra, 19, amp)[:, :n].copy()

        def call(p, s, stream):
            return fn(entry)(o._obj, p["x"], b, s["x"], p["re"], p["im"], stream)

        def anchor(res):
            got = f32(res, "re", (b, o.num, n))[0] + 1j * f32(res, "im", (b, o.num, n))[0]
            name = {"cwtObj_cwtBatchDevice": "cwt", "cwtObj_cwtDetBatchDevice": "cwt_det", "pwtObj_pwtBatchDevice": "pwt"}[entry]
            h = np.asarray(getattr(o, name)(x[0]))
            if not HOSTSTUB:
                assert min(peak_rel(got, h), peak_rel(got, h[::-1])) <= 1e-5, ident + " against the one-chunk host call"
        return Case({"x": In(x, True)}, {"re": Out(b, o.num * n), "im": Out(b, o.num * n)}, call, anchor)


_wavelet_rows("morlet-narrow-4096", af.CWT, "cwtObj_cwtBatchDevice", 12, "afx_cwt.hip narrow-band plan (Morlet, octave scale)",
              num=84, wavelet_type=af.WaveletContinueType.MORLET)
_wavelet_rows("paul-wide-4096", af.CWT, "cwtObj_cwtBatchDevice", 12, "afx_cwt.hip wide-band wavelet: the full-length inverse",
              num=36, wavelet_type=af.WaveletContinueType.PAUL)
_wavelet_rows("morse-1024-td", af.CWT, "cwtObj_cwtBatchDevice", 10, "afx_cwt_td.hip: the time-domain path of small chunks",
              num=48, wavelet_type=af.WaveletContinueType.MORSE)
_wavelet_rows("morlet-det-4096", af.CWT, "cwtObj_cwtDetBatchDevice", 12, "the d/dt planes", num=84,
              wavelet_type=af.WaveletContinueType.MORLET, det=True)
_wavelet_rows("pwt-4096", af.PWT, "pwtObj_pwtBatchDevice", 12, "afx_cwt.hip through the PWT bank, bands ascending", num=84)


def _wsst_row(ident, r, with_cwt, doc, **kw):
    n = 1 << r

    @row("wsstObj_wsstBatchDevice", ident, lambda: af.WSST(radix2_exp=r, samplate=16000, **kw), doc)
    def case(o, big=False):
        b, amp = (4, 10.0) if big else (2, 0.1)
        x = clips(b, n, 20, amp)
        outs = {"sre": Out(b, o.num * n, "rmw", bitwise=False), "sim": Out(b, o.num * n, "rmw", bitwise=False)}
        for k in ("wre", "wim"):
            outs[k] = Out(b, o.num * n) if with_cwt else Out(0, 0, "null")

        def call(p, s, stream):
            return fn("wsstObj_wsstBatchDevice")(o._obj, p["x"], b, s["x"], p["sre"], p["sim"], p["wre"], p["wim"], stream)

        def anchor(res):
            got = f32(res, "sre", (b, o.num, n))[0] + 1j * f32(res, "sim", (b, o.num, n))[0]
            h = np.asarray(o.wsst_raw(x[0])[0])
            if not HOSTSTUB:  # (scatter: the rule of tests/test_wsst_gpu.py, fraction of cells)
                far = np.minimum(np.abs(got - h), np.abs(got - h[::-1])) > 1e-5 * np.abs(h).max()
                assert np.isfinite(got).all() and far.mean() <= 1e-3, (ident, far.mean())
        return Case({"x": In(x, True)}, outs, call, anchor)


_wsst_row("morlet-4096", 12, False, "afx_wsst.hip: k_wsst scatter with atomics onto caller-zeroed planes", num=84)
_wsst_row("morlet-4096-cwt", 12, True, "the same with the CWT planes stored", num=84)


def _reassign_row(ident, r, hop, frames, order, with_stft, doc):
    nf = 1 << r
    n = nf + hop * (frames - 1) + 3

    def make():
        o = af.Reassign(radix2_exp=r, samplate=16000, slide_length=hop)
        if order != 1:
            o.set_order(order)
        return o

    @row("reassignObj_reassignBatchDevice", ident, make, doc)
    def case(o, big=False):
        b, m, amp = _size(big, 2, n, 2 * hop + 1)
        x = clips(b, m, 21, amp)
        t, f = o.cal_time_length(m), nf // 2 + 1
        outs = {"re": Out(b, t * f, "rmw", bitwise=False), "im": Out(b, t * f, "rmw", bitwise=False)}
        for k in ("sre", "sim"):
            outs[k] = Out(b, t * f) if with_stft else Out(0, 0, "null")

        def call(p, s, stream):
            return fn("reassignObj_reassignBatchDevice")(o._obj, p["x"], b, m, s["x"], p["re"], p["im"], p["sre"], p["sim"], stream)

        def anchor(res):
            if with_stft:
                want = restate.stft(x[0].astype(np.float64), nf, hop, int(af.WindowType.HANN))
                parity(f32(res, "sre", (b, t, f))[0] + 1j * f32(res, "sim", (b, t, f))[0], want, ident + " stft planes")
            got = f32(res, "re", (b, t, f))[0] + 1j * f32(res, "im", (b, t, f))[0]
            a = o.reassign_raw(x[0])
            h = a[0] + 1j * a[1]
            if not HOSTSTUB:  # (scatter: the rule of tests/test_reassign_gpu.py, fraction of cells)
                far = np.abs(got - h) > 1e-5 * np.abs(h).max()
                assert np.isfinite(got).all() and far.mean() <= 1e-3, (ident, far.mean())
        return Case({"x": In(x, True)}, outs, call, anchor)


_reassign_row("1024-order1", 10, 256, 9, 1, False, "afx_reassign.hip order 1, scatter with atomics")
_reassign_row("1024-order1-stft", 10, 256, 9, 1, True, "order 1 with the STFT planes stored")
_reassign_row("1024-order2-stft", 10, 256, 8, 2, True, "order 2 (the sorted scatter) with the STFT planes")


def _cep_row(ident, r, hop, frames, cep_num, doc, extra=1):
    nf = 1 << r
    n = nf + hop * (frames - 1) + extra

    @row("cepstrogramObj_cepstrogramBatchDevice", ident,
         lambda: af.Cepstrogram(radix2_exp=r, samplate=16000, window_type=af.WindowType.HANN, slide_length=hop), doc)
    def case(o, big=False):
        b, m, amp = _size(big, 3, n, 2 * hop + 1)
        x = clips(b, m, 22, amp)
        t, f = o.cal_time_length(m), nf // 2 + 1

        def call(p, s, stream):
            return fn("cepstrogramObj_cepstrogramBatchDevice")(o._obj, cep_num, p["x"], b, m, s["x"], p["c"], p["e"], p["d"], stream)

        def anchor(res):
            h = o.cepstrogram(x[0], cep_num)  # (two float32 routes to the same numbers: twice the 1e-5 bar of either)
            for k, name in enumerate("ced"):
                parity(f32(res, name, (b, t, f))[0], np.asarray(h[k]).T, f"{ident} {name} against the one-clip host call", 2e-5)
        # (the `aligned` switch of the wave kernels loads the same samples as float2 / float4 or as scalars into the same
        # arithmetic: bit equality across alignments)
        return Case({"x": In(x, True)}, {k: Out(b, t * f) for k in "ced"}, call, anchor, host=lambda: o.cepstrogram(x[0], cep_num))


_cep_row("2048-cep16", 11, 512, 17, 16, "k_cepstrogram_wave (n_fft 2048), direct lifter (cepNum <= 16), 16 rows + 1")
_cep_row("2048-cep0", 11, 512, 16, 0, "k_cepstrogram_wave (n_fft 2048), cepNum 0")
_cep_row("2048-cep20", 11, 512, 15, 20, "k_cepstrogram_wave (n_fft 2048), cepNum > 16: the non-direct lifter branch")
_cep_row("2048-oddhop", 11, 333, 9, 16, "k_cepstrogram_wave (n_fft 2048), odd hop: the scalar loads")
_cep_row("4096-cep16", 12, 1024, 5, 16, "the n_fft 4096 wave kernel")
_cep_row("1024-wsmall", 10, 333, 9, 16, "k_cepstrogram_wsmall<Fft1k>, odd hop")
_cep_row("512-wsmall-cep0", 9, 128, 15, 0, "k_cepstrogram_wsmall<Fft512>, odd row pitch (257 bins), cepNum 0")
_cep_row("1024-generic-cep17", 10, 256, 9, 17, "k_cepstrogram (size-generic): cepNum 17 at n_fft 1024")
_cep_row("256-generic", 8, 64, 17, 8, "k_cepstrogram (size-generic) at n_fft 256, odd row pitch (129 bins)")
_cep_row("8192-generic", 13, 2048, 3, 16, "k_cepstrogram (size-generic) at n_fft 8192")


def _spectral_row(ident, num, rows_, fpc, reqs, doc, edge=None, phase=True, loose=None):
    def make():
        o = af.Spectral(num, np.linspace(0, 8000, num, dtype=np.float32))
        if edge is not None:
            o.set_edge_arr(np.asarray(edge, np.int32))
        return o

    @row("spectralObj_computeDevice", ident, make, doc, emulated=True)
    def case(o, big=False):
        rows = (rows_ // max(fpc, 1) + 2) * max(fpc, 1) if big and fpc else (rows_ * 2 + 3 if big else rows_)
        spec = (np.abs(clips(rows, num, 23, 10.0 if big else 0.1)) + 1e-4).astype(np.float32)
        ph = np.random.default_rng(24).uniform(-np.pi, np.pi, (rows, num)).astype(np.float32)
        arr = (SpectralRequest * len(reqs))(*reqs)
        slots = af.get_lib().afx_spectralSlots(arr, len(reqs))
        assert slots > 0

        def call(p, s, stream):
            return fn("spectralObj_computeDevice")(o._obj, p["spec"], p["phase"] if phase else None, rows, fpc, arr, len(reqs),
                                                   p["out"], s["out"], stream)

        def anchor(res):
            # every slot of the list against the float64 restatement, clip by clip (the frame differences restart)
            from tests import spectral_cases as sc_
            from tests import spectral_restate as sr_
            if HOSTSTUB:
                return
            got = f32(res, "out", (slots, rows))
            idx = np.asarray(edge) if edge is not None else np.arange(num)
            fre = np.linspace(0, 8000, num, dtype=np.float32).astype(np.float64)
            step = fpc if fpc else rows
            slot = 0
            for q in reqs:
                kind = sc_.KINDS[q.kind]
                parts = [sr_.restate(kind, list(q.iarg), list(q.farg), spec[c:c + step].astype(np.float64),
                                     ph[c:c + step].astype(np.float64) if phase else None, fre, idx, num) for c in range(0, rows, step)]
                for k in range(len(parts[0])):
                    want = np.concatenate([np.asarray(pt[k], np.float64).ravel() for pt in parts])
                    g = got[slot].astype(np.float64)
                    if kind in sc_.DISCRETE:  # decided by a comparison: a frame on the threshold may fall either way
                        assert (g == want).mean() >= 0.9, f"{ident} {kind}: {(g != want).sum()} of {rows} frames differ"
                    else:
                        assert np.isfinite(g).all() and np.abs(g - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-30), \
                            f"{ident} {kind} slot {slot}: {np.abs(g - want).max() / max(np.abs(want).max(), 1e-30):.3e} of the peak"
                    slot += 1
            assert slot == slots
        ins = {"spec": In(spec)}
        if phase:
            ins["phase"] = In(ph)
        # afx_descriptors.hip:728: 16-byte row loads for 16-byte-aligned rows, dword loads otherwise -- another summation order
        return Case(ins, {"out": Out(slots, rows, strided=True)}, call, anchor, keep=[arr], loose=loose)


def _slot_of(reqs, i):
    return sum(2 if q.kind >= 27 else 1 for q in reqs[:i])


_MIXED = [request(3), request(0), request(1, (1, 0, 0, 0), (2.0,)), request(18), request(27), request(12)]
_spectral_row("mixed-128", 128, 37, 0, _MIXED, "k_desc_rows<..> + k_desc_frames + phase + MAX (two slots), one clip; 16-byte row "
              "loads for 16-byte-aligned rows, dword loads otherwise (another summation order: 1e-5 across alignments)", loose=1e-5)
_spectral_row("mixed-128-clips", 128, 36, 12, _MIXED, "the same, framesPerClip 12: the frame differences restart", loose=1e-5)
_spectral_row("mixed-1025", 1025, 9, 0, _MIXED, "k_desc_rows_long, odd row length: dword loads")
_spectral_row("edge-table-40", 40, 17, 0, [request(3), request(2, (), (0.9,)), request(4)], "the index-table forms (setEdgeArr)",
              edge=[1, 2, 3, 5, 8, 13, 21, 34], phase=False)


def _hpss_make(r, h, p, hop=None):
    return lambda: af.HPSS(radix2_exp=r, window_type=af.WindowType.HAMM, slide_length=hop or (1 << r) // 4, h_order=h, p_order=p)


def _hpss_rows(ident, r, frames, batch, h, p, doc, which="hp", env=None, short=False):
    nf, hop = 1 << r, (1 << r) // 4
    n = nf - 5 if short else nf + hop * (frames - 1) + 3

    @row("hpssObj_hpssBatchDevice", ident, _hpss_make(r, h, p), doc, emulated=True, env=env)
    def wave_case(o, big=False):
        b, m, amp = _size(big, batch, n, 3 * hop + 1)
        x = clips(b, m, 25, amp)
        ml = o.cal_data_length(m) if m >= nf else 0
        kind = "rmw" if ml else "untouched"
        gain = 1.0 / restate.istft_norm(o.cal_time_length(m), nf, hop, hr.window(hc.HAMM, nf))[1] if ml else None
        outs = {"h": Out(b, ml or 64, kind, strided=True, gain=gain) if "h" in which else Out(0, 0, "null"),
                "p": Out(b, ml or 64, kind, strided=True, gain=gain) if "p" in which else Out(0, 0, "null")}

        def call(pt, s, stream):
            return fn("hpssObj_hpssBatchDevice")(o._obj, pt["x"], b, m, s["x"], pt["h"], pt["p"],
                                                 s["h" if "h" in which else "p"], stream)

        def anchor(res):
            if not ml or HOSTSTUB:
                return
            from tests.hpss_check import check_waveform
            wh, wp = hr.hpss(x[0].astype(np.float64), r, hc.HAMM, h, p)
            for k, w in (("h", wh), ("p", wp)):
                if k in which:
                    check_waveform(f"{ident}/{k}", f32(res, k, (b, ml))[0], w, np.abs(x[0]).max(), r, hc.HAMM)
        return Case({"x": In(x, True)}, outs, call, anchor)

    @row("hpssObj_spectraBatchDevice", ident, _hpss_make(r, h, p), doc + "; the masked magnitude planes", emulated=True, env=env)
    def mag_case(o, big=False):
        b, m, amp = _size(big, batch, n, 3 * hop + 1)
        x = clips(b, m, 25, amp)
        t, f = (o.cal_time_length(m) if m >= nf else 0), nf // 2 + 1
        kind = "store" if t else "untouched"
        outs = {"h": Out(b, t * f or 64, kind) if "h" in which else Out(0, 0, "null"),
                "p": Out(b, t * f or 64, kind) if "p" in which else Out(0, 0, "null")}

        def call(pt, s, stream):
            return fn("hpssObj_spectraBatchDevice")(o._obj, pt["x"], b, m, s["x"], pt["h"], pt["p"], stream)

        def anchor(res):
            if not t or HOSTSTUB:
                return
            _, mag, wh, wp = hr.spectra(x[0].astype(np.float64), r, hc.HAMM, h, p)
            for k, w in (("h", wh), ("p", wp)):
                if k in which:
                    assert np.abs(f32(res, k, (b, t, f))[0] - w).max() <= 1e-5 * mag.max(), ident
        return Case({"x": In(x, True)}, outs, call, anchor)


_hpss_rows("512-T63", 9, 63, 3, 21, 31, "k_hpss_tile<HPSS, 21, 31>, 64-frame tile - 1")
_hpss_rows("512-T64", 9, 64, 1, 21, 31, "k_hpss_tile, exactly one tile")
_hpss_rows("512-T65-honly", 9, 65, 3, 21, 31, "tile + 1, dP == NULL", which="h")
_hpss_rows("512-T65-ponly", 9, 65, 1, 21, 31, "tile + 1, dH == NULL", which="p")
_hpss_rows("256-T40-order63", 8, 40, 3, 63, 63, "k_hpss_tile<HPSS, 63, 63>: the widest orders of the separation kernel")
_hpss_rows("512-short", 9, 0, 3, 21, 31, "dataLength < fftLength: nothing is written", short=True)
_hpss_rows("512-T65-chunked", 9, 65, 3, 21, 31, "AFX_HPSS_CHUNK_MB=1: chunks of whole clips through one scratch",
           env={"AFX_HPSS_CHUNK_MB": "1"})


def _median_row(ident, rows_, cols, fpc, axis, order, doc):
    @row("afx_medianFilterDevice", ident, lambda: None, doc, emulated=True)
    def case(o, big=False):
        rows = rows_ + (fpc or 7) * 2 if big else rows_
        plane = (clips(rows, cols, 26, 10.0 if big else 0.1) ** 2).astype(np.float32)

        def call(p, s, stream):
            return fn("afx_medianFilterDevice")(p["in"], rows, cols, fpc, axis, order, p["out"], stream)

        def anchor(res):
            want = hr.median_filter(plane, axis, order, fpc)
            assert HOSTSTUB or np.array_equal(f32(res, "out", (rows, cols)).view(np.uint32), want.view(np.uint32)), ident
        return Case({"in": In(plane)}, {"out": Out(1, rows * cols)}, call, anchor)


_median_row("axis0-31-65x129", 65, 129, 0, 0, 31, "k_hpss_tile<AXIS0, 31>, tile + 1 both ways")
_median_row("axis1-31-63x127", 63, 127, 0, 1, 31, "k_hpss_tile<AXIS1, 31>, tile - 1 both ways")
_median_row("axis0-101-clips", 3 * 23 + 7, 40, 23, 0, 101, "k_median_rank along the frames, clips of 23 frames + a short one")
_median_row("axis1-101-64x128", 64, 128, 0, 1, 101, "k_median_rank along the bins, exactly one tile")


def _pitch_make(r, hop, auto, sr=16000):
    def make():
        o = af.PitchYIN(samplate=sr, low_fre=60.0, high_fre=1000.0, radix2_exp=r, slide_length=hop, auto_length=auto)
        o.set_thresh(0.3)
        return o
    return make


def _voiced(batch, n, amp, sr=16000):
    t = np.arange(n) / sr
    rng = np.random.default_rng(27)
    # (300 Hz and up: several periods fit below the longest lag, so every frame has more troughs than troughPitch 1 keeps)
    return np.stack([amp * (np.sin(2 * np.pi * (300.0 + 37 * c) * t) + 0.4 * np.sin(2 * np.pi * (600.0 + 74 * c) * t)
                            + 0.02 * rng.standard_normal(n)) for c in range(batch)]).astype(np.float32)


def _pitch_rows(ident, r, hop, frames, batch, pitch_, doc, nulls=False, short=False):
    nf = 1 << r
    auto = nf // 2
    n = nf - 3 if short else nf + hop * (frames - 1) + 5

    def shapes(o, big):
        b, m, amp = _size(big, batch, n, 2 * hop + 3)
        return b, m, _voiced(b, m, amp), (o.cal_time_length(m) if m >= nf else 0)

    @row("pitchYINObj_pitchBatchDevice", ident, _pitch_make(r, hop, auto), doc, emulated=True)
    def pitch_case(o, big=False):
        b, m, x, t = shapes(o, big)
        kind = "store" if t else "untouched"
        outs = {"fre": Out(b, t or 8, kind, strided=True)}
        for k in ("trough", "min"):
            outs[k] = Out(0, 0, "null") if nulls else Out(b, t or 8, kind, strided=True)

        def call(p, s, stream):
            return fn("pitchYINObj_pitchBatchDevice")(o._obj, p["x"], b, m, s["x"], p["fre"], p["trough"], p["min"], s["fre"], stream)

        def anchor(res):
            if not t or HOSTSTUB:
                return
            frames_ = pr.pitch(x[0], 16000, r, hop, auto, o.min_index, o.min_index + o.yin_length - 1, 0.3)
            got = f32(res, "fre", (b, t))[0]
            found = [i for i, f in enumerate(frames_) if f.get("found")]
            assert found, ident + ": the fixture has no voiced frame"
            # (a frame whose curve grazes the threshold may decide either way in float32: all but one in ten must agree)
            ok = [i for i in found if abs(got[i] - frames_[i]["fre"]) <= 1e-3 * frames_[i]["fre"]]
            assert len(ok) >= 0.9 * len(found), (ident, len(ok), len(found))
        return Case({"x": In(x, True)}, outs, call, anchor)

    @row("pitchYINObj_troughsBatchDevice", ident, _pitch_make(r, hop, auto), doc + "; the capped candidate lists", emulated=True)
    def troughs_case(o, big=False):
        b, m, x, t = shapes(o, big)
        kind = "capped" if t else "untouched"
        outs = {"fre": Out(b * t or 1, pitch_ if t else 8, kind, count="len"), "val": Out(b * t or 1, pitch_ if t else 8, kind, count="len"),
                "len": Out(1, b * t or 8, "store" if t else "untouched")}

        def call(p, s, stream):
            return fn("pitchYINObj_troughsBatchDevice")(o._obj, p["x"], b, m, s["x"], p["fre"], p["val"], p["len"], pitch_, stream)

        def anchor(res):
            if not t or HOSTSTUB:
                return
            frames_ = pr.pitch(x[0], 16000, r, hop, auto, o.min_index, o.min_index + o.yin_length - 1, 0.3)
            lens = res["len"].view(np.int32).ravel()[:t]
            agree = sum(int(lens[i]) == len(f["hits"]) for i, f in enumerate(frames_))
            assert agree >= 0.9 * t, (ident, agree, t)
            assert (lens > pitch_).any() or pitch_ > 1, ident + ": the cap was never reached"
        return Case({"x": In(x, True)}, outs, call, anchor)

    @row("pitchYINObj_curveBatchDevice", ident, _pitch_make(r, hop, auto), doc + "; the difference curve", emulated=True)
    def curve_case(o, big=False):
        b, m, x, t = shapes(o, big)
        yl = o.yin_length

        def call(p, s, stream):
            return fn("pitchYINObj_curveBatchDevice")(o._obj, p["x"], b, m, s["x"], p["yin"], stream)

        def anchor(res):
            if not t or HOSTSTUB:
                return
            frames_ = pr.pitch(x[0], 16000, r, hop, auto, o.min_index, o.min_index + o.yin_length - 1, 0.3)
            got = f32(res, "yin", (b, t, yl))[0]
            for i, f in enumerate(frames_):
                tol = 1e-5 * np.maximum(f["cond"], 1.0) * max(np.abs(f["yin"]).max(), 1.0)
                assert (np.abs(got[i] - f["yin"]) <= tol).all(), (ident, i)
        return Case({"x": In(x, True)}, {"yin": Out(b, t * yl or 8, "store" if t else "untouched")}, call, anchor)


_pitch_rows("1024-T9-pitch4", 10, 256, 9, 3, 4, "k_pitch_yin<10>, troughPitch 4")
_pitch_rows("1024-T1-pitch1", 10, 256, 1, 1, 1, "k_pitch_yin<10>, one frame, troughPitch 1 (the cap bites), optional outputs NULL", nulls=True)
_pitch_rows("4096-T5-pitch1", 12, 1000, 5, 3, 1, "k_pitch_yin<12>, troughPitch 1")
_pitch_rows("1024-short", 10, 256, 0, 3, 4, "fewer samples than one frame: nothing is written", short=True)


def rows(emulated=None, env=False):
    """the table; emulated=True: rows whose device code the emulated contract library holds; env: rows that need their own process"""
    return [r for r in ROWS if (emulated is None or r.emulated == emulated) and (bool(r.env) == env)]


# ---------------------------------------------------------------------------------------------------------------- checks
def check_row(r, backend, stream=None, sync=None, what=("extent", "poison", "alignment", "history", "anchor"), quick=False):
    """every contract check of one row; the baseline is a call on aligned, contiguous, zero-padded buffers.  quick (the
    emulated kernels: one host thread per lane under AddressSanitizer): one poison, two alignments"""
    obj = r.make()
    case = r.case(obj)
    kw = dict(stream=stream, sync=sync)
    base = run(case, backend, **kw)
    if "anchor" in what and case.anchor:
        case.anchor(base)
    rmw = {n for n, o in case.outs.items() if o.kind == "rmw"}
    if "extent" in what:
        got = run(case, backend, out_gap=5, in_gap=3, held=True, **kw)  # (HELD under the read-modify-write outputs)
        same(_without(case, rmw), got, base, f"{r} extent (row pitch + 5)")
        _held_relation(case, got, base, f"{r} extent")
    if "poison" in what:
        for p in list(POISONS)[:1 if quick else None]:
            got = run(case, backend, poison=p, in_gap=7, **kw)
            same(case, got, base, f"{r} poisoned surroundings ({p})")
    if "alignment" in what:
        for in_off, out_off, gap in ((1, 0, 0), (2, 1, 1), (3, 2, 0), (0, 1, 2), (1, 2, 3))[:2 if quick else None]:
            got = run(case, backend, in_off=in_off, out_off=out_off, in_gap=gap, **kw)
            if case.loose is None:
                same(case, got, base, f"{r} input at word offset {in_off}, output at {out_off}, stride + {gap}")
            else:
                close(case, got, base, f"{r} input at word offset {in_off}, output at {out_off}, stride + {gap}", case.loose)
    if "history" in what:
        run(r.case(obj, True), backend, **kw)            # bigger, longer, louder first ...
        got = run(case, backend, **kw)
        same(case, got, base, f"{r} after a bigger, longer, 100 x louder call on the same object")
        if case.host:                                    # ... and the one-clip host call in between
            case.host()
            same(case, run(case, backend, **kw), base, f"{r} after the one-clip host call on the same object")
        fresh = r.make()
        small_first = r.case(fresh)
        run(small_first, backend, **kw)                  # ... and growing after the small call
        big_case = r.case(fresh, True)
        grown = run(big_case, backend, **kw)
        fresh2 = r.make()
        same(big_case, grown, run(r.case(fresh2, True), backend, **kw), f"{r} grown after a small call")
    return base


def _without(case, names):
    c = Case(case.ins, {n: o for n, o in case.outs.items() if n not in names}, case.call)
    return c


def _held_relation(case, got, base, what):
    """read-modify-write outputs, as tests/test_hpss_gpu.py states it: what the buffer held goes through the same division by
    the window sum as the frames, (held + sum of frames) / sum w^2 -- so the result onto HELD minus the result onto zeros is
    HELD x gain in EVERY clip, gain = 1 / sum w^2 (clamped like the library's normaliser); the scatter kernels add: gain 1.
    Bar: 1e-5 of (HELD + the result's peak), times the gain where it exceeds 1 (the float32 rounding of both results reaches
    the difference multiplied by it)"""
    if HOSTSTUB:
        return
    for name, o in case.outs.items():
        if o.kind != "rmw":
            continue
        a = got[name].view(np.float32).astype(np.float64)
        b = base[name].view(np.float32).astype(np.float64)
        assert np.isfinite(a).all(), f"{what}: {name} is not finite"
        d = a - b
        scale = float(HELD) + np.abs(b).max()
        if o.bitwise:
            assert o.gain is not None and o.gain.shape == (o.length,), f"{what}: {name}: the row states no gain"
            tol = 1e-5 * scale * np.maximum(o.gain, 1.0)
            bad = np.abs(d - float(HELD) * o.gain[None, :]) > tol[None, :]
            assert not bad.any(), (f"{what}: {name}: (held + result) / sum w^2 does not hold in {int(bad.sum())} samples, first "
                                   f"{np.argwhere(bad)[0]}: difference {d[bad][0]:.6g}, expected {float(HELD) * o.gain[np.argwhere(bad)[0][1]]:.6g}")
        else:
            assert np.abs(d - float(HELD)).mean() <= 1e-3 * scale, f"{what}: {name}: held + result does not hold"
