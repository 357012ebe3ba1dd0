"""One runner for the table of tests/gemm_cases.py and two kinds of memory: device tensors through torch (tests/test_gemm_gpu.py)
or host arrays (tests/emu/emulated_gemm.py: the emulated library takes host pointers).  The products are called by ctypes on
the library's extern "C" launchers: afxk_gemm_nt, afxk_gemm_nt128_bf16, afxk_gemm_bank_prepare + afxk_gemm_nt_bank, afxdev_free.

Every case: status 0; A and B with NaN in the padding of their pitches; C filled with a sentinel -- every word outside [M, N]
still holds it afterwards, every promised element is finite and within the case's bar (tests/gemm_cases.py: max(4e-7, 2 x E32)
against float64)."""
import ctypes as C

import numpy as np

from tests import gemm_cases as gc
from tests.conftest import HOSTSTUB, parity_log

_VP, _LL = C.c_void_p, C.c_longlong


def bind(lib):
    lib.afxk_gemm_nt.restype = C.c_int
    lib.afxk_gemm_nt.argtypes = [_VP, _LL, _VP, C.c_int, _VP, _LL, _LL, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _VP]
    lib.afxk_gemm_nt128_bf16.restype = C.c_int
    lib.afxk_gemm_nt128_bf16.argtypes = [_VP, _LL, _VP, C.c_int, _VP, _LL, _LL, C.c_int, C.c_int, C.c_int, C.c_float, _VP]
    lib.afxk_gemm_bank_prepare.restype = C.c_int
    lib.afxk_gemm_bank_prepare.argtypes = [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(_VP), _VP]
    lib.afxk_gemm_nt_bank.restype = C.c_int
    lib.afxk_gemm_nt_bank.argtypes = [_VP, _LL, _VP, C.c_int, C.c_int, _VP, _LL, _LL, C.c_int, C.c_float, _VP]
    lib.afxdev_free.restype = None
    lib.afxdev_free.argtypes = [_VP]
    return lib


class Buffer:
    """`words` 32-bit words whose first one lies `shift` words behind a 16-byte boundary"""

    def __init__(self, backend, host, shift=0):
        host = np.ascontiguousarray(host).reshape(-1).view(np.uint32)
        self.backend, self.words = backend, host.size
        if backend == "torch":
            import torch
            self._t = torch.empty(host.size + shift + 4, dtype=torch.int32, device="cuda")
            assert self._t.data_ptr() % 16 == 0
            self._v = self._t[shift:shift + host.size]
            self._v.copy_(torch.from_numpy(host.view(np.int32).copy()))
            self.ptr = self._t.data_ptr() + 4 * shift
        else:
            self._raw = np.empty(host.size + shift + 8, np.uint32)
            off = (-self._raw.ctypes.data // 4) % 4 + shift
            self._v = self._raw[off:off + host.size]
            self._v[:] = host
            self.ptr = self._v.ctypes.data
        assert self.ptr % 16 == (4 * shift) % 16

    def read(self):
        if self.backend == "torch":
            return self._v.cpu().numpy().view(np.uint32)
        return self._v.copy()


def _pitched(X, ld):
    P = np.full((X.shape[0], ld), np.nan, np.float32)
    P[:, :X.shape[1]] = X
    return P


class Runner:
    def __init__(self, lib, backend, stream, sync):
        self.lib, self.backend, self.stream, self.sync = bind(lib), backend, stream, sync or (lambda: None)

    def _c(self, M, ldc):
        return Buffer(self.backend, np.full(M * ldc, gc.SENTINEL, np.uint32))

    def _result(self, st, c, M, ldc):
        self.sync()
        return st, c.read().reshape(M, ldc)

    def product(self, kernel, A, B, lda, ldb, ldc, pre=0, post=0, arg=0.0, a_shift=0):
        """(status, C [M, ldc] as uint32 words) of one product through the entry point of `kernel` ("f32", "nt128", "bank")"""
        if kernel == "bank":
            img = self.bank_prepare(B, ldb)
            try:
                return self.bank_product(img, A, B.shape[0], lda, ldc, post, arg, a_shift)
            finally:
                self.lib.afxdev_free(img)
        (M, K), N = A.shape, B.shape[0]
        a, b, c = Buffer(self.backend, _pitched(A, lda), a_shift), Buffer(self.backend, _pitched(B, ldb)), self._c(M, ldc)
        if kernel == "f32":
            st = self.lib.afxk_gemm_nt(a.ptr, lda, b.ptr, ldb, c.ptr, ldc, M, N, K, pre, post, arg, self.stream)
        else:
            assert kernel == "nt128" and pre == 0
            st = self.lib.afxk_gemm_nt128_bf16(a.ptr, lda, b.ptr, ldb, c.ptr, ldc, M, N, K, post, arg, self.stream)
        return self._result(st, c, M, ldc)

    def bank_prepare(self, B, ldb):
        b, img = Buffer(self.backend, _pitched(B, ldb)), _VP()
        st = self.lib.afxk_gemm_bank_prepare(b.ptr, ldb, B.shape[0], B.shape[1], C.byref(img), self.stream)
        assert st == 0 and img.value, f"afxk_gemm_bank_prepare: status {st}"
        self.sync()  # (b is released when this returns)
        return img

    def bank_product(self, img, A, N, lda, ldc, post=0, arg=0.0, a_shift=0):
        M, K = A.shape
        a, c = Buffer(self.backend, _pitched(A, lda), a_shift), self._c(M, ldc)
        st = self.lib.afxk_gemm_nt_bank(a.ptr, lda, img, N, K, c.ptr, ldc, M, post, arg, self.stream)
        return self._result(st, c, M, ldc)


def split_result(words, N):
    """C [M, ldc] words -> (the [M, N] float32 results, True when every other word still holds the sentinel)"""
    return words[:, :N].view(np.float32), bool(np.all(words[:, N:] == gc.SENTINEL))


def run_case(lib, backend, stream, sync, case):
    """one row of gemm_cases.table(); returns (worst error, bar)"""
    c = case
    what = gc.case_id(c)
    A, B = gc.operands(c.kind, c.M, c.N, c.K)
    st, words = Runner(lib, backend, stream, sync).product(c.kernel, A, B, c.lda, c.ldb, c.ldc, c.pre, c.post, c.arg)
    assert st == 0, f"{what}: status {st}"
    got, clean = split_result(words, c.N)
    assert clean, f"{what}: a word outside the [M, N] results was written"
    if HOSTSTUB:
        return 0.0, 0.0
    ref = gc.reference_of(c)
    assert not np.any(got.view(np.uint32) == gc.SENTINEL), f"{what}: a promised element was not written"
    assert np.all(np.isfinite(got)), f"{what}: non-finite results (padding read?)"
    e = gc.error(got, ref.want, ref.den)
    worst = float(e.max())
    print(f"{what}: elementwise error max {worst:.2e} mean {float(e.mean()):.2e}, float32 chain {ref.e32:.2e}, bar {ref.bar:.2e}", flush=True)
    parity_log(what, worst, ref.bar, "gemm: elementwise |got - want64| / denominator, bar max(4e-7, 2 x float32 chain)",
               {"kernel": c.kernel, "operands": c.kind, "e32": ref.e32})
    i, j = np.unravel_index(int(np.argmax(e)), e.shape)
    assert worst <= ref.bar, f"{what}: error {worst:.3e} > {ref.bar:.3e} at [{i}, {j}]: got {got[i, j]!r}, want {ref.want[i, j]!r}"
    return worst, ref.bar


def check_refusals(lib, backend, stream, sync):
    """the documented refusals return AFX_ERR_UNSUPPORTED and write nothing: a pitch of A that is no multiple of 4 floats, an A off
    a 16-byte boundary (both bf16 entry points), and for the bank form a pitch under K rounded up to 4"""
    r = Runner(lib, backend, stream, sync)
    A, B = gc.operands("flat", 130, 40, 17)
    for kernel, lda, shift, why in (("nt128", 21, 0, "lda % 4"), ("nt128", 24, 1, "misaligned A"), ("bank", 21, 0, "lda % 4"),
                                    ("bank", 24, 1, "misaligned A"), ("bank", 16, 0, "lda < K rounded up to 4")):
        if lda < A.shape[1]:  # (a pitch under K: rows overlap -- the refusal comes before any access; hand it a buffer that holds them)
            img = r.bank_prepare(B, 28)
            a, c = Buffer(backend, np.zeros(130 * 20, np.float32)), r._c(130, 43)
            st = r.lib.afxk_gemm_nt_bank(a.ptr, lda, img, 40, 17, c.ptr, 43, 130, 0, 0.0, stream)
            r.sync()
            words = c.read()
            r.lib.afxdev_free(img)
        else:
            st, words = r.product(kernel, A, B, lda, 28, 43, a_shift=shift)
        if HOSTSTUB:
            continue
        assert st == gc.ERR_UNSUPPORTED, f"{kernel}, {why}: status {st}"
        assert np.all(words == gc.SENTINEL), f"{kernel}, {why}: the refused call wrote"
