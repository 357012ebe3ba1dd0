"""The three matrix-product kernels on the device, element by element against float64: the table of tests/gemm_cases.py (shapes
named by the structure they reach: k-steps, stages of the register ring, K mod 4, column and row tiles, the minimum pitch;
operands over ten decades, flat, signed, with exact zeros, at both ends of float32's exponent range, under the pre-maps)
through tests/gemm_check.py, bar max(4e-7, 2 x the float32 chain's own error) -- tests/test_gemm_cpu.py shows that this bar
sees a single missing term of the bf16x3 expansion at the small K of the table.  Then what the table cannot show: rows do not
leak into each other, Inf / NaN / FLT_MAX in A come out as the IEEE product, and a bank image serves any number of products."""
import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import gemm_check as chk
from tests.conftest import EMULATED, HOSTSTUB

pytestmark = pytest.mark.gpu

ENTRIES = ("bank", "nt128", "f32")


def _backend():
    """(backend, stream, sync): device memory through torch; host memory where the library's device layer is a host stand-in"""
    if HOSTSTUB or EMULATED:
        return "numpy", None, None
    import torch
    return "torch", torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize


def _lib():
    from audioflux_amd import _lib
    return _lib.get_lib()


def _runner():
    return chk.Runner(_lib(), *_backend())


def _pitches(kernel, K):
    """(lda, ldb, ldc) for M = N = 130: the float kernel is reached through an odd pitch"""
    return (K + 1 + K % 2, K + 3, 135) if kernel == "f32" else (((K + 3) & ~3) + 4, ((K + 3) & ~3) + 8, 133)


@pytest.mark.parametrize("case", gc.table(), ids=gc.case_id)
def test_product_against_float64(case):
    chk.run_case(_lib(), *_backend(), case)


def test_documented_refusals_write_nothing():
    chk.check_refusals(_lib(), *_backend())


@pytest.fixture(scope="module", params=[17, 77])
def special(request):
    """per K: (A with Inf / FLT_MAX / NaN, A with 1.0 in their places, B, {entry: (C special, C plain)})"""
    K = request.param
    a_special, a_plain, B, _ = gc.special_operands(K)
    r, out = _runner(), {}
    for kernel in ENTRIES:
        lda, ldb, ldc = _pitches(kernel, K)
        res = []
        for A in (a_special, a_plain):
            st, words = r.product(kernel, A, B, lda, ldb, ldc)
            assert st == 0, (kernel, st)
            got, clean = chk.split_result(words, 130)
            assert clean, kernel
            res.append(got)
        out[kernel] = res
    return K, a_special, B, out


@pytest.mark.parametrize("kernel", ENTRIES)
def test_rows_are_independent(special, kernel):
    """+Inf in row 3, FLT_MAX in row 70, NaN in row 129, each at one k: every other row is bit-equal to the same call with 1.0
    in those three places"""
    K, _, _, out = special
    got, plain = out[kernel]
    if HOSTSTUB:
        return
    others = np.setdiff1d(np.arange(130), list(gc.SPECIAL_ROWS))
    diff = got[others].view(np.uint32) != plain[others].view(np.uint32)
    assert not diff.any(), f"{kernel}, K {K}: {int(diff.sum())} elements of rows {sorted(set(others[np.nonzero(diff)[0]]))[:8]} changed"
    assert np.isfinite(plain).all()


@pytest.mark.parametrize("kernel", ENTRIES)
def test_non_finite_and_huge_values(special, kernel):
    """B strictly positive: the row with +Inf is +Inf everywhere, the row with NaN is NaN everywhere, the row with FLT_MAX equals
    float32(want64): +Inf where the float64 product exceeds FLT_MAX, within 1e-6 of it elsewhere (elements within 1e-6 of
    FLT_MAX are left out: under 1 % of the row, tests/test_gemm_cpu.py).  The float kernel, reached through an odd pitch,
    gives the same answer: what the two bf16 kernels are compared with"""
    K, a_special, B, out = special
    got = out[kernel][0]
    if HOSTSTUB:
        return
    assert np.isposinf(got[3]).all(), f"{kernel}, K {K}: row 3 (+Inf at one k) holds {got[3][~np.isposinf(got[3])][:4]}"
    assert np.isnan(got[129]).all(), f"{kernel}, K {K}: row 129 (NaN at one k) holds {got[129][~np.isnan(got[129])][:4]}"
    want = a_special[70].astype(np.float64) @ B.astype(np.float64).T
    judged = gc.row70_mask(want)
    assert judged.mean() > 0.99
    over = want > gc.FLT_MAX
    row = got[70].astype(np.float64)
    assert np.isposinf(row[judged & over]).all(), f"{kernel}, K {K}: row 70 is finite where float64 exceeds FLT_MAX"
    fin = judged & ~over
    assert np.isfinite(row[fin]).all(), f"{kernel}, K {K}: row 70 is not finite where float64 is under FLT_MAX: {row[fin][~np.isfinite(row[fin])][:4]}"
    rel = np.abs(row[fin] - want[fin]) / want[fin]
    assert rel.max() <= 1e-6, f"{kernel}, K {K}: row 70 is {rel.max():.2e} off float64"
    f32 = out["f32"][0]
    same = np.isposinf(f32[70]) == np.isposinf(got[70])
    assert same[judged].all(), f"{kernel}, K {K}: row 70 overflows in other columns than the float kernel's"


def test_bank_image_reuse():
    """one image, two different A with a larger unrelated launch in between: both results bit-equal to those of fresh images"""
    r = _runner()
    A1, B = gc.operands("decades", 130, 130, 77)
    A2, _ = gc.operands("signed", 129, 130, 77)
    A3, B3 = gc.operands("flat", 300, 130, 129)
    fresh = [r.product("bank", A, B, 84, 88, 133)[1] for A in (A1, A2)]
    img = r.bank_prepare(B, 88)
    try:
        st1, c1 = r.bank_product(img, A1, 130, 84, 133)
        st3, _ = r.product("bank", A3, B3, 136, 140, 257)
        st2, c2 = r.bank_product(img, A2, 130, 84, 133)
        st1b, c1b = r.bank_product(img, A1, 130, 84, 133)
    finally:
        r.lib.afxdev_free(img)
    assert (st1, st2, st3, st1b) == (0, 0, 0, 0)
    if HOSTSTUB:
        return
    assert np.array_equal(c1, fresh[0]) and np.array_equal(c2, fresh[1]) and np.array_equal(c1b, fresh[0])
