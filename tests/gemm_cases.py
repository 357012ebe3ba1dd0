"""The matrix-product kernels element by element: cases, operands and references (numpy only) of tests/test_gemm_cpu.py,
tests/test_gemm_gpu.py and tests/emu/emulated_gemm.py.

Three kernels compute C[M, N] = post(pre(A)[M, K] . B[N, K]^T):
  f32    k_gemm_nt (afx_gemm.hip), float32 MFMA, 64 x 64 tiles, K in steps of 32, the LOG10 / CBRT pre-maps -- through afxk_gemm_nt
         with an odd row pitch of A, which the bf16 launcher declines
  nt128  k_gemm_nt128_bf16x3 (afx_gemm_bf16.hip): three bf16 words per float32 value, six MFMA terms, 128 x 128 tiles, K in steps of 16,
         double-buffered -- through afxk_gemm_nt128_bf16
  bank   k_bank_split + k_gemm_bank_bf16x3: the same expansion with the bank prepared once, loads waited for by count, a two-stage
         register ring (a stage = two k-steps) -- through afxk_gemm_bank_prepare + afxk_gemm_nt_bank

The object-level tests judge these at 1e-5 of a tensor's peak on noise; a missing low-word term of the expansion is 3e-6 ... 7e-6 of
ONE element and invisible there.  Here every element is compared with the float64 product and the bar comes from the float32
chain on the same operands: max(4e-7, 2 x E32), E32 = the worst error of `chain32` under the case's metric.  4e-7 is 3.4 float32
ulp; the factor 2 covers fma against mul + add rounding and the library's log10f / powf against numpy's.  No bar is taken from
what a kernel returns."""
import functools
import zlib
from collections import namedtuple

import numpy as np

MAP_NONE, MAP_LOG10, MAP_CBRT, MAP_POW = 0, 1, 2, 3
ERR_UNSUPPORTED = -4
FLOOR, FACTOR = 4e-7, 2.0
FLT_MAX = float(np.finfo(np.float32).max)
SENTINEL = np.uint32(0xC0FFEE01)  # a finite float32 no product here returns

# the six terms of the expansion as (word of a, word of b), 0 = hi, 1 = mid, 2 = lo, in the kernels' order: smallest first
TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
# what the bars must see (tests/test_gemm_cpu.py): one small term missing, or a_l meeting the wrong word of b
MUTANTS = {"a_l.b_h dropped": tuple(t for t in TERMS if t != (2, 0)),
           "a_h.b_l dropped": tuple(t for t in TERMS if t != (0, 2)),
           "a_m.b_m dropped": tuple(t for t in TERMS if t != (1, 1)),
           "a_l.b_l for a_l.b_h": tuple((2, 2) if t == (2, 0) else t for t in TERMS)}

Case = namedtuple("Case", "kernel kind M N K lda ldb ldc pre post arg")

K_BF16 = (1, 3, 4, 13, 16, 17, 31, 32, 33, 48, 49, 64, 77, 80, 96, 111, 113, 129)  # 1 ... 9 k-steps of 16, 1 ... 5 stages, every K mod 4
K_F32 = (1, 31, 32, 33, 40, 128, 129)                                # 1 ... 5 steps of 32 with and without a tail
M_ALL = (1, 127, 128, 129, 300)
N_OF = {"bank": (1, 12, 40, 128, 129, 130, 257), "nt128": (33, 128, 130, 257), "f32": (1, 13, 32, 33, 64, 65)}
KINDS_BF16 = ("flat", "signed", "bank", "big", "small")
KINDS_F32 = (("flat", MAP_NONE), ("signed", MAP_NONE), ("logmel", MAP_LOG10), ("bank", MAP_NONE), ("big", MAP_NONE), ("small", MAP_NONE),
             ("logmel", MAP_CBRT))


def _up4(k):
    return (k + 3) & ~3


def make_case(kernel, kind, M, N, K, pre=MAP_NONE, post=MAP_NONE, arg=0.0, tight=False):
    """pitches larger than the extents (the padding of A and B is NaN, C holds a sentinel).  bf16 kernels: multiples of 4 floats;
    `tight`: lda = K rounded up to 4, the documented minimum of the bank form.  f32: odd pitches, so that the bf16 launcher
    declines whatever N is"""
    if kernel == "f32":
        lda, ldb, ldc = K + 1 + K % 2, K + 3, N + 5
    else:
        lda, ldb, ldc = (_up4(K) if tight else _up4(K) + 4), _up4(K) + 8, N + 3
    return Case(kernel, kind, M, N, K, lda, ldb, ldc, pre, post, float(np.float32(arg)))


def structure(c):
    """what the shape reaches, for the case id"""
    if c.kernel == "f32":
        s = f"{-(-c.K // 32)}steps32_tail{c.K % 32}_{-(-c.N // 64)}coltiles_{-(-c.M // 64)}rowtiles"
    else:
        nk = -(-c.K // 16)
        s = f"{nk}ksteps_{(nk + 1) // 2}stages_Kmod4is{c.K % 4}_{-(-c.N // 128)}coltiles_{-(-c.M // 128)}rowtiles"
        if c.lda == _up4(c.K):
            s += "_minpitch"
    return s


def case_id(c):
    maps = {MAP_NONE: "", MAP_LOG10: "-log10", MAP_CBRT: "-cbrt"}[c.pre] + ("-pow%g" % c.arg if c.post == MAP_POW else "")
    return f"{c.kernel}-{c.kind}{maps}-M{c.M}-N{c.N}-K{c.K}-{structure(c)}"


@functools.lru_cache(maxsize=None)
def table():
    """about 60 launches per bf16 kernel, 45 for the float32 one, each a few tiles: every K at (M, N) = (130, 40) and (300, 130), every M and every N at K = 77
    and K = 17, K = 1025 once with the power-law epilogue"""
    cases = []
    for kern in ("bank", "nt128"):
        for K in K_BF16:
            cases.append(make_case(kern, "decades", 130, 40, K))
        for i, K in enumerate(K_BF16):
            cases.append(make_case(kern, KINDS_BF16[i % len(KINDS_BF16)], 300, 130, K, tight=i % 2 == 1))
        for K in (77, 17):
            for i, M in enumerate(M_ALL):
                cases.append(make_case(kern, ("decades", "signed")[i % 2], M, 130, K, tight=i % 2 == 0))
            for i, N in enumerate(N_OF[kern]):
                cases.append(make_case(kern, ("decades", "bank", "flat")[i % 3], 130, N, K, tight=i % 2 == 1))
        cases.append(make_case(kern, "decades", 130, 40, 1025, post=MAP_POW, arg=0.5))
    pre3 = (("decades", MAP_NONE), ("logmel", MAP_LOG10), ("logmel", MAP_CBRT))
    for i, K in enumerate(K_F32):
        for kind, pre in (pre3[i % 3], pre3[(i + 1) % 3]):  # (N = 40 > 32 without a pre-map: only the odd pitch keeps it here)
            cases.append(make_case("f32", kind, 130, 40, K, pre=pre))
    for i, K in enumerate(K_F32):
        kind, pre = KINDS_F32[i % len(KINDS_F32)]
        cases.append(make_case("f32", kind, 300, 130, K, pre=pre))
    for K in (77, 17):
        for i, M in enumerate(M_ALL):
            kind, pre = pre3[i % 3]
            cases.append(make_case("f32", kind, M, 33, K, pre=pre))
        for i, N in enumerate(N_OF["f32"]):
            kind, pre = pre3[(i + 1) % 3]
            cases.append(make_case("f32", kind, 130, N, K, pre=pre))
    cases.append(make_case("f32", "decades", 130, 40, 1025, post=MAP_POW, arg=0.5))
    ids = [case_id(c) for c in cases]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    return tuple(cases)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _decades(rng, M, K):
    return rng.standard_normal((M, K)) ** 2 * 10.0 ** rng.uniform(-5, 5, (M, K))


@functools.lru_cache(maxsize=None)
def operands(kind, M, N, K):
    """A [M, K], B [N, K] float32, read-only, the same for every kernel that runs the shape"""
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{M}/{N}/{K}".encode()))
    B = np.abs(rng.standard_normal((N, K))) + 0.05
    if kind == "decades":      # one product dominates a sum: every element tests the split of a single pair
        A = _decades(rng, M, K)
    elif kind == "flat":       # the accumulation over K
        A, B = rng.uniform(0.5, 2.0, (M, K)), rng.uniform(0.5, 2.0, (N, K))
    elif kind == "signed":     # the re / im planes of the complex route
        A = _decades(rng, M, K) * rng.choice([-1.0, 1.0], (M, K))
    elif kind == "bank":       # a filter bank: 30 % exact zeros
        A = _decades(rng, M, K)
        B = np.abs(rng.standard_normal((N, K))) * (rng.uniform(0, 1, (N, K)) < 0.7)
    elif kind == "big":        # float32's exponent range, upper end
        A = _decades(rng, M, K) * 1e25
    elif kind == "small":      # ... lower end; 1e-30 keeps all three words of a value normal bf16 numbers (the lowest bit of a value
        A = np.maximum(_decades(rng, M, K) * 1e-25, 1e-30)  # is 2^-23 of it; subnormal low words are out of scope)
    elif kind == "logmel":     # the cepstral transform: positive spectra with entries under the 1e-8 clamp, DCT-like rows of both signs
        A = _decades(rng, M, K) * 1e-3
        A[rng.uniform(0, 1, (M, K)) < 0.1] *= 1e-9
        B = rng.standard_normal((N, K))
    else:
        raise ValueError(kind)
    A, B = A.astype(np.float32), B.astype(np.float32)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


# ---- references -------------------------------------------------------------------------------------------------------------
def pre64(A, pre):
    """the pre-map in float64 on the float32 inputs; the LOG10 clamp is float32's 1e-8"""
    A = np.asarray(A, np.float64)
    if pre == MAP_LOG10:
        return np.log10(np.maximum(A, float(np.float32(1e-8))))
    if pre == MAP_CBRT:
        return A ** float(np.float32(1.0 / 3))
    return A


def want64(A, B, pre=MAP_NONE, post=MAP_NONE, arg=0.0):
    w = pre64(A, pre) @ np.asarray(B, np.float64).T
    return w ** float(np.float32(arg)) if post == MAP_POW else w


def pre32(A, pre):
    A = np.asarray(A, np.float32)
    if pre == MAP_LOG10:
        return np.log10(np.maximum(A, np.float32(1e-8)))
    if pre == MAP_CBRT:
        return np.power(A, np.float32(1.0 / 3))
    return A


def _post32(acc, post, arg):
    return np.power(acc, np.float32(arg)) if post == MAP_POW else acc


def chain32(A, B, pre=MAP_NONE, post=MAP_NONE, arg=0.0):
    """the float32 product accumulated one k at a time in k order (an fma chain: what the f32 MFMA computes), maps in float32"""
    P, B = pre32(A, pre).astype(np.float64), np.asarray(B, np.float64)
    acc = np.zeros((P.shape[0], B.shape[0]), np.float32)
    for k in range(P.shape[1]):
        acc = (acc.astype(np.float64) + P[:, k:k + 1] * B[None, :, k]).astype(np.float32)
    return _post32(acc, post, arg)


def split3(x):
    """float32 -> the three bf16 words (as float32 values) of k_bank_split / k_gemm_bank_bf16x3: hi and mid rounded half up in
    magnitude on the bit pattern, lo what is left; finite operands below 0x7f7f8000"""
    x = np.ascontiguousarray(x, np.float32)
    words, r = [], x
    for _ in range(2):
        w = ((r.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(np.float32)
        words.append(w)
        r = r - w  # exact
    words.append((r.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32))
    assert np.array_equal(words[2], r) and np.array_equal(words[0].astype(np.float64) + words[1] + words[2], x.astype(np.float64))
    return words


def six(A, B, terms=TERMS, post=MAP_NONE, arg=0.0):
    """the numpy model of the bf16x3 expansion: per 16-wide k-step and per (a word, b word) term in the order given, the
    sixteen products summed exactly and added to the float32 accumulator with one rounding"""
    Aw = [w.astype(np.float64) for w in split3(A)]
    Bw = [w.astype(np.float64) for w in split3(B)]
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k0 in range(0, A.shape[1], 16):
        for wa, wb in terms:
            acc = (acc.astype(np.float64) + Aw[wa][:, k0:k0 + 16] @ Bw[wb][:, k0:k0 + 16].T).astype(np.float32)
    return _post32(acc, post, arg)


# ---- metric and bar ---------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "want den e32 bar")


def error(got, want, den):
    """|got - want| / den element by element; where den is 0 (an all-zero sum of a bank with exact zeros) the result must be 0"""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den > 0, d / den, np.where(d == 0, 0.0, np.inf))
    return e


@functools.lru_cache(maxsize=None)
def reference(kind, M, N, K, pre, post, arg):
    """want64, the metric's denominator, E32 and the bar of a shape: computed once, shared by the kernels and tests, read-only.
    Denominator: |want64| for non-negative operands without a pre-map and for POW (after the map); sum |pre(A)| |B| for
    `signed` operands and pre-maps (sums with cancellation)"""
    A, B = operands(kind, M, N, K)
    want = want64(A, B, pre, post, arg)
    if kind == "signed" or pre != MAP_NONE:
        assert post == MAP_NONE
        den = np.abs(pre64(A, pre)) @ np.abs(B.astype(np.float64)).T
    else:
        den = np.abs(want)
    e32 = float(error(chain32(A, B, pre, post, arg), want, den).max())
    for a in (want, den):
        a.setflags(write=False)
    return Ref(want, den, e32, max(FLOOR, FACTOR * e32))


def reference_of(c):
    return reference(c.kind, c.M, c.N, c.K, c.pre, c.post, c.arg)


# ---- the operands of the non-finite tests (tests/test_gemm_gpu.py; checked on the CPU in tests/test_gemm_cpu.py) ----------------
SPECIAL_ROWS = {3: np.float32(np.inf), 70: np.float32(FLT_MAX), 129: np.float32(np.nan)}


def special_operands(K):
    """a `decades` case M = N = 130 with B strictly positive; (A with +Inf in row 3, FLT_MAX in row 70, NaN in row 129, each at
    one k; the same A with 1.0 in those three places; B; the k)"""
    A, B = operands("decades", 130, 130, K)
    k = K // 2
    plain = A.copy()
    special = A.copy()
    for row, v in SPECIAL_ROWS.items():
        plain[row, k] = 1.0
        special[row, k] = v
    return special, plain, B, k


def row70_mask(want_row):
    """the elements of row 70 that are judged: not within 1e-6 of FLT_MAX (where float32(want64) is decided by the last bit)"""
    return np.abs(want_row / FLT_MAX - 1.0) > 1e-6
