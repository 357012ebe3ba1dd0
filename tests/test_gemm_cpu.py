"""The bars of tests/gemm_cases.py can see what they are for -- shown on the numpy model of the bf16x3 expansion (`six`), no kernel
involved.  For every (operand kind, K <= 129) of the bf16 kernels' table the full six-term model is inside the bar
max(4e-7, 2 x E32); on the `decades` kind each single missing small term (a_l b_h, a_h b_l, a_m b_m), and a_l b_l in place of
a_l b_h, is more than 3 x the bar away at every K <= 77.

At K = 1025 a missing term is about 3.5e-6 and UNDER that shape's bar (the float32 chain itself is 2.5e-6 off there): the
small-K rows of the table are what carry the sensitivity to a single term; K = 1025 is there for the ring and the accumulation.

The operands of the non-finite device tests are checked here too: what float64 says about the row with FLT_MAX."""
import numpy as np
import pytest

from tests import gemm_cases as gc

BF16_SHAPES = sorted({(c.kind, c.M, c.N, c.K) for c in gc.table() if c.kernel != "f32" and c.K <= 129})
# the sensitivity condition is one per (kind, K): on the largest shape the table has for the pair (the worst of 130 elements of an
# M = 1 case says little about a term; that case is there for its clamped rows)
LARGEST = {}
for _s in BF16_SHAPES:
    if _s[1] * _s[2] > LARGEST.get((_s[0], _s[3]), (0, 0, 1, 0))[1] * LARGEST.get((_s[0], _s[3]), (0, 0, 1, 0))[2]:
        LARGEST[(_s[0], _s[3])] = _s


def test_the_table_reaches_what_it_names():
    t = gc.table()
    for kern, ks in (("bank", gc.K_BF16), ("nt128", gc.K_BF16), ("f32", gc.K_F32)):
        mine = [c for c in t if c.kernel == kern]
        assert 35 <= len(mine) <= 70, (kern, len(mine))
        for mn in ((130, 40), (300, 130)):
            assert {c.K for c in mine if (c.M, c.N) == mn} >= set(ks), (kern, mn)
        for K in (77, 17):
            assert {c.M for c in mine if c.K == K} >= set(gc.M_ALL) and {c.N for c in mine if c.K == K} >= set(gc.N_OF[kern]), (kern, K)
        assert [c for c in mine if c.K == 1025 and c.post == gc.MAP_POW and c.arg == 0.5]
        assert all(c.lda >= c.K and c.ldb > c.K and c.ldc > c.N for c in mine) and any(c.lda > c.K for c in mine)
    bank = [c for c in t if c.kernel == "bank"]
    assert {c.K % 4 for c in bank if c.lda == ((c.K + 3) & ~3)} >= {0, 1}, "the minimum pitch with and without a NaN inside the last quad"
    assert {-(-c.K // 16) for c in bank} >= set(range(1, 10)) | {65}
    f32 = [c for c in t if c.kernel == "f32"]
    assert all(c.lda % 2 == 1 for c in f32), "an odd pitch keeps every f32 case away from the bf16 launcher"
    assert [c for c in f32 if c.N > 32 and c.pre != gc.MAP_NONE] and [c for c in f32 if c.N > 32 and c.pre == gc.MAP_NONE]
    kinds = {c.kind for c in t}
    assert kinds == {"decades", "flat", "signed", "bank", "big", "small", "logmel"}, kinds


def test_the_operands_keep_every_word_a_normal_number():
    for kind in ("big", "small"):
        A, B = gc.operands(kind, 300, 130, 77)
        for X in (A, B):
            for w in gc.split3(X):
                nz = np.abs(w[w != 0]).astype(np.float64)
                assert nz.min() >= 2.0 ** -126 and nz.max() < 2.0 ** 127, kind
    A, _ = gc.operands("logmel", 130, 40, 40)
    assert (A > 0).all() and (A < 1e-8).mean() > 0.05


@pytest.mark.parametrize("shape", BF16_SHAPES, ids=lambda s: "%s-M%d-N%d-K%d" % s)
def test_the_bar_passes_the_expansion_and_sees_a_single_term(shape):
    kind, M, N, K = shape
    A, B = gc.operands(kind, M, N, K)
    ref = gc.reference(kind, M, N, K, gc.MAP_NONE, gc.MAP_NONE, 0.0)
    full = float(gc.error(gc.six(A, B), ref.want, ref.den).max())
    print(f"{kind} M {M} N {N} K {K}: six terms {full:.2e}, float32 chain {ref.e32:.2e}, bar {ref.bar:.2e}")
    assert full <= ref.bar, (full, ref.bar)
    if kind == "decades" and K <= 77 and LARGEST[(kind, K)] == shape:
        for name, terms in gc.MUTANTS.items():
            e = float(gc.error(gc.six(A, B, terms), ref.want, ref.den).max())
            print(f"    {name}: {e:.2e} = {e / ref.bar:.1f} x the bar")
            assert e > 3 * ref.bar, (name, e, ref.bar)


def test_the_expansion_passes_at_the_dense_shape_with_the_power_law():
    c = [c for c in gc.table() if c.kernel == "bank" and c.K == 1025][0]
    A, B = gc.operands(c.kind, c.M, c.N, c.K)
    ref = gc.reference_of(c)
    full = float(gc.error(gc.six(A, B, post=c.post, arg=c.arg), ref.want, ref.den).max())
    assert full <= ref.bar, (full, ref.bar)


@pytest.mark.parametrize("K", [17, 77])
def test_the_non_finite_operands(K):
    """row 70 (FLT_MAX at one k): float64 is clear of FLT_MAX in every column but under 1 % of them, and the row has both elements
    that overflow float32 and elements that do not; the other special rows hold what they should"""
    special, plain, B, k = gc.special_operands(K)
    assert (B > 0).all() and np.isposinf(special[3, k]) and np.isnan(special[129, k]) and special[70, k] == np.float32(gc.FLT_MAX)
    assert np.isfinite(plain).all() and (plain != special).sum() == 2 + 1  # (NaN != NaN)
    want = special[70].astype(np.float64) @ B.astype(np.float64).T
    judged = gc.row70_mask(want)
    assert judged.mean() > 0.99
    assert (want[judged] > gc.FLT_MAX).sum() >= 10 and (want[judged] < gc.FLT_MAX).sum() >= 10
    # the split of FLT_MAX itself: the truncated hi word, exact remainders
    x = np.array([gc.FLT_MAX], np.float32)
    hi = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    assert np.isfinite(hi).all() and ((x.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
