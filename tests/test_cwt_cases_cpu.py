"""CPU-only: the table of tests/cwt_cases.py reaches what its rows are named for (the host plan from the bank alone), and the
bars of tests/cwt_check.py see the defects a CWT kernel can have -- each applied in float64 to the reference result of the rows
designed for it, and required to exceed 3 x the row's bar on at least one scale."""
import numpy as np
import pytest

from tests import cwt_cases as cc
from tests import cwt_check as ck

ROWS = cc.table()
FAST = [r.name for r in ROWS if r.path == "fast"]
FLAT = [r.name for r in ROWS if r.custom and r.custom[0] == "flat"]
BITE = 3.0


# ---- reach ----------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_path_size_family_and_input():
    by_path = {p: [r for r in ROWS if r.path == p] for p in ("small", "generic", "fast")}
    assert {cc.fft_length(r) for r in by_path["small"]} == {1 << 4, 1 << 8, 1 << 14}
    assert {(r.r, r.pad) for r in by_path["small"]} == {(3, True), (8, False), (13, True), (14, False)}
    assert {r.wavelet for r in by_path["small"]} == set(cc.FAMILIES)
    assert {cc.fft_length(r) for r in by_path["generic"]} == {1 << 15, 1 << 16, 1 << 18}
    assert {(r.r, r.pad) for r in by_path["generic"]} >= {(14, True), (15, True), (16, False), (18, False)}
    assert len({r.wavelet for r in by_path["generic"]}) >= 4 and any(r.det for r in by_path["generic"])
    assert all(cc.fft_length(r) == cc.L17 for r in by_path["fast"])
    for pad in (True, False):  # both paddings at L = 2^17, all eight families
        assert {r.wavelet for r in by_path["fast"] if r.pad == pad and r.wavelet} == set(cc.FAMILIES)
    assert {r.wavelet for r in by_path["fast"] if r.det and r.wavelet} >= {"morlet", "morse", "dog"}
    assert any(r.td_det == ("1", "0") and r.det and r.counts[0] > 0 for r in ROWS)
    assert any(r.shift and r.path == "fast" for r in ROWS)
    nofused = [r for r in ROWS if r.nofused]
    assert {r.name for r in by_path["small"]} <= {r.name for r in nofused} and any((r.r, r.pad) == (16, True) for r in nofused)
    kinds = {s[0] for r in ROWS for s in r.x}
    assert kinds == {"noise", "level_step", "dc_offset"}


@pytest.mark.parametrize("name", FAST)
def test_fast_path_row_reaches_its_classes(name):
    """bank -> afx_cwt_support_host -> afx_cwt_classify_host (+ the restated time-domain rule) = the counts in the table, which the
    device test asserts on the object itself (afx_cwt_plan_counts)"""
    row, plan = cc.by_name(name), cc.host_plan(name)
    assert plan.counts == row.counts, (plan.counts, row.counts, plan.width)
    assert plan.det_images == row.det_images
    assert sum(plan.counts) == row.num
    if row.wavelet:  # one row of a family holds two-pass, narrow-band and (Morlet) time-domain scales at once
        assert plan.counts[2] > 0 and sum(plan.counts[3:]) > 0
        assert (plan.counts[0] > 0) == (row.wavelet == "morlet")


def test_every_narrow_class_by_a_family_and_by_a_flat_band():
    for cls, R in enumerate(cc.CLASS_ROWS):
        fam = [r.name for r in ROWS if r.path == "fast" and r.wavelet and r.counts[3 + cls] > 0]
        flat = [n for n in FLAT if cc.by_name(n).counts[3 + cls] > 0]
        assert fam and flat, (R, fam, flat)


def test_flat_bands_hold_every_width_and_position():
    seen = set()
    for n in FLAT:
        row = cc.by_name(n)
        b = cc.bank(n).reshape(row.num, 512, 256)
        for j, (lo, w) in enumerate(row.custom[1]):
            rows = np.nonzero(b[j].any(axis=1))[0]
            assert rows.min() == lo and rows.max() == lo + w - 1 and np.all(b[j][lo:lo + w] == 1.0) and b[j].sum() == 256 * w
            seen.add((w, "row0" if lo == 0 else "row1" if lo == 1 else "nyquist" if lo + w == 256 else "clamp" if lo + w == 512 else "mid"))
    for w in cc.FLAT_WIDTHS:
        assert {(w, p) for p in ("row0", "row1", "mid", "nyquist")} <= seen
    clamp = sorted(w for w, p in seen if p == "clamp")
    assert len(clamp) == 7
    for w, R, below in zip(clamp, cc.CLASS_ROWS, (0,) + cc.CLASS_ROWS):  # one per class, whose R rows from 512 - w would leave the spectrum
        assert below < w < R


def test_time_domain_rows_reach_both_tap_classes_the_unpaired_scale_and_the_fallback():
    one = cc.host_plan("fast_gauss_td_one_unpaired_short")
    assert one.counts[0] == 1 and cc.taps_of(one.kh[0]) == cc.TD_SHORTK  # a single scale: one pair with an empty half
    three = cc.host_plan("fast_gauss_td_pair_and_unpaired_both_classes_and_overlength")
    row = cc.by_name("fast_gauss_td_pair_and_unpaired_both_classes_and_overlength")
    kh = dict(zip([s[1] for s in row.custom[1] if s[0] == "gauss"], cc.td_half_lengths(cc.bank(row.name), [0, 1, 2, 4], 1 << 16, 1 << 15)))
    assert kh == cc.TD_KH
    assert three.counts[0] == 3 and three.counts[2] == 1  # (the over-length kernel: two passes on the FFT path)
    longest_first = sorted(three.kh, reverse=True)
    pairs = [longest_first[0:2], longest_first[2:]]
    assert cc.taps_of(pairs[0][0]) > cc.TD_SHORTK and len(pairs[1]) == 1 and cc.taps_of(pairs[1][0]) == cc.TD_SHORTK
    assert cc.taps_of(184) == 384 and cc.taps_of(186) == 416          # either side of the class split
    # ... and 416 taps is an image the device builds: a pair whose LONGER kernel has half length 186, in the long class
    pair = cc.host_plan("fast_gauss_td_pair_416_taps_first_of_the_long_class")
    assert pair.counts[0] == 2 and sorted(pair.kh, reverse=True) == [186, 184] and sorted(pair.kh_det, reverse=True) == [186, 184]
    assert cc.taps_of(max(pair.kh)) == 416 > cc.TD_SHORTK and cc.taps_of(max(pair.kh_det)) == 416
    # (in the five-scale row the 186 kernel rides in the 480 kernel's image: 992 taps)
    assert cc.taps_of(pairs[0][0]) == 992 and pairs[0][1] == 186
    assert one.det_images == 1 and one.kh_det == (184,) and cc.by_name("fast_gauss_td_one_unpaired_short").det
    assert 2 * 480 + 8 <= cc.TD_MAXK - 56 < 2 * 483 + 8               # either side of the limit
    morlet = cc.host_plan("fast_r16_pad_morlet")
    assert any(cc.taps_of(h) <= cc.TD_SHORTK for h in morlet.kh) and any(cc.taps_of(h) > cc.TD_SHORTK for h in morlet.kh)
    assert morlet.det_images == 1 and morlet.kh_det != morlet.kh     # the derivative bank's kernels are its own


@pytest.mark.parametrize("name", [r.name for r in ROWS if r.custom])
def test_custom_banks_are_valid(name):
    row, b = cc.by_name(name), cc.bank(name)
    assert b.shape == (row.num, cc.fft_length(row)) == (row.num, cc.L17) and b.dtype == np.float32 and b.flags.c_contiguous
    assert np.all(np.isfinite(b)) and np.all(b.any(axis=1)), "finite, and no all-zero row"


def test_every_reference_row_has_a_peak():
    for r in ROWS:
        assert np.all(cc.bank(r.name).any(axis=1)), r.name


# ---- the bars bite --------------------------------------------------------------------------------------------------------------
def _noise_chunk(row):
    return next(c for c, s in enumerate(row.x) if s[0] == "noise")


def _bitten(row, det, bad, c):
    """worst e_j / bar_j of a defective float64 result [num][D] against the reference result of chunk c"""
    ref = ck.reference(row.name, det)
    return float((ck.per_scale(bad, ref.f64[c]) / ref.bar[c]).max())


def _uncropped(row, c, det=False, bank=None, circular=False):
    x = cc.inputs(row)[c].astype(np.float64)
    pad = cc.pad_of(row)
    xp = np.concatenate([x[len(x) - pad:], x, x[:pad]]) if circular and pad else ck.reflect(x, pad)
    return ck.transform64(np.asarray(cc.bank(row.name) if bank is None else bank, np.float64), xp, det)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_bar_sees_shift_row_order_crop_and_padding(name):
    row = cc.by_name(name)
    c, pad, D = _noise_chunk(row), cc.pad_of(row), 1 << row.r
    ref = ck.reference(name, False)
    good = ref.f64[c]
    assert _bitten(row, False, good, c) == 0.0
    assert _bitten(row, False, np.roll(good, 1, axis=1), c) > BITE, "output shifted by one sample"
    assert _bitten(row, False, good[::-1], c) > BITE, "rows in ascending instead of descending frequency"
    if row.pad:
        full = _uncropped(row, c)
        for off in (-1, 1):
            assert _bitten(row, False, full[:, pad + off:pad + off + D], c) > BITE, f"crop taken from pad {off:+d}"
        assert _bitten(row, False, _uncropped(row, c, circular=True)[:, pad:pad + D], c) > BITE, "circular padding for reflect"
    else:
        # reflect for circular: the time kernels g = IFFT(bank) meet the chunk extended by reflection (exact where g is short
        # against the chunk; the long ones only make the defect larger)
        x = cc.inputs(row)[c].astype(np.float64)
        g = np.fft.ifft(cc.bank(name).astype(np.float64), axis=1)
        g2 = np.zeros((row.num, 2 * D), np.complex128)
        g2[:, :D // 2], g2[:, -(D // 2):] = g[:, :D // 2], g[:, D // 2:]
        bad = np.fft.ifft(np.fft.fft(g2, axis=1) * np.fft.fft(ck.reflect(x, D // 2))[None, :], axis=1)[:, D // 2:D // 2 + D]
        assert _bitten(row, False, bad, c) > BITE, "reflect padding for circular"


@pytest.mark.parametrize("name", FAST)
def test_bar_sees_a_dropped_or_borrowed_support_row(name):
    """L = 2^17: row k2 of the transposed layout = bins [256 k2, 256 k2 + 256).  Flat bands: EVERY scale, its first row dropped
    (1 / w of the band); the other rows: the strongest row of one scale.  Borrowed: the row where a scale differs most from its
    neighbour, taken from that neighbour"""
    row = cc.by_name(name)
    c, pad, D = _noise_chunk(row), cc.pad_of(row), 1 << row.r
    ref = ck.reference(name, False)
    b = cc.bank(name).astype(np.float64).reshape(row.num, 512, 256)
    scales = range(row.num) if name in FLAT else [row.num // 2]
    bad = b.copy()
    for j in scales:
        k2 = int(np.nonzero(b[j].any(axis=1))[0][0]) if name in FLAT else int(np.argmax(np.abs(b[j]).max(axis=1)))
        bad[j, k2] = 0.0
    e = ck.per_scale(_uncropped(row, c, bank=bad.reshape(row.num, -1))[:, pad:pad + D], ref.f64[c]) / ref.bar[c]
    assert np.all(e[list(scales)] > BITE), ("dropped support row", e)
    bad = b.copy()
    for j in scales:
        nb = j + 1 if j + 1 < row.num else j - 1
        k2 = int(np.argmax(np.abs(b[j] - b[nb]).max(axis=1)))
        bad[j, k2] = b[nb, k2]
    e = ck.per_scale(_uncropped(row, c, bank=bad.reshape(row.num, -1))[:, pad:pad + D], ref.f64[c]) / ref.bar[c]
    assert np.all(e[list(scales)] > BITE), ("support row of the neighbouring scale", e)


def test_bar_sees_a_derivative_without_the_negative_mirror():
    """omega = 2 pi k / L on every bin: only a bank with negative-frequency content tells -- the flat bands at rows 512 - w"""
    row = cc.by_name("fast_flat_clamp")
    assert row.det
    c, pad, D = _noise_chunk(row), cc.pad_of(row), 1 << row.r
    L = cc.fft_length(row)
    xp = ck.reflect(cc.inputs(row)[c], pad)
    B = cc.bank(row.name).astype(np.float64) * (1j * 2 * np.pi * np.arange(L) / L)[None, :]
    bad = np.fft.ifft(B * np.fft.fft(xp)[None, :], axis=1)[:, pad:pad + D]
    ref = ck.reference(row.name, True)
    e = ck.per_scale(bad, ref.f64[c]) / ref.bar[c]
    assert np.all(e > BITE), e
