"""CPU-only: the packed band plan (afx_bandplan.c: afx_bandpack_build, AfxBandPack in afx_bandpack.h) -- one stream of three
partitions a | b | c per lane, each partition continuing the row before it or starting a new one.  For every plan it makes:
the weights re-assemble the dense bank exactly, every row appears once and in ONE chain with its taps in ascending bin order,
bases are even and stay inside the power row's zero pad, the continuation flags agree with the bases, and the lane pairs that
meet on an LDS bank pair are the number it reports.  The banks are those of tests/test_bandplan.py.

Headline bank (mel-128, 16 kHz, n_fft 2048) on the compiled layout: the bounds are those of a crude search (rows dealt to
classes by length, one matching per partition in turn): 48 slots with one conflicting row.  The planner's own numbers:
48 slots, no conflicting row."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af
from oracle import restate
from tests.test_bandplan import Band, _bank

ROW_CAP = 1104                 # floats of k_stft_mel_v2's zero-padded power row (PROW_F)
COMPILED = ((24, 12, 12),)     # kPacks of afx_melfused2.hip
WIDE = ((24, 12, 12), (32, 16, 16), (40, 16, 16), (48, 24, 24), (64, 32, 32))  # the planner itself takes any layouts
BANKS = [(128, 2048, 16000, "slaney"), (128, 2048, 32000, "slaney"), (80, 2048, 16000, "etsi"), (64, 2048, 16000, "slaney"),
         (40, 2048, 16000, "slaney"), (128, 2048, 44100, "etsi"), (13, 2048, 8000, "slaney")]


class Pack(C.Structure):
    _fields_ = [("num", C.c_int), ("taps", C.c_int * 3), ("slots", C.c_int), ("conflicts", C.c_int),
                ("base", (C.c_int * 64) * 3), ("row", (C.c_int * 64) * 3), ("cont", (C.c_int * 64) * 3),
                ("w", C.POINTER(C.c_float))]


def whole_plan(bank):
    b = Band()
    fp = C.POINTER(C.c_float)
    assert af.get_lib().afx_bandplan_build(bank.ctypes.data_as(fp), bank.shape[0], bank.shape[1], C.byref(b)) == 0
    return b


def pack(b, layouts, cur_slots):
    p = Pack()
    lay = ((C.c_int * 3) * len(layouts))(*layouts)
    rc = af.get_lib().afx_bandpack_build(C.byref(b), lay, len(layouts), ROW_CAP, cur_slots, C.byref(p))
    assert rc in (0, 1)
    if rc:
        assert not p.w and p.slots == 0  # nothing left allocated
    return rc, p


def conflicting_rows(base):
    """lanes of a 32-lane half beyond the first on a bank pair (ds_read_b64: 32 pairs of banks), over the three partitions"""
    return sum(32 - len(set((base[q, 32 * h:32 * h + 32] // 2) % 32)) for q in range(3) for h in range(2))


def check(p, bank):
    num, F = bank.shape
    taps = list(p.taps)
    assert p.slots == sum(taps) and all(t > 0 and t % 4 == 0 for t in taps) and p.num == num
    w = np.ctypeslib.as_array(p.w, (p.slots, 64))
    base, row, cont = np.array(p.base), np.array(p.row), np.array(p.cont)
    off = [0, taps[0], taps[0] + taps[1]]
    assert (cont[0] == 0).all() and set(np.unique(cont)) <= {0, 1}
    assert (base >= 0).all() and (base % 2 == 0).all()
    for q in range(3):
        assert (base[q] + taps[q] <= ROW_CAP).all()  # no read past the power row's zero pad
    rec = np.zeros_like(bank)
    seen, rows_per_lane = [], []
    for l in range(64):
        chain, n = [], 0
        for q in range(3):
            if cont[q, l]:
                assert base[q, l] == base[q - 1, l] + taps[q - 1]  # a continued partition reads on where the last one ended
                assert row[q - 1, l] == -1                          # ... and the row is stored once, from its last partition
            else:
                chain = []
            chain += [(base[q, l] + k, w[off[q] + k, l]) for k in range(taps[q])]
            last = q == 2 or not cont[q + 1, l]
            if row[q, l] >= 0:
                assert last
                bins = [b for b, v in chain if v != 0]
                assert bins == sorted(bins) and len(set(bins)) == len(bins) and max(bins) < F
                for b, v in chain:
                    if v != 0:
                        rec[row[q, l], b] += v
                seen.append(int(row[q, l]))
                n += 1
            elif last:
                assert all(v == 0 for _, v in chain)  # an empty chain
        rows_per_lane.append(n)
    assert np.array_equal(rec, bank)
    assert sorted(seen) == list(range(num))
    if num == 128:
        assert rows_per_lane.count(3) == rows_per_lane.count(1)  # as many lanes carry three rows as carry one
    got = conflicting_rows(base)
    pairs = sum(c * (c - 1) // 2 for q in range(3) for h in range(2)
                for c in np.bincount((base[q, 32 * h:32 * h + 32] // 2) % 32, minlength=32))
    assert p.conflicts == pairs and (got == 0) == (pairs == 0)
    assert pairs <= 1  # AFX_BANDPACK_MAX_PAIRS: the planner declines a layout that it cannot place with fewer
    return got


def test_headline_bank_on_the_compiled_layout():
    bank, _, _ = restate.mel_bank(128, 2048, 16000, 0, 8000, "slaney")
    b = whole_plan(bank)
    assert b.tapsA <= 48 and b.tapsB <= 16  # the (48, 16) variant runs it today
    rc, p = pack(b, COMPILED, 48 + 16)
    assert rc == 0
    rows = check(p, bank)
    print(f"headline bank: {p.slots} slots, {rows} conflicting rows, {p.conflicts} lane pairs")
    assert p.slots <= 48 and rows <= 1
    af.get_lib().afx_bandpack_free(C.byref(p))
    # the same plan again: the planner is deterministic
    rc, p2 = pack(b, COMPILED, 64)
    assert rc == 0 and np.array_equal(np.array(p2.base), np.array(p.base)) and np.array_equal(np.array(p2.row), np.array(p.row))
    af.get_lib().afx_bandpack_free(C.byref(p2))
    af.get_lib().afx_bandplan_free(C.byref(b))


@pytest.mark.parametrize("num,n,sr,style", BANKS)
def test_packed_plans_of_the_bandplan_banks(num, n, sr, style):
    """every bank of tests/test_bandplan.py, on the compiled layout (against the (48, 16) variant's 64 slots) and on a wider set
    that holds the longer rows of the other banks too"""
    bank, _, _ = restate.mel_bank(num, n, sr, 0, sr / 2, style)
    b = whole_plan(bank)
    # slots a row needs: its taps, and one more when its first bin is odd (bases are even)
    longest = max(int(np.nonzero(r)[0][-1] - np.nonzero(r)[0][0] + 1 + (np.nonzero(r)[0][0] & 1)) for r in bank)
    for layouts, cur in ((COMPILED, 64), (WIDE, 1 << 20)):
        rc, p = pack(b, layouts, cur)
        fits = [sum(t) for t in layouts if sum(t) >= longest]
        if num <= 64:
            assert rc == 1  # mel-13 / -40 / -64: at most one row per lane, nothing to pack
            continue
        if not fits:
            assert rc == 1  # a row longer than every layout
            continue
        assert rc == 0 and p.slots == min(fits) and p.slots >= longest
        rows = check(p, bank)
        print(f"mel-{num} at {sr} Hz ({style}): longest row {longest}, layout {list(p.taps)}, {rows} conflicting rows")
        af.get_lib().afx_bandpack_free(C.byref(p))
    af.get_lib().afx_bandplan_free(C.byref(b))


def test_declines():
    lib = af.get_lib()
    fp = C.POINTER(C.c_float)
    # not shorter than the variant the bank would otherwise run
    bank, _, _ = restate.mel_bank(128, 2048, 16000, 0, 8000, "slaney")
    b = whole_plan(bank)
    assert pack(b, COMPILED, 48)[0] == 1
    rc, p = pack(b, COMPILED, 49)
    assert rc == 0
    lib.afx_bandpack_free(C.byref(p))
    # a layout that holds the rows (longest: 44 slots) but is only placed with several conflicting pairs
    assert pack(b, ((24, 12, 8),), 64)[0] == 1
    lib.afx_bandplan_free(C.byref(b))
    # a split plan
    sb = _bank(64, 2048, 16000, "mel")
    s = Band()
    assert lib.afx_bandplan_build_split(sb.ctypes.data_as(fp), 64, 1025, 48, 16, ROW_CAP, C.byref(s)) == 0 and s.split == 1
    s.num = 128  # (were it not for the flag ...)
    assert pack(s, COMPILED, 64)[0] == 1
    lib.afx_bandplan_free(C.byref(s))
    # a row of 100 taps among 128 rows
    wide = np.zeros((128, 1025), np.float32)
    for m in range(128):
        wide[m, 4 * m:4 * m + 6] = 1.0 + m
    wide[77, 300:400] = 0.5
    b = whole_plan(wide)
    assert b.tapsA >= 100
    assert pack(b, COMPILED, 1 << 20)[0] == 1
    rc, p = pack(b, ((64, 32, 32),), 1 << 20)  # (a layout that holds it: the planner itself has no trouble with the bank)
    assert rc == 0
    check(p, wide)
    lib.afx_bandpack_free(C.byref(p))
    lib.afx_bandplan_free(C.byref(b))
