"""The continuous wavelet transform scale by scale: the table of tests/test_cwt_cases_cpu.py and tests/test_cwt_cases_gpu.py
(numpy + the library's device-free bank / plan entry points only; the comparison is tests/cwt_check.py).

Five execution paths, chosen by the transform length L (2 x 2^r for a reflect-padded chunk, 2^r for an unpadded, circular one):
  small    L <= 2^14: k_cwt_small_fwd / _inv, the whole transform in LDS
  generic  L = 2^15, 2^16, >= 2^18, and every L under AFX_NO_FUSED: k_cwt_fwd_cols / _rows, k_cwt_inv_rows / _cols
  fast     L = 2^17: per scale one of
             wide    k_cwt_inv_rows512 + k_cwt_inv_cols256 (support of more rows of the transposed spectrum than the widest class)
             narrow  k_cwt_inv_cols256_nb<2 4 8 16>, _nb2<4 8 16>: support <= R rows, R = 2, 4, 8, 16, 20, 24, 32
             td      k_cwt_td<1024> / <384>: a short time kernel, two tap classes (K <= 384 and K <= 1024 with the 8 phase shifts)

A row is named for what it reaches.  `counts` is the plan the object must report (afx_cwt_plan_counts: nTd, derivative images,
nWide, the seven narrow classes); tests/test_cwt_cases_cpu.py derives the same numbers on the host -- the narrow classes through
afx_cwt_support_host / afx_cwt_classify_host, the time-domain scales through `td_half_lengths`, a restatement of td_candidates
(afx_cwt.c) -- so a row cannot silently stop reaching its kernel when a planning rule changes.

(2^17 samples cannot be padded: the reference leaves powers of two there and the library refuses -- L = 2^18 is reached by
2^18 unpadded samples.)"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from tests import cases

WAVELET, SCALE = cases.WAVELET, cases.SCALE
FAMILIES = tuple(WAVELET)
DEFAULTS = {"morse": (3, 20), "morlet": (6, 2), "bump": (5, 0.6), "paul": (4, 2), "dog": (2, 2), "mexican": (2, 2), "hermit": (5, 2),
            "ricker": (4, 2)}
CLASS_ROWS = (2, 4, 8, 16, 20, 24, 32)
FLAT_WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 21, 24, 25, 32, 33)  # either side of every class boundary
TD_MAXK, TD_SHORTK = 1024, 384  # afx_device.h AFX_CWT_TD_MAXK, afx_cwt_td.hip SHORTK
L17 = 1 << 17
ERR_UNSUPPORTED, ERR_ARG = -4, -6  # afx_device.h AFX_ERR_UNSUPPORTED, AFX_ERR_ARG

Row = namedtuple("Row", "name path r pad num x wavelet gamma beta scale sr lo hi bpo custom det counts det_images narrow_max td_det shift nofused")


def _row(name, path, r, pad, num, x, wavelet=None, scale="log", sr=32000, lo=None, hi=None, bpo=12, custom=None, det=False,
         counts=None, det_images=0, narrow_max=None, td_det=("1",), shift=False, nofused=False):
    g, b = DEFAULTS[wavelet] if wavelet else (None, None)
    return Row(name, path, r, bool(pad), num, tuple(x), wavelet, g, b, scale, sr, lo, hi if hi is not None else sr / 2.0, bpo, custom, det,
               tuple(counts) if counts else (0,) * 10, det_images, narrow_max, tuple(td_det), shift, nofused)


N1, N2, N3 = (("noise", 11),), (("noise", 21), ("level_step",)), (("level_step",), ("dc_offset",), ("noise", 31))


def _flat_rows():
    """flat-top bands: 1.0 on rows [lo, lo + w) of the transposed layout, every width at lo = 0 (bin 0 included), 1, a mid value
    and 256 - w (the band ends at the Nyquist row); and, one width per class, w < R at lo = 512 - w, where lo + R would
    leave the spectrum: the kernels clamp to lo = 512 - R.  Widths 1 ... 32 with AFX_CWT_NARROW_MAX=32: two per class, 33: two-pass"""
    per_lo = (0, 1, 2, 2, 2, 2, 2, 2, 2, 2)  # nTd, det images, nWide (w = 33: a sinc has no short kernel), two widths per class
    rows = []
    for tag, lo_of in (("row0", lambda w: 0), ("row1", lambda w: 1), ("mid", lambda w: 97), ("nyquist", lambda w: 256 - w)):
        bands = tuple((lo_of(w), w) for w in FLAT_WIDTHS)
        rows.append(_row(f"fast_flat_{tag}", "fast", 16, True, len(bands), N1, custom=("flat", bands), counts=(0, 0, 1) + per_lo[3:],
                         narrow_max=32))
    bands = tuple((512 - w, w) for w in (1, 3, 5, 9, 17, 21, 25))
    rows.append(_row("fast_flat_clamp", "fast", 16, True, len(bands), N2, custom=("flat", bands), counts=(0, 0, 0, 1, 1, 1, 1, 1, 1, 1),
                     narrow_max=32, det=True, nofused=True))  # (negative frequencies: the one bank that sees the mirror of the
    #                                  derivative's omega.  AFX_NO_FUSED: no two-pass scale in the plan, yet every scale takes both generic passes)
    return rows


# Gaussian bands exp(-(k - c)^2 / (2 s^2)) around bin c = 20000: time kernel exp(-(2 pi s t / L)^2 / 2), above 1e-6 of its peak
# for |t| < 109655 / s; half length kh = ceil(1.08 k6) + 2 (td_candidates).  Pair images hold 2 roundup8(kh) + 8 taps rounded up to
# 32: kh <= 184 -> 384 taps (the short class), kh >= 185 -> the long one, kh <= 480 the last that fits (2 kh + 8 <= 968), above:
# two passes on the FFT path (support 28.8 s bins > 20 rows).  s: 650 -> kh 184, 643 -> 186, 248 -> 480, 246 -> 483
GAUSS_C = 20000
TD_KH = {650: 184, 643: 186, 248: 480, 246: None}


def _gauss_rows():
    """time-domain pairs are formed longest first and a pair's image is sized by its longer kernel: the 186 half length meets the
    416-tap image -- the first of the long class -- only as the LONGER member of a pair, so it has a row where it is that"""
    return [_row("fast_gauss_td_one_unpaired_short", "fast", 16, True, 2, N2, custom=("mixed", (("gauss", 650), ("flat", 40, 4))),
                 counts=(1, 0, 0, 0, 1, 0, 0, 0, 0, 0), det_images=1, det=True),
            _row("fast_gauss_td_pair_416_taps_first_of_the_long_class", "fast", 16, True, 3, N2,
                 custom=("mixed", (("gauss", 650), ("flat", 40, 4), ("gauss", 643))),
                 counts=(2, 0, 0, 0, 1, 0, 0, 0, 0, 0), det_images=1, det=True),
            _row("fast_gauss_td_pair_and_unpaired_both_classes_and_overlength", "fast", 16, True, 5, N2,
                 custom=("mixed", (("gauss", 650), ("gauss", 246), ("gauss", 643), ("flat", 40, 4), ("gauss", 248))),
                 counts=(3, 0, 1, 0, 1, 0, 0, 0, 0, 0), det_images=1)]


# built-in families on the fast path: one log-spaced bank per family whose 16 scales run from a few rows of support to hundreds
FAST_RANGE = {"morse": (40.0, 14000.0), "morlet": (40.0, 14000.0), "bump": (40.0, 14000.0), "paul": (33.0, 4000.0),
              "dog": (33.0, 6000.0), "mexican": (33.0, 6000.0), "hermit": (40.0, 14000.0), "ricker": (33.0, 6000.0)}
# (nTd, derivative images, nWide, narrow classes) at the default AFX_CWT_NARROW_MAX (20): the host plan, see the CPU tests
# (the same for both paddings: L, and with it the bank, is the same).  Only the Morlet wavelet -- a Gaussian in frequency, so one
# in time -- has short kernels; the others are one-sided with a kink at zero or compactly supported: algebraic tails
FAST_COUNTS = {"morse": ((0, 0, 8, 2, 1, 2, 2, 1, 0, 0), 0), "morlet": ((8, 0, 1, 1, 2, 2, 1, 1, 0, 0), 1),
               "bump": ((0, 0, 2, 7, 2, 2, 2, 1, 0, 0), 0), "paul": ((0, 0, 13, 0, 0, 0, 2, 1, 0, 0), 0),
               "dog": ((0, 0, 11, 0, 1, 2, 2, 0, 0, 0), 0), "mexican": ((0, 0, 11, 0, 1, 2, 2, 0, 0, 0), 0),
               "hermit": ((0, 0, 9, 1, 2, 2, 2, 0, 0, 0), 0), "ricker": ((0, 0, 11, 0, 1, 2, 2, 0, 0, 0), 0)}
FAST_DET = ("morlet", "morse", "dog", "mexican")


def _family_rows():
    rows = []
    for fam in FAMILIES:
        lo, hi = FAST_RANGE[fam]
        for tag, r, pad in (("r16_pad", 16, True), ("r17_wrap", 17, False)):
            det = fam in FAST_DET and (pad or fam == "morlet")
            c = FAST_COUNTS[fam]
            rows.append(_row(f"fast_{tag}_{fam}", "fast", r, pad, 16, N3 if pad else N2, wavelet=fam, sr=44100, lo=lo, hi=hi, det=det,
                             counts=c[0], det_images=c[1],
                             td_det=("1", "0") if (fam, pad) == ("morlet", True) else ("1",),
                             shift=(fam, pad) == ("morlet", True), nofused=(fam, pad) == ("bump", True)))
    # AFX_CWT_NARROW_MAX=32: the two widest classes with a built-in family
    rows.append(_row("fast_r16_pad_dog_narrow_max_32", "fast", 16, True, 16, N1, wavelet="dog", sr=44100, lo=33.0, hi=6000.0,
                     narrow_max=32, counts=(0, 0, 9, 0, 1, 2, 2, 0, 1, 1)))
    return rows


def _small_and_generic_rows():
    S = lambda *a, **k: _row(*a, nofused=True, **k)
    return [
        # the whole transform in LDS; the last size is L = 2^14.  (All of these again under AFX_NO_FUSED: the generic kernels at
        # L = 2^4 ... 2^14, r1 = r2 and r1 != r2, tiles narrower than 16 columns)
        S("small_r3_pad_ricker", "small", 3, True, 3, N3, wavelet="ricker", scale="erb", sr=16000, lo=500.0, hi=6000.0),
        S("small_r8_wrap_hermit", "small", 8, False, 20, N3, wavelet="hermit", scale="bark", sr=16000, lo=100.0, hi=6000.0),
        S("small_r8_wrap_paul", "small", 8, False, 12, N2, wavelet="paul", scale="linspace", sr=8000, lo=200.0, hi=3000.0, det=True),
        S("small_r13_pad_morse", "small", 13, True, 12, N3, wavelet="morse", sr=32000, lo=60.0, hi=12000.0, det=True),
        S("small_r13_pad_bump", "small", 13, True, 12, N2, wavelet="bump", scale="mel", sr=16000, lo=50.0, hi=7000.0),
        S("small_r13_pad_dog", "small", 13, True, 12, N2, wavelet="dog", sr=32000, lo=100.0, hi=9000.0),
        S("small_r14_wrap_morlet", "small", 14, False, 12, N3, wavelet="morlet", sr=32000, lo=40.0, hi=12000.0, det=True),
        S("small_r14_wrap_mexican", "small", 14, False, 12, N2, wavelet="mexican", sr=32000, lo=100.0, hi=9000.0),
        # four-step kernels: L = 2^15 (r1 = 7, r2 = 8), 2^16 padded and circular, 2^18
        _row("generic_r14_pad_morlet", "generic", 14, True, 12, N3, wavelet="morlet", sr=32000, lo=40.0, hi=12000.0),
        _row("generic_r15_pad_paul_det", "generic", 15, True, 12, N2, wavelet="paul", scale="mel", sr=32000, lo=50.0, hi=12000.0, det=True),
        _row("generic_r15_pad_hermit", "generic", 15, True, 12, N2, wavelet="hermit", sr=32000, lo=60.0, hi=12000.0),
        _row("generic_r16_wrap_dog", "generic", 16, False, 12, N3, wavelet="dog", sr=44100, lo=50.0, hi=15000.0),
        _row("generic_r16_wrap_morse", "generic", 16, False, 12, N2, wavelet="morse", scale="erb", sr=44100, lo=50.0, hi=15000.0),
        _row("generic_r18_wrap_bump", "generic", 18, False, 8, N1, wavelet="bump", sr=44100, lo=40.0, hi=15000.0),
    ]


@functools.lru_cache(maxsize=None)
def table():
    rows = _small_and_generic_rows() + _family_rows() + _flat_rows() + _gauss_rows()
    names = [r.name for r in rows]
    assert len(set(names)) == len(names), "row names must be unique"
    for r in rows:
        assert r.num <= (8 if r.r >= 18 else 16 if fft_length(r) >= L17 else 20) and len(r.x) <= 3, r.name
    return tuple(rows)


def by_name(name):
    return next(r for r in table() if r.name == name)


def fft_length(row):
    return (2 if row.pad else 1) << row.r


def pad_of(row):
    return (1 << row.r) // 2 if row.pad else 0


# ---- inputs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk(spec, n):
    """one chunk of 2^r samples, float32, read-only: white noise, or a hard clip repeated to the length (np.resize)"""
    x = cases.noise(spec[1], n) if spec[0] == "noise" else np.resize(cases.hard_clip(spec[0]), n).astype(np.float32)
    x.setflags(write=False)
    return x


def inputs(row):
    return np.stack([chunk(s, 1 << row.r) for s in row.x])


# ---- banks --------------------------------------------------------------------------------------------------------------------
def _flat(L, lo, w):
    b = np.zeros(L, np.float32)
    b[256 * lo:256 * (lo + w)] = 1.0
    return b


def _gauss(L, s):
    k = np.arange(L // 2, dtype=np.float64)
    b = np.zeros(L, np.float32)
    b[:L // 2] = np.exp(-0.5 * ((k - GAUSS_C) / s) ** 2).astype(np.float32)  # (float32 flushes the tails to zero: a finite support)
    return b


def custom_bank(row):
    L = fft_length(row)
    kind, spec = row.custom
    if kind == "flat":
        return np.stack([_flat(L, lo, w) for lo, w in spec])
    assert kind == "mixed"
    return np.stack([_flat(L, *s[1:]) if s[0] == "flat" else _gauss(L, s[1]) for s in spec])


_FP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_int)


def _lib():
    import audioflux_amd as af
    return af.get_lib()


@functools.lru_cache(maxsize=8)
def bank(name):
    """[num][L] float32 in natural bin order, row 0 = the highest centre frequency: the array the object multiplies with -- the
    custom array, or the library's own bank for the resolved parameters of the row (afx_cwt_bank_host)"""
    row = by_name(name)
    if row.custom:
        b = custom_bank(row)
    else:
        lib = _lib()
        lib.afx_cwt_bank_host.restype = C.c_int
        lib.afx_cwt_bank_host.argtypes = [C.c_int] * 5 + [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, _FP, _FP, _IP]
        b = np.zeros((row.num, fft_length(row)), np.float32)
        st = lib.afx_cwt_bank_host(row.num, 1 << row.r, row.sr, pad_of(row), WAVELET[row.wavelet], row.gamma, row.beta, SCALE[row.scale],
                                   row.lo, row.hi, row.bpo, b.ctypes.data_as(_FP), None, None)
        assert st == 0, st
    b.setflags(write=False)
    return b


# ---- the plan on the host -----------------------------------------------------------------------------------------------------
def support(b):
    lib = _lib()
    sup = np.zeros(2 * len(b), np.int32)
    lib.afx_cwt_support_host.restype = None
    lib.afx_cwt_support_host.argtypes = [_FP, C.c_int, C.c_longlong, C.c_int, _IP]
    lib.afx_cwt_support_host(np.ascontiguousarray(b).ctypes.data_as(_FP), len(b), b.shape[1], 8, sup.ctypes.data_as(_IP))
    return sup


def classify(sup, max_r):
    lib = _lib()
    num = len(sup) // 2
    order, n_wide, n_narrow = np.full(num, -1, np.int32), C.c_int(-1), (C.c_int * 7)(*([-1] * 7))
    lib.afx_cwt_classify_host.restype = None
    lib.afx_cwt_classify_host.argtypes = [_IP, C.c_int, C.c_int, _IP, _IP, C.c_int * 7]
    lib.afx_cwt_classify_host(sup.ctypes.data_as(_IP), num, max_r, order.ctypes.data_as(_IP), C.byref(n_wide), n_narrow)
    return order, n_wide.value, list(n_narrow)


def omega(L):
    """the angular frequencies of cwtObj_enableDet: 2 pi k / L up to L / 2, their negative mirror above"""
    w = 2 * np.pi * np.arange(L) / L
    w[L // 2 + 1:] = -w[1:L - L // 2][::-1]
    return w


def td_half_lengths(b, scales, D, pad, det=False):
    """td_candidates (afx_cwt.c) restated: for each scale of `scales` the half length kh of its time kernel g = IFFT(psi) --
    the last |t| above 1e-6 of the peak, x 1.08, + 2 -- or None where the kernel does not fit the image (2 kh + 8 > 968), is
    longer than the padding or the chunk, or leaves more than 5e-7 of its L2 norm outside"""
    L = b.shape[1]
    out = []
    for j in scales:
        row = b[j].astype(np.float64)
        if det:
            row = 1j * (b[j] * omega(L).astype(np.float32)).astype(np.float32).astype(np.float64)
        a2 = np.abs(np.fft.ifft(row) * L) ** 2
        peak = a2.max()
        if not peak > 0:
            out.append(None)
            continue
        k = np.nonzero(a2 > 1e-12 * peak)[0]
        k6 = int(np.minimum(k, L - k).max())
        kh = int(np.ceil(1.08 * k6)) + 2
        if 2 * kh + 8 > TD_MAXK - 56 or (pad > 0 and kh > pad) or kh >= D or a2[kh + 1:L - kh].sum() > 2.5e-13 * a2.sum():
            out.append(None)
        else:
            out.append(kh)
    return out


def taps_of(kh):
    """taps of the pair image whose longer kernel has half length kh (td_upload)"""
    return max(64, (2 * ((kh + 7) & ~7) + 8 + 31) & ~31)


Plan = namedtuple("Plan", "counts det_images kh kh_det width labels")  # labels: per scale "td", "wide" or "narrow<R>"


@functools.lru_cache(maxsize=None)
def host_plan(name):
    """the plan cwt_create makes for a fast-path row, from the bank alone"""
    row = by_name(name)
    assert row.path == "fast" and fft_length(row) == L17
    b = bank(name)
    sup = support(b)
    order, n_wide, n_narrow = classify(sup, row.narrow_max if row.narrow_max is not None else 20)
    wide = [int(j) for j in order[:n_wide]]
    kh = td_half_lengths(b, wide, 1 << row.r, pad_of(row))
    td = [j for j, h in zip(wide, kh) if h is not None]
    assert len(td) <= 96
    khd = td_half_lengths(b, td, 1 << row.r, pad_of(row), det=True) if td else []
    det_images = int(bool(td) and all(h is not None for h in khd))
    labels = {j: "wide" if h is None else "td" for j, h in zip(wide, kh)}
    pos = n_wide
    for cls, n in zip(CLASS_ROWS, n_narrow):
        labels.update({int(j): f"narrow{cls}" for j in order[pos:pos + n]})
        pos += n
    return Plan((len(td), 0, n_wide - len(td)) + tuple(n_narrow), det_images, tuple(h for h in kh if h is not None), tuple(khd),
                tuple(int(w) for w in sup[1::2] - sup[0::2]), tuple(labels[j] for j in range(row.num)))
