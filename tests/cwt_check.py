"""The reference, the comparison and the runner of the table in tests/cwt_cases.py.

Reference: the operation the kernels perform, in float64, from the BANK and not from wavelet formulas --
    W_j = ifft(bank_j . fft(xp))[pad : pad + D],   xp = the chunk reflect padded (cwt_algorithm.c:404-414) or the chunk itself,
bank_j = the float32 row the object multiplies with (afx_cwt_bank_host / the custom array) taken to float64; the derivative
multiplies by j omega (the omega of cwtObj_enableDet: negative mirror above L / 2).  One formula for all eight families.

Comparison: for every chunk and every scale j over ALL samples  e_j = max|got_j - want_j| / max|want_j|.
Bar: built-in wavelets max(1e-5, 2 r_j), r_j = the compiled reference's own e_j against the same float64 result (the form and
factor of check() in tests/test_realaudio_gpu.py), against float64 and against the compiled reference; custom banks (no
compiled reference) plain 1e-5.  Nothing here is taken from what a kernel returns."""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np

from tests import cwt_cases as cc
from tests.conftest import parity_log

FLOOR, FACTOR = 1e-5, 2.0
KIND = "cwt: per scale max|got - want| / max|want| over all samples, bar max(1e-5, 2 x reference-vs-float64)"


def reflect(x, pad):
    x = np.asarray(x, np.float64)
    return np.concatenate([x[:pad][::-1], x, x[len(x) - pad:][::-1]]) if pad else x


def transform64(bank64, xp, det=False):
    """the uncropped float64 transform [num][L] of an already padded chunk"""
    B = bank64 * (1j * cc.omega(bank64.shape[1]))[None, :] if det else bank64
    return np.fft.ifft(B * np.fft.fft(xp)[None, :], axis=1)


def want64(bank, x, pad, det=False):
    D = len(x)
    return transform64(np.asarray(bank, np.float64), reflect(x, pad), det)[:, pad:pad + D]


def per_scale(got, want):
    """e_j; every scale is judged: an all-zero row of the reference is an error of the table"""
    peak = np.abs(want).max(axis=-1)
    assert np.all(peak > 0), "a scale of the float64 reference is zero throughout"
    return np.abs(np.asarray(got) - want).max(axis=-1) / peak


Ref = namedtuple("Ref", "f64 compiled r bar")  # per transform (plain, derivative): [chunks][num][D] | the same or None | [chunks][num] x 2


def compiled_available():
    from oracle import ref
    return ref.available()


@functools.lru_cache(maxsize=3)
def reference(name, det):
    row = cc.by_name(name)
    bank, x, pad = cc.bank(name), cc.inputs(row), cc.pad_of(row)
    b64 = bank.astype(np.float64)
    f64 = np.stack([want64(b64, xc, pad, det) for xc in x])
    compiled, r = None, np.zeros(f64.shape[:2])
    if not row.custom and compiled_available():
        from oracle import ref
        o = ref.RefCWT(num=row.num, radix2_exp=row.r, samplate=row.sr, low_fre=row.lo, high_fre=row.hi, bin_per_octave=row.bpo,
                       wavelet_type=cc.WAVELET[row.wavelet], scale_type=cc.SCALE[row.scale], gamma=row.gamma, beta=row.beta,
                       is_padding=int(row.pad))
        assert o.status == 0, (name, o.status)
        compiled = np.stack([(lambda a, b: a + 1j * b)(*o.cwt(xc, det=det)) for xc in x])
        r = np.stack([per_scale(c, f) for c, f in zip(compiled, f64)])
        # (the bank of afx_cwt_bank_host IS the reference's for these parameters: another bank would be percent away)
        assert r.max() < 1e-2, f"{name}: the compiled reference is {r.max():.2e} from the float64 transform of the row's bank"
    bar = np.maximum(FLOOR, FACTOR * r)
    for a in (f64, compiled, r, bar):
        if a is not None:
            a.setflags(write=False)
    return Ref(f64, compiled, r, bar)


def scale_classes(row):
    """the kernel each scale of a row runs in, for the log"""
    if row.path != "fast":
        return [row.path] * row.num
    return list(cc.host_plan(row.name).labels)


def judge(row, got, det=False, tag=""):
    """got [chunks][num][D] complex, C order (row 0 = the highest frequency).  Every scale of every chunk at every sample, against
    float64 and against the compiled reference where there is one; returns the worst error / bar"""
    what = f"{row.name}{' derivative' if det else ''}{tag}"
    assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), f"{what}: non-finite results (a sample nobody wrote?)"
    ref = reference(row.name, det)
    assert got.shape == ref.f64.shape, (what, got.shape, ref.f64.shape)
    classes = scale_classes(row)
    worst_ratio, fails = 0.0, []
    for target, want in (("float64", ref.f64), ("compiled reference", ref.compiled)):
        if want is None:
            continue
        e = np.stack([per_scale(g, w) for g, w in zip(got, want)])  # [chunk][scale]
        for cls in sorted(set(classes)):
            sel = [j for j in range(row.num) if classes[j] == cls]
            ratio = e[:, sel] / ref.bar[:, sel]
            c, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            print(f"{what} vs {target}, {cls}: worst {e[c, sel[k]]:.2e} (chunk {c}, scale {sel[k]}; bar {ref.bar[c, sel[k]]:.2e}, "
                  f"reference vs float64 {ref.r[c, sel[k]]:.2e}); largest error {e[:, sel].max():.2e}", flush=True)
            parity_log(f"{what} vs {target}", e[c, sel[k]], ref.bar[c, sel[k]], KIND,
                       {"row": row.name, "path": row.path, "class": cls, "reference_vs_float64": float(ref.r[c, sel[k]]),
                        "largest_error": float(e[:, sel].max())})
        ratio = e / ref.bar
        worst_ratio = max(worst_ratio, float(ratio.max()))
        for c, j in zip(*np.nonzero(ratio > 1.0)):
            fails.append(f"chunk {c} ({row.x[c][0]}) scale {j} ({classes[j]}) vs {target}: {e[c, j]:.3e} > {ref.bar[c, j]:.3e}")
    assert not fails, f"{what}: {len(fails)} scale(s) over their bar: " + "; ".join(fails[:8])
    return worst_ratio


# ---- the runner (device) ------------------------------------------------------------------------------------------------------
def custom_object(row):
    import audioflux_amd as af

    class Custom(af.CWT):
        def __init__(self, row):
            from audioflux_amd import _lib
            self._lib = _lib.get_lib()
            self._obj = C.c_void_p(None)
            self.num, self.radix2_exp, self.fft_length = row.num, row.r, 1 << row.r
            bank = np.ascontiguousarray(cc.bank(row.name))
            fre, bins = np.arange(row.num, 0, -1, dtype=np.float32), np.arange(row.num, 0, -1, dtype=np.int32)
            fn = self._lib.afx_cwt_create_custom
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
            st = fn(C.byref(self._obj), row.num, row.r, row.sr, int(row.pad), bank.ctypes.data, fre.ctypes.data, bins.ctypes.data,
                    b"tests/cwt_check.py")
            _lib.check(st, "afx_cwt_create_custom")

    return Custom(row)


def make(row):
    """the object of a row; AFX_CWT_NARROW_MAX (read when an object is created) is the caller's to set"""
    import audioflux_amd as af
    if row.custom:
        return custom_object(row)
    return af.CWT(num=row.num, radix2_exp=row.r, samplate=row.sr, low_fre=row.lo, high_fre=row.hi, bin_per_octave=row.bpo,
                  wavelet_type=af.WaveletContinueType(cc.WAVELET[row.wavelet]), scale_type=af.SpectralFilterBankScaleType(cc.SCALE[row.scale]),
                  gamma=row.gamma, beta=row.beta, is_padding=row.pad)


def set_narrow_max(row, env=os.environ):
    if row.narrow_max is None:
        env.pop("AFX_CWT_NARROW_MAX", None)
    else:
        env["AFX_CWT_NARROW_MAX"] = str(row.narrow_max)


def plan_counts(o):
    out = (C.c_int * 10)(*([-1] * 10))
    fn = o._lib.afx_cwt_plan_counts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int * 10]
    assert fn(o._obj, out) == 0
    return tuple(out)


def run_device(o, row, det=False):
    """the batched device entry on all chunks of the row -> complex128 [chunks][num][D].  The outputs are NaN beforehand (the
    wrapper allocates with torch.empty).  `shift` rows: chunk 0 starts 4 bytes behind a 16-byte boundary, odd chunk stride"""
    import torch
    x = cc.inputs(row)
    chunks, D = x.shape
    if row.shift:
        stride = D + 3
        base = torch.zeros(chunks * stride + 8, dtype=torch.float32, device="cuda")
        assert base.data_ptr() % 16 == 0
        xd = torch.as_strided(base, (chunks, D), (stride, 1), 1)
        xd.copy_(torch.from_numpy(x))
        assert xd.data_ptr() % 16 == 4 and xd.stride(0) % 2 == 1
    else:
        xd = torch.from_numpy(x).cuda()
    re = torch.full((chunks, row.num, D), float("nan"), dtype=torch.float32, device="cuda")
    im = torch.full_like(re, float("nan"))
    o.cwt_device(xd, out_real=re, out_imag=im, det=det)
    torch.cuda.synchronize()
    return re.cpu().numpy(), im.cpu().numpy()


def run_host(o, row, chunk=0, det=False):
    """the one-chunk host entry, back in the library's row order"""
    w = (o.cwt_det if det else o.cwt)(cc.inputs(row)[chunk])[::-1]
    return np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
