"""The CWT kernels scale by scale on the device: every row of tests/cwt_cases.py through af.CWT / afx_cwt_create_custom and the
batched device entry, every scale of every chunk at every sample against the float64 transform of the row's own bank and against
the compiled reference (tests/cwt_check.py: bar max(1e-5, 2 x the reference's own distance from float64), custom banks 1e-5).
Each row also asserts the plan the object reports (afx_cwt_plan_counts) -- the kernels the row is named for -- and that the
one-chunk host entry returns the same bits as the device entry."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cwt_cases as cc
from tests import cwt_check as ck

pytestmark = pytest.mark.gpu
ROWS = cc.table()


def _need_reference(row):
    if not row.custom and not ck.compiled_available():
        pytest.skip("compiled reference not built (the bar of a built-in wavelet is taken from it)")


def _one_transform(o, row, det, tag=""):
    re, im = ck.run_device(o, row, det)
    hre, him = ck.run_host(o, row, 0, det)
    ck.judge(row, re.astype(np.float64) + 1j * im, det, tag)
    assert np.array_equal(hre, re[0]) and np.array_equal(him, im[0]), f"{row.name}: host entry and device entry differ on chunk 0"


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_row(name, monkeypatch):
    import torch  # noqa: F401
    row = cc.by_name(name)
    _need_reference(row)
    ck.set_narrow_max(row, _Env(monkeypatch))
    for i, td_det in enumerate(row.td_det):
        monkeypatch.setenv("AFX_CWT_TD_DET", td_det)  # (read by cwtObj_enableDet)
        o = ck.make(row)
        assert ck.plan_counts(o) == row.counts, (ck.plan_counts(o), row.counts)
        if i == 0:
            _one_transform(o, row, False)
        if row.det:
            o.enable_det(True)
            want = row.counts[:1] + (row.det_images if td_det == "1" else 0,) + row.counts[2:]
            assert ck.plan_counts(o) == want, (ck.plan_counts(o), want)
            _one_transform(o, row, True, f" AFX_CWT_TD_DET={td_det}" if len(row.td_det) > 1 else "")
        del o


class _Env:
    """os.environ's pop / item assignment on a monkeypatch"""

    def __init__(self, mp):
        self.mp = mp

    def pop(self, key, default=None):
        self.mp.delenv(key, raising=False)

    def __setitem__(self, key, value):
        self.mp.setenv(key, value)


# ---- the size-generic kernels at the small and the fast sizes: AFX_NO_FUSED is read once per process ------------------------------
NOFUSED = [r.name for r in ROWS if r.nofused]


def _nofused_child(out):
    import torch  # noqa: F401
    assert os.environ.get("AFX_NO_FUSED")
    res = {}
    for name in NOFUSED:
        row = cc.by_name(name)
        ck.set_narrow_max(row)
        o = ck.make(row)
        for det in ((False, True) if row.det else (False,)):
            if det:
                o.enable_det(True)
            re, im = ck.run_device(o, row, det)
            hre, him = ck.run_host(o, row, 0, det)
            assert np.array_equal(hre, re[0]) and np.array_equal(him, im[0]), f"{name}: host entry and device entry differ on chunk 0"
            res[f"{name}/{int(det)}/re"], res[f"{name}/{int(det)}/im"] = re, im
        del o
    np.savez(out, **res)


def test_generic_kernels_at_small_and_fast_sizes(tmp_path):
    """every small-path row (L = 2^4, 2^8, 2^14) and one L = 2^17 row through k_cwt_fwd_cols / _rows and k_cwt_inv_rows / _cols:
    one fresh child process with AFX_NO_FUSED set; its arrays are judged here, at the bars of the rows"""
    for name in NOFUSED:
        _need_reference(cc.by_name(name))
    out = str(tmp_path / "nofused.npz")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {os.getcwd()!r}); from tests import test_cwt_cases_gpu as t; "
                        f"t._nofused_child({out!r})"], capture_output=True, text=True, env=dict(os.environ, AFX_NO_FUSED="1"), timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    for name in NOFUSED:
        row = cc.by_name(name)
        for det in ((False, True) if row.det else (False,)):
            ck.judge(row._replace(path="generic"), z[f"{name}/{int(det)}/re"].astype(np.float64) + 1j * z[f"{name}/{int(det)}/im"], det,
                     " AFX_NO_FUSED")


# ---- refusals that stay refusals ----------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C

    import torch

    import audioflux_amd as af
    lib = af.get_lib()
    fn = lib.afx_cwt_create_custom
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
    fre, bins, bank = np.ones(2, np.float32), np.ones(2, np.int32), np.ones((2, 2048), np.float32)
    F, B, K = fre.ctypes.data, bins.ctypes.data, bank.ctypes.data
    # the arguments cwt_create would copy from or size by: a NULL bank (it would fall through to the analytic bank of a zeroed
    # parameter set), NULL band arrays, no scale, a chunk exponent outside 1 ... 30 -- AFX_ERR_ARG and no object
    for what, args in (("NULL bank", (2, 10, None, F, B)), ("NULL fre", (2, 10, K, None, B)), ("NULL bin", (2, 10, K, F, None)),
                       ("num 0", (0, 10, K, F, B)), ("radix2Exp 0", (2, 0, K, F, B)), ("radix2Exp 31", (2, 31, K, F, B))):
        h = C.c_void_p(0xdead)
        st = fn(C.byref(h), args[0], args[1], 32000, 1, args[2], args[3], args[4], b"test")
        assert st == cc.ERR_ARG and not h.value, f"{what}: status {st}"
    assert fn(None, 2, 10, 32000, 1, K, F, B, b"test") == cc.ERR_ARG
    # 2^17 samples cannot be padded (the transform would leave powers of two)
    with pytest.raises(RuntimeError):
        af.CWT(num=4, radix2_exp=17, is_padding=True)
    # more chunks than a launch grid's y / z extent.  The launchers are called bare, with NULL pointers: each checks `chunks`
    # before it reads anything but r1 / r2 of the dims (afxk_cwt_small, afxk_cwt_forward, afxk_cwt_inverse in afx_cwt.hip: the
    # `chunks > 65535` line is the first or second statement), so nothing is launched.  The objects never get there: they hand
    # the launchers at most 4096 chunks at a time.  `dims`: zeroed memory larger than any AfxCwtPlanDims (about 100 bytes)
    dims = (C.c_char * 512)()
    UNSUPPORTED = cc.ERR_UNSUPPORTED
    lib.afxk_cwt_small.restype = lib.afxk_cwt_forward.restype = lib.afxk_cwt_inverse.restype = C.c_int
    P, LL, I = C.c_void_p, C.c_longlong, C.c_int
    lib.afxk_cwt_small.argtypes = [P, P, P, LL, I, P, I, I, P, P, P, P]
    lib.afxk_cwt_forward.argtypes = [P, P, P, LL, I, P, P, P]
    lib.afxk_cwt_inverse.argtypes = [P, P, P, P, I, I, I, P, P, P, I, P]
    for chunks, want in ((65536, UNSUPPORTED), (0, 0)):
        assert lib.afxk_cwt_small(dims, None, None, 0, chunks, None, 2, 0, None, None, None, None) == want
        assert lib.afxk_cwt_forward(dims, None, None, 0, chunks, None, None, None) == want
        assert lib.afxk_cwt_inverse(dims, None, None, None, 2, 0, chunks, None, None, None, 3, None) == want
    torch.cuda.synchronize()
    assert af.runtime_status() == 0
