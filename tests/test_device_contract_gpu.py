"""The device-pointer contract of include/afx_batch.h on the GPU: every row of the registry in tests/device_contract.py --
every entry point that takes device pointers, in enough configurations to reach every launcher behind it -- through
sentinel-filled arenas with 1 MiB guards (a stray access is observed as data, never becomes a fault):

  extent     guards and every word outside the documented extent untouched, every promised word written, payload bit-equal
             to the baseline call; read-modify-write outputs keep the held + result relation
  poison     NaN / +Inf / 3e38 in every input word outside [b * stride, b * stride + length): outputs bit-equal to the baseline
  alignment  input at word offsets 1, 2, 3 and output at word offsets 1, 2 from a 256-byte boundary, even and odd strides
  history    after a bigger, longer, 100 x louder call on the same object, and growing after a small one: bit-equal to a
             fresh object
  anchor     the baseline against the float64 restatement (or the one-clip host call) at the bar of the entry point's own tests

Scatter outputs (wsst, reassign: float atomics, no fixed order of the additions) are compared by the fraction-of-cells rule of
their own test files instead of bit for bit; the extent and poison checks apply to them unchanged.  Across alignments xxcc, the
inverse STFT and the descriptors on rows of a multiple of 4 bins run another instantiation (named in their rows) and compare
at the entry point's parity bar; every other row is bit for bit.  Rows that need
their own environment (AFX_CQT_PYRAMID=0, AFX_HPSS_CHUNK_MB) run in a child process."""
import os
import subprocess
import sys

import pytest

from tests import device_contract as dc
from tests.conftest import EMULATED, HOSTSTUB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _backend():
    """(backend, stream, sync): device memory through torch; host memory where the library's device layer is a host stand-in"""
    if HOSTSTUB or EMULATED:
        return "numpy", None, None
    import torch
    return "torch", torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize


@pytest.mark.parametrize("row", dc.rows(env=False), ids=str)
def test_contract(row):
    backend, stream, sync = _backend()
    dc.check_row(row, backend, stream, sync)


@pytest.mark.parametrize("row", dc.rows(env=True), ids=str)
def test_contract_in_its_own_environment(row):
    """the row's switches are read once per process: a child process with them set"""
    e = dict(os.environ, **row.env)
    code = ("import sys; sys.path.insert(0, %r)\nfrom tests import device_contract as dc\nfrom tests.test_device_contract_gpu import _backend\n"
            "r = [r for r in dc.rows(env=True) if str(r) == %r][0]\ndc.check_row(r, *_backend())\nprint('CONTRACT OK')" % (ROOT, str(row)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "CONTRACT OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
