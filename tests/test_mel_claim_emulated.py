"""CPU-only: the claim path of the headline kernel (afx_melfused2.hip: the waves of a workgroup claim runs of frames from a
counter in LDS) through the emulation of tests/test_emulated_kernels.py -- the kernel's fetch-add is the host's
__atomic_fetch_add there, lanes are threads, workgroups run one after the other.  AFX_MEL_CUS=1 sizes the grid for one CU."""
import os

from tests.test_emulated_kernels import ROOT, _run, emulated, pytestmark  # noqa: F401  (the emulated library: a module-scoped fixture)


def test_claimed_runs_emulated_equal_per_clip_calls(emulated):
    """3 clips x 301 frames, mel-128 + MFCC-13: one workgroup's claimed runs against the same clips one per call, bit for bit"""
    out = _run(emulated, os.path.join(ROOT, "tests", "mel_claim_emulated_case.py"), [], env="AFX_MEL_CUS=1")
    assert "equal the per-clip calls" in out, out[-800:]
