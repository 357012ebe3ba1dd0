"""CPU-only: the packed band plan of the headline kernel (afx_bandplan.c: afx_bandpack_build; afx_melparts.h: band_stage3) through
the emulation of tests/test_emulated_kernels.py -- the plan layer re-packs mel-128 at n_fft 2048 into 48 tap slots per lane, and
every result keeps its bits: a row's multiply-adds are the same, in the same order, whichever partitions of a lane hold it."""
from tests.test_emulated_kernels import _run, emulated, pytestmark  # noqa: F401  (the emulated library: a module-scoped fixture)


def test_packed_plan_emulated_equals_the_unpacked_plan(emulated):
    """3 clips x 37 frames at hop 512 (runs of four frames, the cepstrum block's tail form): mel-128 + MFCC-13, complex results and
    the temporal instantiation, packed against AFX_MEL_NOPACK=1, bit for bit, on one CU's claimed runs and on the whole device;
    3 clips x 301 frames on one CU (runs of 32 and 16 frames: whole 16-row cepstrum blocks between the band stage and the row
    stores, then the tail); a flipped continuation flag is caught"""
    out = _run(emulated, "mel_pack_emulated_case.py", [])
    assert out.count("packed equals unpacked") == 7 and "16-row blocks: 903 frames in one workgroup" in out and "is caught" in out, out[-1500:]
