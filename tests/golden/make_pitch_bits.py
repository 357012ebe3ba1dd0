#!/usr/bin/env python3
"""Writes tests/golden/pitch_bits.npz: what the pitch trackers of THIS build write on an MI355X for the seeded cases of
tests/test_pitch_bits_gpu.py, made by that test's own functions.  Run it once with the library of the commit BEFORE a change
that must not move a bit (AFX_LIB selects the library); the test then holds the changed library to these arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_pitch_bits_gpu as t  # noqa: E402


def main():
    import audioflux_amd as af
    lib, dev = t.bind(af.get_lib()), t.Torch()
    out = {}
    for family in (t.hs_outputs, t.pef_outputs, t.yin_outputs):
        out.update(family(lib, dev))
    np.savez_compressed(t.GOLDEN, **out)
    print(f"{t.GOLDEN}: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes, {os.path.getsize(t.GOLDEN)} on disk")


if __name__ == "__main__":
    main()
