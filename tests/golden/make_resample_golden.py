#!/usr/bin/env python3
"""Writes tests/golden/resample.npz: the compiled reference's outputs (oracle/_ref/libaudioflux_ref.so, `make -C oracle`) of
every case of tests/resample_cases.py -- all values, or for the LONG cases the selection of resample_cases.selection and the
length -- and of the streamed pieces and the ratio sequence.  Inputs are not stored: resample_cases.signal restates them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resample_cases as rc  # noqa: E402


def main():
    ref = rc.ref_lib()
    assert ref is not None, "needs oracle/_ref/libaudioflux_ref.so"
    out = {}
    for name in rc.CASES:
        y = rc.run_case(ref, name)
        if name in rc.LONG:
            out[name + "/len"] = np.int64(len(y))
            out[name + "/sel"] = y[rc.selection(len(y))]
        else:
            out[name + "/out"] = y
    for k, y in enumerate(rc.run_pieces(ref)):
        out[f"pieces/{k}"] = y
    for k, y in enumerate(rc.run_sequence(ref)):
        out[f"sequence/{k}"] = y
    path = os.path.join(rc.GOLDEN, "resample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
