#!/usr/bin/env python3
"""afx_onset.hip and afx_descriptors.hip as emulated device code through the C host object: the small fixture cases
(tests/onset_cases.py: SMALL) by the rule of the GPU tests (tests/onset_check.py), and with "extras" the checks of
tests/onset_suite.py that the GPU runs too -- the filter and the picker against their restatements, ties, edge lengths, index
tables, batches, both sides of the picker's LDS bound, the dB map, refusals.
AFX_LIB = the library tests/test_onset_emulated.py builds.  Arguments: case names (default: SMALL) and / or "extras"."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import onset_cases as oc  # noqa: E402
from tests import onset_suite as suite  # noqa: E402

lib = oc.bind_device(C.CDLL(os.environ["AFX_LIB"]))
D = suite.NumpyDev


def main(argv):
    gold = np.load(os.path.join(oc.GOLDEN, "onset.npz"))
    names = [a for a in argv if a != "extras"] or (list(oc.SMALL) if not argv else [])
    for name in names:
        suite.fixture_case(lib, D, name, gold)
    if not argv or "extras" in argv:
        suite.max_filter(lib, D)
        suite.peak_pick(lib, D)
        suite.ties(lib, D)
        suite.edge_lengths(lib, D)
        suite.index_tables(lib, D)
        suite.unknown_kind(lib, D)
        suite.batches(lib, D)
        suite.lds_bound(lib, D)
        suite.envelope_is_normalised_descriptor(lib, D)
        suite.power_to_db(lib, D, gold)
        suite.refusals(lib, D)
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
