#!/usr/bin/env python3
"""Writes tests/golden/spectral.npz: every spectral descriptor of the compiled reference (oracle.ref.lib()) -- default and
one non-default parameter set each (tests/spectral_cases.py) -- on four committed inputs under three edges.  Only the [T]
output vectors are stored; the inputs are referenced by key.  Key: <input>/<edge>/<case>[/fre for the second output].

    python tests/golden/make_spectral_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref  # noqa: E402
from tests import spectral_cases as sc  # noqa: E402
from tests.spectral_ref import RefSpectral  # noqa: E402


def main():
    lib = ref.lib()
    out = {}
    for iname, (spec, phase, fre) in sc.inputs().items():
        num = spec.shape[1]
        for ename, edge in sc.edges(num).items():
            r = RefSpectral(lib, num, fre, edge)
            for case in sc.names_for(phase):
                kind, iarg, farg = sc.PARAMS[case]
                outs = r.run(kind, iarg, farg, spec, phase)
                out[f"{iname}/{ename}/{case}"] = outs[0]
                if len(outs) == 2:
                    out[f"{iname}/{ename}/{case}/fre"] = outs[1]
    path = os.path.join(ROOT, "tests", "golden", "spectral.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} vectors -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
