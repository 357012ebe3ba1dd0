"""The reference's own unmodified `audioflux.PitchHPS` / `audioflux.PitchLHS` wrappers (python/audioflux/mir/pitch_hps.py,
pitch_lhs.py) on one library, in a FRESH interpreter: staged as tests/dropin/flows.py stages the wrapper.  The docstring
flow of each class -- the default constructor at 32 kHz, cal_time_length, pitch -- on the input of the fixture case
d8_default_r12 (tests/pitch_hs_cases.py), once as one channel and once as two channels of it.

usage: python flows_pitch_hs.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flows on that library, write the results
  cpu: no device -- select the product library and resolve every symbol the two modules look up"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402
sys.path.insert(0, flows.ROOT)

CASE = "d8_default_r12"


def symbols(workdir):
    names = set()
    for mod in ("pitch_hps.py", "pitch_lhs.py"):
        with open(os.path.join(workdir, "audioflux", "mir", mod)) as f:
            names.update(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read()))
    return sorted(names)


def run(workdir, out, tag):
    from tests import pitch_hs_cases as hc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    x = hc.case_input(CASE)
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    for name, cls in (("HPS", af.PitchHPS), ("LHS", af.PitchLHS)):
        o = cls(samplate=32000)
        res[f"{name}/frames"] = np.array(o.cal_time_length(len(x)))
        res[f"{name}/fre"] = o.pitch(x)
        res[f"{name}/fre2"] = o.pitch(np.stack([x, x[::-1].copy()]))
    np.savez(out, meta=json.dumps(meta), **res)


def run_cpu(workdir, out):
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext="mi355x")
    lib = af.fftlib.get_fft_lib()
    names = symbols(workdir)
    missing = []
    for n in names:
        try:
            lib[n]
        except AttributeError:
            missing.append(n)
    np.savez(out, meta=json.dumps({"lib": os.path.realpath(af.fftlib.get_fft_lib_fp()), "symbols": names, "missing": missing}))


if __name__ == "__main__":
    if sys.argv[3] == "cpu":
        run_cpu(sys.argv[1], sys.argv[2])
    else:
        run(sys.argv[1], sys.argv[2], sys.argv[3])
