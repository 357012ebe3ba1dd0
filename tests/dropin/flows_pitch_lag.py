"""The reference's own unmodified `audioflux.PitchNCF` / `audioflux.PitchCEP` wrappers (python/audioflux/mir/pitch_ncf.py,
pitch_cep.py) on one library, in a FRESH interpreter: staged as tests/dropin/flows.py stages the wrapper.  The docstring
flow -- the default constructor at 32 kHz, cal_time_length, pitch -- on the input of the fixture case r12_default
(tests/pitch_lag_cases.py), once as one channel and once as two channels of it.

usage: python flows_pitch_lag.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flows on that library, write the results
  cpu: no device -- select the product library and resolve every symbol the modules look up"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402
sys.path.insert(0, flows.ROOT)

CASE = "r12_default"
KINDS = ("NCF", "CEP")


def symbols(workdir):
    names = set()
    for kind in KINDS:
        with open(os.path.join(workdir, "audioflux", "mir", f"pitch_{kind.lower()}.py")) as f:
            names |= set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read()))
    return sorted(names)


def run(workdir, out, tag):
    from tests import pitch_lag_cases as pc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    x = pc.case_input(CASE)
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    for kind in KINDS:
        o = getattr(af, "Pitch" + kind)(samplate=32000)
        res[kind + "/frames"] = np.array(o.cal_time_length(len(x)))
        res[kind + "/fre"] = o.pitch(x)
        res[kind + "/fre2"] = o.pitch(np.stack([x, x[::-1].copy()]))
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
