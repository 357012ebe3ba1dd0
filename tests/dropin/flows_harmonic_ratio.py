"""The reference's own unmodified `audioflux.HarmonicRatio` wrapper (python/audioflux/mir/harmonic_ratio.py) on one library, in
a FRESH interpreter: staged as tests/dropin/flows.py stages the wrapper.  The docstring flow -- the constructor at the
wrapper's default size, cal_time_length, harmonic_ratio -- on the input of the fixture case r12_default
(tests/harmonic_ratio_cases.py), once as one channel and once as two channels of it.

usage: python flows_harmonic_ratio.py WORKDIR OUT.npz stock|mi355x|cpu
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


def symbols(workdir):
    with open(os.path.join(workdir, "audioflux", "mir", "harmonic_ratio.py")) as f:
        return sorted(set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read())))


def run(workdir, out, tag):
    from tests import harmonic_ratio_cases as hc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    x = hc.case_input(CASE)
    c = hc.CASES[CASE]
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    o = af.HarmonicRatio(samplate=c[0], low_fre=c[1], radix2_exp=c[2], slide_length=c[3])
    res["frames"] = np.array(o.cal_time_length(len(x)))
    res["value"] = o.harmonic_ratio(x)
    res["value2"] = o.harmonic_ratio(np.stack([x, x[::-1].copy()]))
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
