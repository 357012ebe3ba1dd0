"""The reference's own unmodified `audioflux.Resample` / `audioflux.WindowResample` wrappers
(python/audioflux/dsp/resample.py) on one library, in a FRESH interpreter: staged as tests/dropin/flows.py stages the
wrapper.  The docstring flow -- constructor, set_samplate, resample -- at Best and Fast 44100 -> 16000, a default
WindowResample 48000 -> 16000 and a scaled up-sampling, on the input of the case 441_16_best (tests/resample_cases.py), once
as one channel and once as two channels.

usage: python flows_resample.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flows on that library, write the results
  cpu: no device -- select the product library and resolve every symbol the module looks up"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402
sys.path.insert(0, flows.ROOT)

CASE = "441_16_best"


def symbols(workdir):
    with open(os.path.join(workdir, "audioflux", "dsp", "resample.py")) as f:
        return sorted(set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read())))


def run(workdir, out, tag):
    from tests import resample_cases as rc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    from audioflux.type import ResampleQualityType
    x = rc.case_input(CASE)
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    for name, o, rates in (("best", af.Resample(qual_type=ResampleQualityType.BEST, is_scale=False), (44100, 16000)),
                           ("fast", af.Resample(qual_type="fast"), (44100, 16000)),
                           ("window", af.WindowResample(), (48000, 16000)),
                           ("up_scaled", af.Resample(qual_type=ResampleQualityType.MID, is_scale=True), (16000, 44100))):
        o.set_samplate(*rates)
        res[name + "/one"] = o.resample(x)
        res[name + "/two"] = o.resample(np.stack([x, x[::-1].copy()]))
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
