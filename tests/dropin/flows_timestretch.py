"""The reference's own unmodified `audioflux.TimeStretch` / `audioflux.PitchShift` wrappers
(python/audioflux/mir/time_stretch.py, pitch_shift.py) on one library, in a FRESH interpreter: staged as tests/dropin/flows.py
stages the wrapper.  The docstring flows -- constructor, time_stretch(x, rate) / pitch_shift(x, n_semitone, samplate) -- at
n_fft 256, hop 64 on the input of timestretch_cases.DROPIN_CASE, once as one channel and once as two
channels (the second: the input reversed).

usage: python flows_timestretch.py WORKDIR OUT.npz stock|mi355x|cpu
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


def symbols(workdir):
    names = set()
    for mod in ("time_stretch.py", "pitch_shift.py"):
        with open(os.path.join(workdir, "audioflux", "mir", mod)) as f:
            names |= set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read()))
    return sorted(names)


def run(workdir, out, tag):
    from tests import timestretch_cases as tc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    from audioflux.type import WindowType
    x = tc.case_input(tc.DROPIN_CASE)
    two = np.stack([x, x[::-1].copy()])
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    ts = af.TimeStretch(radix2_exp=8, window_type=WindowType.HANN, slide_length=64)
    for name, rate in tc.DROPIN_STRETCH.items():
        res[name + "/one"] = ts.time_stretch(x, rate)
        res[name + "/two"] = ts.time_stretch(two, rate)
    ps = af.PitchShift(radix2_exp=8, slide_length=64, window_type=WindowType.HANN)
    for name, semi in tc.DROPIN_SHIFT.items():
        res[name + "/one"] = ps.pitch_shift(x, n_semitone=semi, samplate=32000)
        res[name + "/two"] = ps.pitch_shift(two, n_semitone=semi, samplate=32000)
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
