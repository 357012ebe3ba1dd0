"""The reference's own unmodified `audioflux.FST` wrapper (python/audioflux/fst.py) on one library, in a FRESH interpreter:
staged as tests/dropin/flows.py stages the wrapper.  The docstring flow of the class on two configurations:
  doc     -- radix2_exp 12, min_index 1, max_index 1024, on the `tone` input of case r12doc of tests/fst_cases.py;
  default -- radix2_exp 9, the default range 1 ... 255, on the `tone` input of case r9default.

usage: python flows_fst.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flows on that library, write the results
  cpu: no device -- select the product library and resolve every symbol fst.py looks up"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402
sys.path.insert(0, flows.ROOT)


def fst_symbols(workdir):
    with open(os.path.join(workdir, "audioflux", "fst.py")) as f:
        return sorted(set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read())))


def docstring_flow(o, x):
    spec = o.fst(x)
    return {"spec": spec, "abs": np.abs(spec), "num": np.array(o.num), "fft_length": np.array(o.fft_length),
            "fre": o.get_fre_band_arr(), "x_coords": o.x_coords(), "y_coords": o.y_coords()}


def run(workdir, out, tag):
    from tests import fst_cases as fc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    o = af.FST(radix2_exp=12, min_index=1, max_index=1024, samplate=32000)
    for k, v in docstring_flow(o, fc.inputs("r12doc")[1]).items():
        res[f"doc/{k}"] = np.asarray(v)
    o = af.FST(radix2_exp=9)
    for k, v in docstring_flow(o, fc.inputs("r9default")[1]).items():
        res[f"default/{k}"] = np.asarray(v)
    np.savez(out, meta=json.dumps(meta), **res)


def run_cpu(workdir, out):
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext="mi355x")
    lib = af.fftlib.get_fft_lib()
    names = fst_symbols(workdir)
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
