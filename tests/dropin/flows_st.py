"""The reference's own unmodified `audioflux.ST` wrapper (python/audioflux/st.py) on one library, in a FRESH interpreter:
staged as tests/dropin/flows.py stages the wrapper.  Two configurations:
  doc     -- the docstring flow of the class: radix2_exp 12, min_index 1, max_index 1024, on the `tone` input of case r12doc
             of tests/st_cases.py;
  default -- radix2_exp 9, the default range 1 ... 255, on the `tone` input of case r9default: st, then set_value(2.5, 0.8)
             and st again, then use_bin_arr([3, 5, 9]) and st again.  That wrapper hands the list over as float32 words to
             the library's `int *`: 3.0 read as an int is 1077936128, so both libraries ignore the list and the rows stay
             1 ... 255.

usage: python flows_st.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flows on that library, write the results
  cpu: no device -- select the product library and resolve every symbol st.py looks up"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402
sys.path.insert(0, flows.ROOT)


def st_symbols(workdir):
    with open(os.path.join(workdir, "audioflux", "st.py")) as f:
        return sorted(set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read())))


def docstring_flow(o, x):
    spec = o.st(x)
    return {"spec": spec, "abs": np.abs(spec), "num": np.array(o.num), "fft_length": np.array(o.fft_length),
            "fre": o.get_fre_band_arr(), "x_coords": o.x_coords(), "y_coords": o.y_coords()}


def run(workdir, out, tag):
    from tests import st_cases as sc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    o = af.ST(radix2_exp=12, min_index=1, max_index=1024, samplate=32000)
    for k, v in docstring_flow(o, sc.inputs("r12doc")[1]).items():
        res[f"doc/{k}"] = np.asarray(v)
    o = af.ST(radix2_exp=9)
    x = sc.inputs("r9default")[1]
    for k, v in docstring_flow(o, x).items():
        res[f"default/{k}"] = np.asarray(v)
    o.set_value(2.5, 0.8)
    res["default/spec_set_value"] = o.st(x)
    o.use_bin_arr([3, 5, 9])
    res["default/spec_bin_arr"] = o.st(x)
    np.savez(out, meta=json.dumps(meta), **res)


def run_cpu(workdir, out):
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext="mi355x")
    lib = af.fftlib.get_fft_lib()
    names = st_symbols(workdir)
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
