"""The reference's own unmodified `audioflux.NSGT` wrapper (python/audioflux/nsgt.py) on one library, in a FRESH interpreter:
staged as tests/dropin/flows.py stages the wrapper.  The docstring flow of the class on two configurations:
  oct84  -- num 84, radix2_exp 15, 32 kHz, octave scale from C1, on the `tone` input of tests/nsgt_cases.py;
  mel12  -- with set_min_length(5) BEFORE the first transform only (afterwards the reference reads stale time arrays).

usage: python flows_nsgt.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flows on that library, write the results
  cpu: no device -- select the product library and resolve every symbol nsgt.py looks up"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flows  # noqa: E402
sys.path.insert(0, flows.ROOT)


def nsgt_symbols(workdir):
    with open(os.path.join(workdir, "audioflux", "nsgt.py")) as f:
        return sorted(set(re.findall(r"_lib\['([A-Za-z0-9_]+)'\]", f.read())))


def docstring_flow(af, o, x):
    spec = o.nsgt(x)
    return {"spec": spec, "abs": np.abs(spec), "max": np.array(o.get_max_time_length()), "total": np.array(o.get_total_time_length()),
            "len": o.get_time_length_arr(), "fre": o.get_fre_band_arr(), "bin": o.get_bin_band_arr(),
            "x_coords": o.x_coords(x.shape[-1]), "y_coords": o.y_coords()}


def run(workdir, out, tag):
    from tests import nsgt_cases as nc
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    T = af.type
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    o = af.NSGT(num=84, radix2_exp=15, samplate=32000, bin_per_octave=12, scale_type=T.SpectralFilterBankScaleType.OCTAVE,
                style_type=T.SpectralFilterBankStyleType.SLANEY, normal_type=T.SpectralFilterBankNormalType.BAND_WIDTH)
    for k, v in docstring_flow(af, o, nc.inputs("oct84")[1]).items():
        res[f"oct84/{k}"] = np.asarray(v)
    o = af.NSGT(num=12, radix2_exp=9, samplate=16000, low_fre=0., scale_type=T.SpectralFilterBankScaleType.MEL,
                style_type=T.SpectralFilterBankStyleType.SLANEY, normal_type=T.SpectralFilterBankNormalType.BAND_WIDTH)
    o.set_min_length(5)
    for k, v in docstring_flow(af, o, nc.inputs("mel12")[1]).items():
        res[f"mel12/{k}"] = np.asarray(v)
    np.savez(out, meta=json.dumps(meta), **res)


def run_cpu(workdir, out):
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext="mi355x")
    lib = af.fftlib.get_fft_lib()
    names = nsgt_symbols(workdir)
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
