"""The reference's own unmodified `audioflux.Onset` wrapper (python/audioflux/mir/onset.py) and `audioflux.utils.power_to_db`
(python/audioflux/utils/convert.py) on one library, in a FRESH interpreter: staged as tests/dropin/flows.py stages the
wrapper.  The Onset docstring flow -- BFT (mel, power) -> power_to_db -> Onset(FLUX).onset with NoveltyParam(1, 2, 0, 1, 0, 0,
0, 1) -- on a synthetic signal of decaying tones; power_to_db on two channels as well.  (Onset.onset on more than one channel
ends in a ValueError inside the reference wrapper itself, mir/onset.py:205, on either library: it is not part of the flow.)

usage: python flows_onset.py WORKDIR OUT.npz stock|mi355x|cpu
  stock / mi355x: run the flow on that library, write the results
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

SR, HOP = 32000, 2048


def signal():
    rng = np.random.default_rng(11)
    n = SR * 4
    x = 0.003 * rng.standard_normal(n)
    for t0 in rng.integers(4000, n - 16000, 10):
        k = np.arange(12000)
        x[t0:t0 + 12000] += np.sin(2 * np.pi * rng.uniform(150, 4000) * k / SR) * np.exp(-k / 2500.0) * rng.uniform(0.2, 1.0)
    return x.astype(np.float32)


def symbols(workdir):
    names = set()
    for rel, pat in (("mir/onset.py", r"_lib\['([A-Za-z0-9_]+)'\]"), ("utils/convert.py", r"get_fft_lib\(\)\['(util_powerToDB)'\]")):
        with open(os.path.join(workdir, "audioflux", rel)) as f:
            names.update(re.findall(pat, f.read()))
    return sorted(names)


def run(workdir, out, tag):
    flows.stage(workdir)
    af = flows.import_wrapper(workdir)
    af.fftlib.set_fft_lib(lib_ext=None if tag == "stock" else "mi355x")
    from audioflux.type import NoveltyType, SpectralDataType, SpectralFilterBankScaleType
    x = signal()
    res, meta = {}, {"lib": os.path.realpath(af.fftlib.get_fft_lib_fp())}
    bft_obj = af.BFT(num=128, samplate=SR, radix2_exp=12, slide_length=HOP, scale_type=SpectralFilterBankScaleType.MEL,
                     data_type=SpectralDataType.POWER)
    spec_arr = bft_obj.bft(x)
    spec_db = af.utils.power_to_db(np.abs(spec_arr))
    n_fre, n_time = spec_db.shape
    onset_obj = af.Onset(time_length=n_time, fre_length=n_fre, slide_length=bft_obj.slide_length, samplate=bft_obj.samplate,
                         novelty_type=NoveltyType.FLUX)
    params = af.NoveltyParam(1, 2, 0, 1, 0, 0, 0, 1)
    res["power"], res["db"] = np.abs(spec_arr), spec_db
    res["point"], res["evn"], res["time"], res["value"] = onset_obj.onset(spec_db, novelty_param=params)
    res["db2"] = af.utils.power_to_db(np.stack([np.abs(spec_arr), 2 * np.abs(spec_arr)]))
    res["point_default"], res["evn_default"], _, _ = onset_obj.onset(spec_db)  # the wrapper's own default parameters
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
