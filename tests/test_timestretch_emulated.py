"""CPU-only: the DEVICE code of audioflux_amd/csrc/hip/afx_phasevocoder.hip compiled for the host (tests/emu/hip/hip_runtime.h:
one thread per lane), linked with the C host objects and the generated stand-in for the rest of the device layer
(tests/emu/emulated_timestretch.py): afx_phase_vocoder_device on the reference's own STFT of the n_fft 128 and 256 cases of
tests/timestretch_cases.py against the reference's phase_vocoder at the recorded bars, exact conjugate mirrors, two clips in
one call, refusals, the plan's k / alpha table.  No sanitizer is involved."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
INC = [f"-I{ROOT}/include", f"-I{ROOT}/audioflux_amd/csrc/hip", f"-I{ROOT}/audioflux_amd/csrc/host"]

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang")


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("emu_timestretch"))
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hoststub", "gen_stub.py"),
                    os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"), stub, "--omit=afxk_phase_vocoder",
                    "--omit=afxk_rows_fit"], check=True)
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [["gcc", "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", *INC, "-c", os.path.join(hostdir, f), "-o",
             os.path.join(tmp, f[:-2] + "_c.o")] for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    jobs.append(["gcc", "-std=c99", "-O2", "-fPIC", *INC, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for f in ("emu_engine", "phasevocoder_emulated"):
        jobs.append([CLANG + "++", "-std=c++17", "-O2", "-g", "-fPIC", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c",
                     os.path.join(EMU, f + ".cpp"), "-o", os.path.join(tmp, f + ".o")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    lib = os.path.join(tmp, "libafx_emulated_timestretch.so")
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    r = subprocess.run([CLANG + "++", "-shared", *objs, "-lm", "-lpthread", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def _run(lib, *what):
    e = dict(os.environ, AFX_LIB=lib, AFX_QUIET="1")
    r = subprocess.run([sys.executable, os.path.join(EMU, "emulated_timestretch.py"), *what], capture_output=True, text=True, env=e,
                       timeout=1500)
    assert r.returncode == 0 and "\nOK" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_vocoder_kernels_emulated_meet_the_reference(emulated):
    """k_pv_polar / k_pv_phase / k_pv_synthesis through afx_phase_vocoder_device: every case of timestretch_cases.SMALL"""
    from tests import timestretch_cases as tc
    out = _run(emulated, *tc.SMALL)
    assert sum(line.startswith("vocoder ") for line in out.splitlines()) == len(tc.SMALL), out[-2000:]


def test_vocoder_refusals_and_plan_table_emulated(emulated):
    out = _run(emulated, "extras")
    assert "refusals" in out and "k / alpha table" in out
