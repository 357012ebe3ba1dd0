"""CPU-only: the DEVICE code of audioflux_amd/csrc/hip/afx_harmonic_ratio.hip compiled for the host
(tests/emu/hip/hip_runtime.h: one thread per lane), linked with the C host objects and the generated stand-in for the rest of
the device layer (tests/emu/emulated_harmonic_ratio.py): the smallest fixture case of each class (N = 64, 256 and 512, frames
that inherit minIndex, an empty range, a clip without a crossing, silence) at the bars of the GPU tests, batches, a split
call, refusals.  No sanitizer is involved."""
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
    tmp = str(tmp_path_factory.mktemp("emu_harmonic_ratio"))
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hoststub", "gen_stub.py"),
                    os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"), stub, "--omit=afxk_harmonic_ratio"], check=True)
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [["gcc", "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", *INC, "-c", os.path.join(hostdir, f), "-o",
             os.path.join(tmp, f[:-2] + "_c.o")] for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    jobs.append(["gcc", "-std=c99", "-O2", "-fPIC", *INC, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for f in ("emu_engine", "harmonic_ratio_emulated"):
        jobs.append([CLANG + "++", "-std=c++17", "-O2", "-g", "-fPIC", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c",
                     os.path.join(EMU, f + ".cpp"), "-o", os.path.join(tmp, f + ".o")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    lib = os.path.join(tmp, "libafx_emulated_harmonic_ratio.so")
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    r = subprocess.run([CLANG + "++", "-shared", *objs, "-lm", "-lpthread", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def _run(lib, *what):
    e = dict(os.environ, AFX_LIB=lib, AFX_QUIET="1")
    r = subprocess.run([sys.executable, os.path.join(EMU, "emulated_harmonic_ratio.py"), *what], capture_output=True, text=True, env=e,
                       timeout=1500)
    assert r.returncode == 0 and "\nOK" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_harmonic_ratio_kernel_emulated_meets_the_reference_vectors(emulated):
    """k_harmonic_ratio (both passes) and k_harmonic_ratio_resolve through harmonicRatio / harmonicRatioBatchDevice / curveBatchDevice: every case of
    harmonic_ratio_cases.SMALL"""
    from tests import harmonic_ratio_cases as hc
    out = _run(emulated, *hc.SMALL)
    assert sum(line.startswith("harmonic_ratio ") for line in out.splitlines()) == len(hc.SMALL), out[-2000:]


def test_harmonic_ratio_batches_and_split_calls_emulated(emulated):
    out = _run(emulated, "extras")
    assert "bitwise the single calls" in out and "restarts from 0" in out
