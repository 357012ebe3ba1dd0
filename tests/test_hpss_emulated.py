"""CPU-only: the DEVICE code of audioflux_amd/csrc/hip/afx_hpss.hip compiled for the host (tests/emu/hip/hip_runtime.h: one
thread per lane), linked with the C host objects, the emulated inverse STFT, a float64 forward transform and the generated
stand-in for the rest of the device layer (tests/emu/emulated_hpss.py): the median primitive bitwise against numpy, the whole
hpssObj_hpss against tests/golden/hpss.npz at the bars of the GPU tests."""
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
    tmp = str(tmp_path_factory.mktemp("emu_hpss"))
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hoststub", "gen_stub.py"),
                    os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"), stub, "--omit=afxk_hpss_mask",
                    "--omit=afxk_median_filter"], check=True)
    # (the stand-in's own forward / inverse STFT launchers step aside for the ones that compute)
    renames = [f"-D{n}=standin_{n}" for n in ("afxk_stft", "afxk_istft", "afxk_istft_fused")]
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [["gcc", "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", *INC, "-c", os.path.join(hostdir, f), "-o",
             os.path.join(tmp, f[:-2] + "_c.o")] for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    jobs.append(["gcc", "-std=c99", "-O2", "-fPIC", *INC, *renames, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for f in ("emu_engine", "hpss_emulated", "istft_emulated"):
        jobs.append([CLANG + "++", "-std=c++17", "-O2", "-g", "-fPIC", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c",
                     os.path.join(EMU, f + ".cpp"), "-o", os.path.join(tmp, f + ".o")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    lib = os.path.join(tmp, "libafx_emulated_hpss.so")
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    r = subprocess.run([CLANG + "++", "-shared", *objs, "-lm", "-lpthread", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def _run(lib, what):
    e = dict(os.environ, AFX_LIB=lib, AFX_QUIET="1")
    e.pop("AFX_HPSS_CHUNK_MB", None)
    r = subprocess.run([sys.executable, os.path.join(EMU, "emulated_hpss.py"), what], capture_output=True, text=True, env=e,
                       timeout=1500)
    assert r.returncode == 0 and "\nOK" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_median_filter_kernels_emulated_are_bitwise_the_sorted_window(emulated):
    """k_hpss_tile<AXIS0 | AXIS1, K = 21 | 31 | 63> and k_median_rank: every odd order 1 ... 63 and 65 / 101 / 255, both axes, tile-edge and
    tiny planes, ties, clip boundaries, refusals"""
    out = _run(emulated, "median")
    assert sum(line.startswith("median") for line in out.splitlines()) == 4, out[-2000:]


def test_hpss_emulated_meets_the_reference_vectors(emulated):
    """every fixture case through hpssObj_hpss (k_hpss_tile<HPSS, 21, 31> and <HPSS, 63, 63>), order 1, batch == single calls and
    chunked == unchunked bitwise, the magnitude planes"""
    from tests import hpss_cases as hc
    out = _run(emulated, "hpss")
    assert sum(line.startswith("hpss ") for line in out.splitlines()) == len(hc.CASES) + 2, out[-2000:]
