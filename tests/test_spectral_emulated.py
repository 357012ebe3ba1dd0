"""CPU-only: the DEVICE code of audioflux_amd/csrc/hip/afx_descriptors.hip compiled for the host (tests/emu/hip/hip_runtime.h:
one thread per lane, DPP / ds_bpermute / shuffles as rendezvous), linked with the C host objects and the generated stand-in
for the rest of the device layer, against tests/golden/spectral.npz at the bars of the GPU tests
(tests/emu/emulated_descriptors.py)."""
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
    tmp = str(tmp_path_factory.mktemp("emu_desc"))
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hoststub", "gen_stub.py"),
                    os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"), stub,
                    "--omit=afxk_descriptors", "--omit=afxk_desc_preprocess"], check=True)
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [["gcc", "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", *INC, "-c", os.path.join(hostdir, f), "-o",
             os.path.join(tmp, f[:-2] + "_c.o")] for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    jobs.append(["gcc", "-std=c99", "-O2", "-fPIC", *INC, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for f in ("emu_engine", "descriptors_emulated"):
        jobs.append([CLANG + "++", "-std=c++17", "-O2", "-g", "-fPIC", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c",
                     os.path.join(EMU, f + ".cpp"), "-o", os.path.join(tmp, f + ".o")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    lib = os.path.join(tmp, "libafx_emulated_descriptors.so")
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    r = subprocess.run([CLANG + "++", "-shared", *objs, "-lm", "-lpthread", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def test_descriptor_kernels_emulated_meet_the_reference_vectors(emulated):
    """every fixture case (4 inputs x 3 edges x default / non-default parameters) through k_desc_rows<16 | 32 | 64, 4>,
    k_desc_rows_wide, k_desc_rows_long and k_desc_frames in their 16-byte, dword and index-table forms; request lists
    against single requests and clips against per-clip calls, bitwise"""
    e = dict(os.environ, AFX_LIB=emulated, AFX_QUIET="1")
    r = subprocess.run([sys.executable, os.path.join(EMU, "emulated_descriptors.py")], capture_output=True, text=True, env=e,
                       timeout=1500)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "\nOK" in r.stdout, out[-3000:]
    assert sum(line.startswith("descriptors ") for line in r.stdout.splitlines()) == 12, out[-2000:]
