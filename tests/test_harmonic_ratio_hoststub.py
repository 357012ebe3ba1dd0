"""CPU-only: tests/hoststub/driver_harmonic_ratio.c -- the harmonic-ratio host object (construction and free, the plans and
their LDS budget, refusals, a NULL object and a NULL output, fewer samples than a window, repeated calls of different lengths
through the staging buffers and the scratch, the batch guards and optional outputs) as a stand-alone program under
AddressSanitizer + UBSan against the generated stand-in of the device layer, with a launcher that touches every table entry,
sample, scratch word and output the kernels would.  Built and run as a program, like tests/test_pitch_lag_hoststub.py."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hoststub")
INC = [f"-I{ROOT}/include", f"-I{ROOT}/audioflux_amd/csrc/hip", f"-I{ROOT}/audioflux_amd/csrc/host"]
SAN = ["-std=c99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off"]


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


pytestmark = pytest.mark.skipif(shutil.which("gcc") is None or _asan_runtime() is None,
                                reason="needs gcc with the AddressSanitizer runtime")


def test_harmonic_ratio_host_object_is_clean_under_sanitizers(tmp_path):
    tmp = str(tmp_path)
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(HERE, "gen_stub.py"), os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"),
                    stub, "--omit=afxk_harmonic_ratio"], check=True)
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    host = sorted(os.path.join(hostdir, f) for f in os.listdir(hostdir) if f.endswith(".c"))
    exe = os.path.join(tmp, "driver_harmonic_ratio")
    r = subprocess.run(["gcc", *SAN, *INC, *host, stub, os.path.join(HERE, "driver_harmonic_ratio.c"), "-lm", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "\nOK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out and "LeakSanitizer" not in out, out[-3000:]
    assert sum(line.startswith("harmonic_ratio ") for line in r.stdout.splitlines()) == 3, out[-3000:]
