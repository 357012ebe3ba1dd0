"""CPU-only: the device-pointer contract of include/afx_batch.h (tests/device_contract.py) against DEVICE code compiled for
the host with -fsanitize=address,undefined: afx_hpss.hip, afx_istft.hip, afx_pitch_yin.hip and afx_descriptors.hip (tests/emu),
linked with the C host objects and the generated stand-in for the rest of the device layer.  Every caller's buffer is
malloc'ed at exactly its size, so this is where over-READS are shown absent (on the GPU they can only be shown not to reach
the result) and where a kernel that assumes an alignment it never checks is found before any GPU time is spent.  Also: the
registry against the header, and the arena's own checks."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
INC = [f"-I{ROOT}/include", f"-I{ROOT}/audioflux_amd/csrc/hip", f"-I{ROOT}/audioflux_amd/csrc/host"]
SAN = ["-DAFX_EMU_VECTOR_TYPES", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-shared-libsan"]
UNITS = ("emu_engine", "hpss_emulated", "istft_emulated", "pitch_emulated", "descriptors_emulated")
OMIT = ("afxk_hpss_mask", "afxk_median_filter", "afxk_pitch_yin", "afxk_descriptors", "afxk_desc_preprocess")


def _asan_runtime():
    if not os.path.exists(CLANG):
        return None
    p = subprocess.run([CLANG, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(p) and os.path.exists(p):
        return p
    d = subprocess.run([CLANG, "-print-resource-dir"], capture_output=True, text=True).stdout.strip()
    p = os.path.join(d, "lib", "linux", "libclang_rt.asan-x86_64.so")
    return p if os.path.exists(p) else None


needs_clang = pytest.mark.skipif(_asan_runtime() is None, reason="needs clang with the shared AddressSanitizer runtime")


def test_registry_covers_every_device_entry_point():
    """a new *Device prototype in afx_batch.h without a registry row fails here"""
    from tests import device_contract as dc
    header = dc.header_device_entry_points()
    assert len(header) >= 23 and dc.NOT_COVERED <= header, sorted(header)
    table = {r.entry for r in dc.ROWS}
    assert table == header - dc.NOT_COVERED, sorted(table ^ (header - dc.NOT_COVERED))
    assert set(dc._SIG) == table
    assert len({str(r) for r in dc.ROWS}) == len(dc.ROWS) and all(r.doc for r in dc.ROWS)


def test_arena_sees_what_it_is_meant_to_see():
    """the arena itself, on host memory: a stray store in a guard, in the row-pitch padding, a missing store"""
    from tests import device_contract as dc
    a = dc.Arena("numpy", 3 * 10 + 7, offset=3)
    assert a.ptr() % 256 == 12 and a.guards_intact()
    m = dc.Arena.mask(3, 7, 10, a.words)
    assert m.sum() == 21 and a.unwritten(m) and a.unwritten(~m) and not a.written(m)
    pay = np.full(a.words, dc.SENTINEL, np.uint32)
    pay[m] = np.float32(1.5).view(np.uint32)
    a.write(pay)
    assert a.written(m) and a.unwritten(~m) and a.guards_intact()
    pay[7] = 0                      # one word of padding
    a.write(pay)
    assert not a.unwritten(~m)
    pay[7], pay[12] = dc.SENTINEL, dc.SENTINEL      # one promised word missing
    a.write(pay)
    assert a.unwritten(~m) and not a.written(m)
    np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint32 * 1).from_address(a.ptr(a.words)))[0] = 0   # one word behind the payload
    assert not a.guards_intact()
    # the sentinel is a NaN: as a float it never compares equal, hence the integer comparisons
    assert np.isnan(np.array([dc.SENTINEL], np.uint32).view(np.float32)[0])


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("emu_contract"))
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hoststub", "gen_stub.py"),
                    os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"), stub, *[f"--omit={n}" for n in OMIT]],
                   check=True)
    # (the stand-in's own forward / inverse STFT launchers step aside for the ones that compute)
    renames = [f"-D{n}=standin_{n}" for n in ("afxk_stft", "afxk_istft", "afxk_istft_fused")]
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [[CLANG, "-std=c99", "-O1", "-g", "-fPIC", "-ffp-contract=off", *SAN, *INC, "-c", os.path.join(hostdir, f), "-o",
             os.path.join(tmp, f[:-2] + "_c.o")] for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    jobs.append([CLANG, "-std=c99", "-O1", "-g", "-fPIC", *SAN, *INC, *renames, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for f in UNITS:
        jobs.append([CLANG + "++", "-std=c++17", "-O1", "-g", "-fPIC", *SAN, f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c",
                     os.path.join(EMU, f + ".cpp"), "-o", os.path.join(tmp, f + ".o")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    lib = os.path.join(tmp, "libafx_emulated_contract.so")
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    r = subprocess.run([CLANG + "++", "-shared", *SAN, *objs, "-lm", "-lpthread", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def _run(lib, args, env_rows=False):
    preload = " ".join(p for p in (_asan_runtime(), os.environ.get("LD_PRELOAD")) if p)  # (the sanitizer runtime goes first)
    e = dict(os.environ, AFX_LIB=lib, AFX_QUIET="1", AFX_HIP_RUNTIME="system", LD_PRELOAD=preload,
             ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("AFX_HPSS_CHUNK_MB", "AFX_CONTRACT_ENV_ROWS"):
        e.pop(k, None)
    if env_rows:
        e["AFX_CONTRACT_ENV_ROWS"] = "1"
    r = subprocess.run([sys.executable, os.path.join(EMU, "emulated_contract.py"), *args], capture_output=True, text=True, env=e,
                       timeout=1700)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert r.returncode == 0 and "\nOK" in r.stdout, out[-4000:]
    return r.stdout


ENTRIES = ("afx_medianFilterDevice", "hpssObj_hpssBatchDevice", "hpssObj_spectraBatchDevice", "stftObj_istftBatchDevice",
           "pitchYINObj_pitchBatchDevice", "pitchYINObj_troughsBatchDevice", "pitchYINObj_curveBatchDevice",
           "spectralObj_computeDevice")


@needs_clang
@pytest.mark.parametrize("entry", ENTRIES)
def test_contract_on_sanitized_emulated_kernels(emulated, entry):
    """extent, poisoned surroundings (NaN), two misalignments, history and the value anchor of every row of `entry`, buffers
    allocated at exactly their size: no AddressSanitizer / UBSan report from device code, every check of tests/device_contract.py holds"""
    from tests import device_contract as dc
    want = [r for r in dc.rows(emulated=True) if r.entry == entry]
    assert want, entry
    out = _run(emulated, [entry])
    assert sum(line.startswith("contract ") for line in out.splitlines()) == len(want), out[-2000:]


@needs_clang
def test_contract_rows_with_their_own_environment(emulated):
    """AFX_HPSS_CHUNK_MB=1: the chunked scratch of hpssObj_*"""
    from tests import device_contract as dc
    want = dc.rows(emulated=True, env=True)
    out = _run(emulated, [], env_rows=True)
    assert want and sum(line.startswith("contract ") for line in out.splitlines()) == len(want), out[-2000:]


def test_every_emulated_entry_is_run():
    from tests import device_contract as dc
    assert {r.entry for r in dc.rows(emulated=True)} == set(ENTRIES)
