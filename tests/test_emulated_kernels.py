"""CPU-only: DEVICE code of the wave kernels, compiled for the host and run one thread per lane (tests/emu).

tests/emu/hip/hip_runtime.h emulates the slice of HIP / gfx950 the f16 CQT kernels and the bf16 GEMM use -- the MFMA
operand / result layouts, DPP, readlane, raw buffer loads and stores with their bounds behaviour, LDS with the wave /
workgroup rendezvous -- and the kernels' .hip files are included unchanged: their hand-issued instruction sequences all
live in <afx_asm.h>, which resolves to tests/emu/hip/afx_asm.h (the same operations in C) in these builds and to
audioflux_amd/csrc/hip/afx_asm.h (inline assembly) in the product; afx_cqt.hip's two static LDS arrays become host statics.  The library under test is
the C host code + the real launchers of those files + their kernels, emulated: every launch of the CQT path.

  * the shipped kernels -- the headline k_stft_mel_v2 (BASELINE cfg 1: mel 1.8e-7, MFCC 2.0e-7 of the golden vectors, the
    device's own figures), k_cqt_decimate, k_cqt_octave_f16, k_cqt_chroma and the f32 matrix-core octave kernels, all
    measured and parity-tested on the MI355X -- reproduce the golden vectors here too: that calibrates the emulation;
  * k_cqt_chroma (host-built bin lists) and k_gemm_nt128_bf16x3 were written against this emulation at the end of round 2
    and passed their first device run in round 3 unchanged (profiles/r03_round_start.txt); they stay covered here;
  * the rest of the fused STFT family (n_fft 1024, 4096, 2048 complex) runs its golden cases the same way.

What this cannot show: timing, register pressure, the hardware's own accumulation order inside an MFMA.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
STUB = os.path.join(ROOT, "tests", "hoststub")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
INC = [f"-I{ROOT}/include", f"-I{ROOT}/audioflux_amd/csrc/hip", f"-I{ROOT}/audioflux_amd/csrc/host"]

STANDIN_RENAMES = [f"-D{n}=standin_{n}" for n in ("afxk_cwt_td_fits", "afxk_cwt_td", "afxk_cqt_deconv", "afxk_melfused_variant", "afxk_melfused_create", "afxk_melfused_run",
                                                     "afxk_melfused_destroy", "afxk_melfused_kind", "afxk_istft", "afxk_istft_fused")]

EMU_UNITS = ("emu_engine", "cqt_emulated_f16", "cwt_emulated_td", "gemm_emulated_bf16", "mel_emulated_v2", "mel_emulated_melfused",
             "mel_emulated_melfused1k", "mel_emulated_4k2", "mel_emulated_melfused512", "istft_emulated", "stft256_emulated")

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang (x86 _Float16 / __bf16 vectors)")


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    """C host objects + the launchers AND kernels of afx_cqt.hip, afx_cqt_f16.hip, afx_gemm_bf16.hip compiled
    for the host (every CQT launch is emulated device code) + the stand-in for the rest of the device layer"""
    import re
    from concurrent.futures import ThreadPoolExecutor
    tmp = str(tmp_path_factory.mktemp("emu"))
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(STUB, "gen_stub.py"), os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"),
                    stub, "--functional-cqt", "--omit=afxk_gemm_nt128_bf16", "--omit=afxk_gemm_bank_prepare", "--omit=afxk_gemm_nt_bank", "--omit=afxk_cqt_pyramid", "--omit=afxk_cqt_pyramid_plan"], check=True)
    # afx_cqt.hip keeps two arrays in static LDS: on the host, storage shared by the lanes' threads
    src = open(os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_cqt.hip")).read()
    patched, n = re.subn(r"(?m)^(\s*)__shared__ ", r"\1static ", src)
    assert n == 2, n
    with open(os.path.join(tmp, "afx_cqt_host.hip"), "w") as f:
        f.write(patched)
    with open(os.path.join(tmp, "cqt_emulated_main.cpp"), "w") as f:
        f.write('#include "hip/hip_runtime.h"\nnamespace {\nalignas(16) unsigned char smem_raw[160 * 1024];\n}\n'
                f'#include "{tmp}/afx_cqt_host.hip"\n')
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [["gcc", "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", *INC, "-c", os.path.join(hostdir, f), "-o",
             os.path.join(tmp, f[:-2] + "_c.o")] for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    # (the stand-in's own versions of the launchers that the emulated translation units bring step aside)
    jobs.append(["gcc", "-std=c99", "-O2", "-fPIC", "-ffp-contract=off", *STANDIN_RENAMES, *INC, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for f in EMU_UNITS:
        jobs.append([CLANG + "++", "-std=c++17", "-O2", "-g", "-fPIC", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c", os.path.join(EMU, f + ".cpp"), "-o",
                     os.path.join(tmp, f + ".o")])
    jobs.append([CLANG + "++", "-std=c++17", "-O2", "-g", "-fPIC", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c", os.path.join(tmp, "cqt_emulated_main.cpp"), "-o",
                 os.path.join(tmp, "cqt_emulated_main.o")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    lib = os.path.join(tmp, "libafx_emulated.so")
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    r = subprocess.run([CLANG + "++", "-shared", *objs, "-lm", "-lpthread", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def _run(lib, script, args, env=""):
    e = dict(os.environ)
    for k in ("AFX_CQT_CHUNK", "AFX_CQT_F32", "AFX_NO_FUSED", "AFX_CQT_PYRAMID", "AFX_CQT_PYR_TILES"):
        e.pop(k, None)
    if env:
        e.update(kv.split("=") for kv in env.split())
    e.update(AFX_LIB=lib, AFX_QUIET="1")
    r = subprocess.run([sys.executable, os.path.join(EMU, script), *args], capture_output=True, text=True, env=e, timeout=1500)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "\nOK" in r.stdout, out[-3000:]
    return r.stdout


def _launches(out):
    import re
    m = re.search(r"emulated octave_f16 (\d+);.*\n\s+emulated pyramid (\d+)\n\s+emulated decimate (\d+), chroma (\d+), chroma_scan (\d+), "
                  r"octave_mfma \(f32\) (\d+)", out)
    assert m, out[-2000:]
    return dict(zip(("octave_f16", "pyramid", "decimate", "chroma", "chroma_scan", "octave_f32"), map(int, m.groups())))


def test_shipped_cqt_kernels_emulated_meet_the_golden_vectors(emulated):
    """calibration: the kernels the device runs by default through the emulation.  The default ladder (84 bins) is ONE
    launch, k_cqt_pyramid: eight role-specialised waves per workgroup, the 2:1 resampler as a matrix-core product from
    the octave waves' own planes, level rings in memory behind one barrier per step, chroma-12 as partial sums through
    the output rows; 6 classes (six_min) go through k_cqt_chroma.  Runs of 3 tiles (AFX_CQT_PYR_TILES) make the 157
    frames of the golden clip cross run boundaries: same numbers."""
    for env in ("", "AFX_CQT_PYR_TILES=3"):
        n = _launches(_run(emulated, "emulated_cqt.py", ["c84_32k_area", "power_max", "mag_p2", "six_min"], env))
        assert n["pyramid"] == 4 and n["chroma"] == 1 and n["octave_f16"] + n["decimate"] + n["chroma_scan"] + n["octave_f32"] == 0, n


def test_pyramid_level_rings_emulated_against_the_float64_resampler(emulated):
    """the ladder's level signals themselves (never visible in an output): the rings of the first workgroup after a run
    that ends mid-clip (runs of three tiles) against restate.decimate2 in float64 -- 1e-6 of the level's peak; where six stages add up to more (levels
    3-6: 1.1e-6 ... 1.9e-6), not farther from float64 than the reference's own float32 resampler chain (1.2e-6 ... 2.2e-6).  The matrix-core resampler replaces src/dsp/resample_algorithm.c:430-521; tests/test_cqt_pyramid.py runs the
    same check on the device."""
    out = _run(emulated, "emulated_cqt_rings.py", [], "AFX_CQT_PYR_TILES=3")
    assert out.count("of the level's peak") == 6, out


def test_per_octave_cqt_kernels_emulated_meet_the_golden_vectors(emulated):
    """AFX_CQT_PYRAMID=0: the per-octave launches -- k_cqt_decimate, k_cqt_octave_f16 (all seven hop instantiations, the
    12-byte transposed stores), k_cqt_chroma (12 and 6 classes, max and min normalisation); what every plan outside the
    default ladder still runs"""
    n = _launches(_run(emulated, "emulated_cqt.py", ["c84_32k_area", "power_max", "six_min"], "AFX_CQT_PYRAMID=0"))
    assert n["octave_f16"] == 21 and n["decimate"] == 18 and n["chroma"] == 2 and n["pyramid"] + n["chroma_scan"] + n["octave_f32"] == 0, n


def test_streaming_cqt_through_the_emulated_octave_kernels(emulated):
    """isContinue = 1 objects frame from sample 0 (rightPad of AfxCqtOctaveArgs): pieces of a signal through
    k_cqt_octave_f16 / k_cqt_decimate on the CPU against the float64 restatement of the reference's tail rule"""
    _run(emulated, "emulated_cqt.py", ["stream"])


def test_headline_kernel_emulated_meets_the_golden_vectors(emulated):
    """k_stft_mel_v2 (afx_melfused2.hip; 624-654 M frames/s on the device): BASELINE cfg 1 -- golden mel spectrogram and
    MFCC-13 of the reference -- from ONE emulated launch (wave FFT, band plan, log10 + DCT-II on the f32 matrix cores),
    two clips with an odd row stride; mel alone equals mel beside the cepstra bit for bit.  On the device: 1.8e-7 /
    2.6e-7; here 1.8e-7 / 2.0e-7.  (This kernel's cross-lane LDS exchanges rely on a wave's DS operations executing in
    issue order: the emulation makes every DS read a rendezvous of the wave.)"""
    out = _run(emulated, "emulated_bft.py", [])
    assert "emulated k_stft_mel_v2 2" in out, out[-500:]


def test_fused_stft_kernels_emulated_meet_the_golden_vectors(emulated):
    """the other fused STFT -> filter-bank kernels, through the product's own dispatcher: n_fft 2048 complex results
    (k_stft_mel_v2<..., CPLX>), n_fft 1024 (k_stft_band_1k: mel-80 magnitudes with area normalisation, mel-64 with temporal
    features), n_fft 4096 (k_stft_band_4k2: 60 octave bands), and the ragged-tail clip on the headline kernel"""
    out = _run(emulated, "emulated_bft_cases.py", ["cfg1_mel_complex", "tones_mel_mag_area", "mel_temporal", "octave_hann_style", "ragged_tail"])
    for k in ("k_stft_band_1k", "k_stft_band_4k2", "k_stft_mel_v2"):  # (complex results at n_fft 2048: the headline kernel's CPLX instantiation since round 5)
        assert k in out, out


def test_n512_bank_kernel_emulated_against_the_restatement(emulated):
    """k_stft_band_512 (round 5; n_fft 512 had run the size-generic kernels): the 4 x 4 x 4 x 4 transform in four registers
    per lane with its three transposes, every tap variant, real / magnitude / norm-exponent / complex results, register re-use
    and whole-frame fetches, through bftObj_new's own plan and dispatcher -- and the row-segment plans (SPLIT instantiations) of
    the n_fft 512 and n_fft 1024 kernels; on the device the same cases meet the compiled reference (tests/test_bft_gpu.py)"""
    out = _run(emulated, "emulated_bft512.py", [])
    assert "emulated k_stft_band_512 9, k_stft_band_1k 3" in out, out[-800:]


def test_one_launch_mel_mfcc_emulated_at_every_fused_size(emulated):
    """round 6: the cepstrum block of afx_ccblock.h inside k_stft_band_512 / _1k / _4k2 and the general form of k_stft_mel_v2 --
    mel + MFCC from ONE emulated launch per call at n_fft 512 / 1024 / 2048 / 4096: whole-row and segment plans, num 128 / 64 /
    40 / 20, log and cube-root rectification, partial 16-row blocks -- against the float64 restatement, route asserted"""
    out = _run(emulated, "emulated_mfcc_sizes.py", [])
    assert "one-launch mel + MFCC cases: 11" in out, out[-800:]
    # long runs of frames per wave: whole 16-row blocks behind each other
    out = _run(emulated, "emulated_mfcc_sizes.py", [], env="AFX_EMU_CUS=1")
    assert "one-launch mel + MFCC cases: 4" in out, out[-800:]


def test_spectrum_kernels_emulated_against_float64(emulated):
    """afxk_stft4k / afxk_stft1k / afxk_stft512 = k_stft_band_4k2 / _1k / _512 <STFT> (round 5: the STFT object, the linear-scale
    slices and the reassignment object's transforms at n_fft 4096 / 1024 / 512): every store family of the epilogues -- a lane's
    bins and their partners, lane 0's special slots, the conjugate mirrors above N / 2 -- with and without range checks, plain
    and mapped, against numpy's float64 FFT; on the device the same kernels meet the compiled reference (tests/test_stft_gpu.py)"""
    out = _run(emulated, "emulated_stft4k.py", [])
    for k in ("k_stft_band_4k2", "k_stft_band_1k", "k_stft_band_512"):
        assert f"emulated {k} 4" in out, out[-1200:]
    assert out.count("mirrors are exact conjugates") == 3, out[-1200:]


def test_one_launch_inverse_stft_and_stft256_emulated_against_float64(emulated):
    """round 6: k_istft_w256 / _wsmall / _w2048 / _w4096 (the inverse of a frame as ONE forward real wave transform of re + im of the
    Hermitian part; overlap-add in an LDS ring over runs of frames, the frames before a run transformed again for their tails; an
    output buffer that is not zero; a non-Hermitian part in the input that must not reach the output) and k_stft_256 (two real frames
    per 256-point complex transform, odd and even frame counts, a mapped bin slice) against numpy in float64; on the device the same
    kernels meet the compiled reference (tests/test_stft_gpu.py)"""
    out = _run(emulated, "emulated_istft.py", [])
    lines = out.splitlines()
    assert sum(l.startswith("istft n_fft") for l in lines) == 6 and sum(l.startswith("stft n_fft 256") for l in lines) == 3, out[-1500:]


def test_f32_matrix_core_octave_kernels_emulated(emulated):
    """calibration of the f32 MFMA model: k_cqt_octave_mfma / _mfma_w (AFX_CQT_F32=1; measured on the device in round 1)"""
    n = _launches(_run(emulated, "emulated_cqt.py", ["c84_32k_area", "power_max"], "AFX_CQT_F32=1"))
    assert n["octave_f32"] == 14 and n["octave_f16"] == 0, n


def test_time_domain_cwt_kernel_emulated(emulated):
    """k_cwt_td (round 3, afx_cwt_td.hip): the host plan (double IFFT of the bank rows, truncation, pairing, f16 images),
    the launcher (two kernel classes, exact workgroup shares) and the device code -- window fetch with the reflect / wrap
    index map at the chunk edges, the (hi, lo) split, the K loop, the transposed epilogue -- on BASELINE cfg 4's plan,
    padded and circular, a speech clip and a -80 dB level step, and the derivative transform's plan (cwtObj_enableDet,
    round 4): every row the plan owns within 5e-6 of the reference (on the MI355X: 4e-7 on the bench clip)"""
    out = _run(emulated, "emulated_cwt_td.py", [])
    assert out.count("time-domain rows") == 4 and "derivative: 16 time-domain rows" in out and "against float64" in out, out[-800:]


def test_bf16x3_gemm_emulated_matches_float64(emulated):
    """k_gemm_nt128_bf16x3 and k_bank_split + k_gemm_bank_bf16x3: loader / three-word split / 24 MFMAs per k-step / epilogue with
    every tail, elementwise against float64 on operands spanning ten decades; then the whole table of tests/test_gemm_gpu.py for
    these two entry points through the same runner, its refusals and its non-finite operands"""
    out = _run(emulated, "emulated_gemm.py", [])
    assert out.count("elementwise relative error") == 8 and out.count("bank form") == 5
    # the table of the device test (tests/gemm_cases.py) on the two bf16 entry points, every case at the device test's bar
    from tests import gemm_cases
    n = sum(c.kernel != "f32" for c in gemm_cases.table())
    assert n >= 100 and out.count("elementwise error max") == n and f"table: {n} cases, 0 over their bars" in out, out[-2000:]
    assert out.count("non-finite operands") == 4


def test_dense_route_producer_emulated_against_float64(emulated):
    """afxk_stft2k = k_stft_mel_v2 <STFT> (round 6): the headline kernel's transform storing its mapped spectrum row -- the [T, F]
    rows of the dense-bank route (16-byte stores on rows of 1028 floats, zero pad), bin slices, magnitude / power-law maps, hops
    with and without the register re-use -- against numpy's float64 FFT.  With k_gemm_bank_bf16x3 (the prepared-bank product,
    test above) these are the two launches of bftObj_bft for dense (gammatone) banks; on the device they meet the compiled
    reference (tests/test_bft_gpu.py::test_dense_bank_at_the_headline_shape)"""
    out = _run(emulated, "emulated_stft2k.py", [])
    assert "pad words are zeros" in out and "power law 0.3" in out, out[-800:]


@pytest.fixture(scope="module")
def emulated_tsan(tmp_path_factory):
    """the same objects under clang's ThreadSanitizer with two small C drivers (tests/emu/driver_emu_small.c, _gemm.c); a
    second build of the f16 octave kernel with its LDS ordering points removed (the check's own test)"""
    import re
    from concurrent.futures import ThreadPoolExecutor
    tmp = str(tmp_path_factory.mktemp("emu_tsan"))
    san = ["-O1", "-gline-tables-only", "-fsanitize=thread", "-fno-omit-frame-pointer"]
    stub = os.path.join(tmp, "stub.c")
    subprocess.run([sys.executable, os.path.join(STUB, "gen_stub.py"), os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_device.h"),
                    stub, "--functional-cqt", "--omit=afxk_gemm_nt128_bf16", "--omit=afxk_gemm_bank_prepare", "--omit=afxk_gemm_nt_bank", "--omit=afxk_cqt_pyramid", "--omit=afxk_cqt_pyramid_plan"], check=True)
    src = open(os.path.join(ROOT, "audioflux_amd", "csrc", "hip", "afx_cqt.hip")).read()
    with open(os.path.join(tmp, "afx_cqt_host.hip"), "w") as f:
        f.write(re.sub(r"(?m)^(\s*)__shared__ ", r"\1static ", src))
    with open(os.path.join(tmp, "cqt_emulated_main.cpp"), "w") as f:
        f.write('#include "hip/hip_runtime.h"\nnamespace {\nalignas(16) unsigned char smem_raw[160 * 1024];\n}\n'
                f'#include "{tmp}/afx_cqt_host.hip"\n')
    hostdir = os.path.join(ROOT, "audioflux_amd", "csrc", "host")
    jobs = [[CLANG, "-std=gnu11", *san, "-ffp-contract=off", *INC, "-c", os.path.join(hostdir, f), "-o", os.path.join(tmp, f[:-2] + "_c.o")]
            for f in sorted(os.listdir(hostdir)) if f.endswith(".c")]
    jobs.append([CLANG, "-std=gnu11", *san, *STANDIN_RENAMES, *INC, "-c", stub, "-o", os.path.join(tmp, "stub.o")])
    for d in ("driver_emu_small", "driver_emu_gemm", "driver_emu_bft"):
        jobs.append([CLANG, "-std=gnu11", *san, *INC, "-c", os.path.join(EMU, d + ".c"), "-o", os.path.join(tmp, d + ".drv")])
    for f in EMU_UNITS:
        jobs.append([CLANG + "++", "-std=c++17", *san, f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c", os.path.join(EMU, f + ".cpp"), "-o", os.path.join(tmp, f + ".o")])
    jobs.append([CLANG + "++", "-std=c++17", *san, f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c", os.path.join(tmp, "cqt_emulated_main.cpp"), "-o",
                 os.path.join(tmp, "cqt_emulated_main.o")])
    jobs.append([CLANG + "++", "-std=c++17", *san, "-DAFX_EMU_NO_LDS_ORDER", f"-I{EMU}", f"-I{EMU}/hip", *INC, "-c", os.path.join(EMU, "cqt_emulated_f16.cpp"),
                 "-o", os.path.join(tmp, "cqt_emulated_f16.neg")])
    with ThreadPoolExecutor(8) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(".o"))
    exes = {}
    for name, drv, swap in (("small", "driver_emu_small.drv", None), ("gemm", "driver_emu_gemm.drv", None), ("bft", "driver_emu_bft.drv", None),
                            ("negative", "driver_emu_small.drv", "cqt_emulated_f16")):
        use = [o for o in objs if not (swap and o.endswith(swap + ".o"))] + ([os.path.join(tmp, swap + ".neg")] if swap else [])
        exes[name] = os.path.join(tmp, "emu_tsan_" + name)
        r = subprocess.run([CLANG + "++", *san, *use, os.path.join(tmp, drv), "-lm", "-lpthread", "-o", exes[name]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exes


@pytest.mark.parametrize("exe,env", [("small", ""), ("small", "AFX_CQT_F32=1"), ("gemm", ""), ("bft", "")])
def test_emulated_kernels_have_no_lds_races(emulated_tsan, exe, env):
    """the lanes of an emulated kernel are host threads that meet only at the kernel's own cross-lane operations and
    LDS-ordering points (wave_lds_order, __syncthreads): under ThreadSanitizer an LDS word written by one lane and read
    by another without such a point in between is a data race -- a missing ordering point in the kernel, which on the
    device shows up only when the compiler or the hardware reorders the two accesses.  None in the CQT kernels or the
    three-word GEMM; "bft": the fused STFT -> filter-bank kernels of n_fft 1024 /
    4096 / 2048-complex (tests/emu/driver_emu_bft.c)."""
    e = dict(os.environ)
    for k in ("AFX_CQT_CHUNK", "AFX_CQT_F32", "AFX_NO_FUSED"):
        e.pop(k, None)
    if env:
        e.update(kv.split("=") for kv in env.split())
    e.update(AFX_QUIET="1")
    r = subprocess.run([emulated_tsan[exe]], capture_output=True, text=True, env=e, timeout=1500)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "OK" in r.stdout, out[-3000:]
    assert "ThreadSanitizer" not in out, out[-3000:]


def test_the_lds_race_check_sees_missing_ordering_points(emulated_tsan):
    """with the wave_lds_order() calls of afx_cqt_f16.hip (k_cqt_pyramid, k_cqt_octave_f16) compiled out the same run is
    full of reports"""
    r = subprocess.run([emulated_tsan["negative"]], capture_output=True, text=True, env=dict(os.environ, AFX_QUIET="1"), timeout=1500)
    assert "WARNING: ThreadSanitizer: data race" in r.stderr and ("k_cqt_pyramid" in r.stderr or "k_cqt_octave_f16" in r.stderr), \
        (r.stdout + r.stderr)[-2000:]
