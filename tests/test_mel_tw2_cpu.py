"""CPU: the W_64 twiddles of the headline kernel's n_fft 2048 transform applied by the READER of exchange 2
(afx_melfused2.hip, round 10): the table's index algebra and LDS banks (tools/proto_fft1024_v3.py), its entries against
the writer-side table it replaces, and one wave's transform restated in float32 both ways.

A product cmul(value, twiddle) has the same operands in the same roles on either side of the exchange, so the power
spectrum keeps its bits; only elements multiplied by (1, -0) on one side and not at all on the other can differ, in the
sign of an exact zero, which |X|^2 does not see."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
T_TW2, TW2_PITCH, T_BAND = 16384, 32, 21056  # afx_melfused2.hip


@pytest.fixture(scope="module")
def proto():
    spec = importlib.util.spec_from_file_location("proto_fft1024_v3", os.path.join(ROOT, "tools", "proto_fft1024_v3.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def wave_lib():
    """tests/emu/mel_tw2_emulated.cpp compiled for the host like the emulated kernels (tests/test_emulated_kernels.py)"""
    if not os.path.exists(CLANG):
        pytest.skip("needs clang (the emulated device headers use its vector types)")
    tmp = tempfile.mkdtemp(prefix="afx_tw2_")
    lib = os.path.join(tmp, "libtw2.so")
    inc = [f"-I{EMU}", f"-I{EMU}/hip", f"-I{ROOT}/include", f"-I{ROOT}/audioflux_amd/csrc/hip", f"-I{ROOT}/audioflux_amd/csrc/host"]
    r = subprocess.run([CLANG + "++", "-std=c++17", "-O2", "-fPIC", "-shared", *inc, os.path.join(EMU, "mel_tw2_emulated.cpp"),
                        "-lm", "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = C.CDLL(lib)
    fp = C.POINTER(C.c_float)
    h.afx_tw2_wave.argtypes = [fp, fp, C.c_int, fp]
    h.afx_tw2_wave.restype = None
    h.afx_tw2_old_table.argtypes = [fp]
    h.afx_tw2_old_table.restype = None
    return h


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_prototype_banks_and_rows(proto):
    """every stage-3 read class of the table, lane group by lane group, meets no bank twice; the rows are the issue's"""
    proto.check_rows()
    res = proto.check_banks()
    assert len(res) == 8 and all(v == 1 for v in res.values()), res
    assert proto.TW2_PITCH == TW2_PITCH and TW2_PITCH % 16 == 0
    proto.main()


def test_table_entries_have_the_old_table_bits(wave_lib):
    """entry (m, j) of the kernel's table -- row j, place m - 1 -- against entry (m, j) of the [4][16] writer-side table"""
    import audioflux_amd
    lib = audioflux_amd.get_lib()
    lib.afxk_mel2k_tables.restype = C.c_int
    lib.afxk_mel2k_tables.argtypes = [C.POINTER(C.c_float), C.c_int]
    assert lib.afxk_mel2k_tables(None, 0) == T_BAND
    tab = np.full(T_BAND // 4, np.nan, np.float32)
    assert lib.afxk_mel2k_tables(fptr(tab), T_BAND) == T_BAND
    new = tab[T_TW2 // 4: T_TW2 // 4 + 16 * TW2_PITCH // 4].reshape(16, 4, 2)
    old = np.zeros((4, 16, 2), np.float32)
    wave_lib.afx_tw2_old_table(fptr(old))
    for j in range(16):
        for m in (1, 2, 3):
            assert new[j, m - 1].tobytes() == old[m, j].tobytes(), (m, j, new[j, m - 1], old[m, j])
    # row 0 is (1, -0) three times: the old table's column j = 0
    assert np.all(new[0, :3, 0] == 1.0) and np.all(new[0, :3, 1] == 0.0) and np.all(np.signbit(new[0, :3, 1]))
    assert np.all(old[0, :, 0] == 1.0) and np.all(np.signbit(old[0, :, 1]))
    assert np.all(new[:, 3] == 0.0)  # the pad
    # the table ends before the split twiddles that follow it (T_TW3 = 16960)
    assert T_TW2 + 16 * TW2_PITCH <= 16960


def _inputs():
    n = np.arange(2048)
    noise = (0.1 * np.random.default_rng(10).standard_normal(2048)).astype(np.float32)
    silence = np.zeros(2048, np.float32)
    imp0 = np.zeros(2048, np.float32)
    imp0[0] = 1.0
    imp_odd = np.zeros(2048, np.float32)
    imp_odd[777] = 1.0
    sine = np.sin(2 * np.pi * 200 * n / 2048).astype(np.float32)  # full scale, centre of bin 200
    return {"noise": noise, "silence": silence, "impulse at 0": imp0, "impulse at 777": imp_odd, "sine on bin 200": sine}


@pytest.mark.parametrize("name", list(_inputs()))
@pytest.mark.parametrize("window", ["hann", "rect"])
def test_power_bins_keep_their_bits(wave_lib, name, window):
    """one wave's transform with the twiddles before and behind exchange 2: 1025 power bins, bit for bit.  (rect: the
    impulse at sample 0 survives the window -- under hann it is a second silence)"""
    x = _inputs()[name]
    n = np.arange(2048)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * n / 2048)).astype(np.float32) if window == "hann" else np.ones(2048, np.float32)
    out = {}
    for side in (0, 1):
        p = np.full(1025, np.nan, np.float32)
        wave_lib.afx_tw2_wave(fptr(x), fptr(win), side, fptr(p))
        assert np.isfinite(p).all()
        out[side] = p
    assert out[0].tobytes() == out[1].tobytes(), np.nonzero(out[0] != out[1])
    # the restatement is the transform: float64 rfft of the same windowed samples (2e-6 of the peak: tests/emu/emulated_stft2k.py's bar)
    want = np.abs(np.fft.rfft(x.astype(np.float64) * win.astype(np.float64))) ** 2
    if want.max() > 0:
        assert np.abs(out[1] - want).max() <= 2e-6 * want.max()
    else:
        assert np.all(out[1] == 0.0)
