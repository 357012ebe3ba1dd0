"""CPU-only: one frame / tail state machine.  The STFT object's streaming hook (afx_test_stft_stream, what stftObj_stft
and the spectrogram object upload call after call) and the frame-tail hook (afx_test_frametail, what the CQT and YIN
objects upload) are fed the same random call-length sequences and must agree on every frame count, every kept tail and
every assembled signal.  Both drive afx_frametail.c; a framing rule written a second time somewhere would part here."""
import ctypes as C

import numpy as np
import pytest

import audioflux_amd as af

fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)


def _lens(rng, n_fft, hop, calls):
    kind = rng.integers(0, 3, calls)
    big = rng.integers(1, 3 * n_fft + hop, calls)
    small = rng.integers(1, max(2, hop), calls)  # shorter than a hop
    return np.where(kind == 0, 1, np.where(kind == 1, small, big)).astype(np.int32)  # a third are single samples


@pytest.mark.parametrize("r,hop", [(6, 16), (6, 64), (6, 23), (6, 100), (6, 333), (7, 1), (4, 5)])
def test_stft_hook_and_frametail_hook_agree(r, hop):
    L = af.get_lib()
    L.afx_test_stft_stream.restype = C.c_int
    L.afx_test_stft_stream.argtypes = [C.c_int, C.c_int, C.c_int, fp, ip, C.c_int, fp, ip, ip, ip]
    L.afx_test_frametail.restype = C.c_int
    L.afx_test_frametail.argtypes = [C.c_int, C.c_int, C.c_int, fp, ip, C.c_int, ip, ip, ip, dp]
    n_fft = 1 << r
    rng = np.random.default_rng(100 * r + hop)
    for _ in range(8):
        k = 60
        lens = _lens(rng, n_fft, hop, k)
        lens[-1] = 5 * hop + n_fft  # the last call always has frames
        x = rng.standard_normal(int(lens.sum())).astype(np.float32)
        cur = np.zeros(len(x) + n_fft * k + 16, np.float32)
        cur_l, tl, tails_s = (np.zeros(k, np.int32) for _ in range(3))
        assert L.afx_test_stft_stream(r, hop, 0, x.ctypes.data_as(fp), lens.ctypes.data_as(ip), k, cur.ctypes.data_as(fp),
                                      cur_l.ctypes.data_as(ip), tl.ctypes.data_as(ip), tails_s.ctypes.data_as(ip)) == 0
        frames, tails_f, curs = (np.zeros(k, np.int32) for _ in range(3))
        sums = np.zeros(k, np.float64)
        assert L.afx_test_frametail(n_fft, hop, 1, x.ctypes.data_as(fp), lens.ctypes.data_as(ip), k, frames.ctypes.data_as(ip),
                                    tails_f.ctypes.data_as(ip), curs.ctypes.data_as(ip), sums.ctypes.data_as(dp)) == 0
        assert np.array_equal(tl, frames), (r, hop)
        assert np.array_equal(tails_s, tails_f), (r, hop)
        assert np.array_equal(cur_l, curs), (r, hop)
        assert int(frames.sum()) == (len(x) - n_fft) // hop + 1  # the pieces yield the frames of the whole
        assert (frames > 0).any() and (hop < 16 or (frames == 0).any())  # calls with and without frames
        ends, pos = np.cumsum(lens), 0
        for c in range(k):
            seg = cur[pos:pos + cur_l[c]]
            pos += cur_l[c]
            if frames[c] == 0:
                assert cur_l[c] == 0
                continue
            # the assembled signal: the samples up to the end of this call, `total` of them ...
            assert np.array_equal(seg, x[ends[c] - cur_l[c]:ends[c]]), (r, hop, c)
            # ... and the one the frame-tail hook summed
            want = float(np.dot(seg.astype(np.float64), np.arange(1, len(seg) + 1)))
            assert np.isclose(sums[c], want, rtol=1e-12, atol=1e-9), (r, hop, c)
