#!/usr/bin/env python3
"""Writes tests/golden/timestretch.npz (and timestretch_vocoder.npz: the STFT and vocoder planes of the n_fft 128 and 256 cases) from the compiled reference alone (oracle/_ref/libaudioflux_ref.so): per case of
tests/timestretch_cases.py the expected output and the parity bar.

The bar.  The phase accumulator of the vocoder is an unbounded float32 sum, so two correct float32 implementations of the
algorithm whose FFTs round differently sit far above 1e-5 from each other.  That distance is measured:
  1. the reference's STFT of the case against a float64 STFT of the same frames: peak error e (relative to the spectrum's peak);
  2. white noise of standard deviation e * peak on the real and imaginary planes of the half spectrum (the imaginary parts of
     bins 0 and N / 2 stay as they are), eight seeds;
  3. the reference's phase_vocoder and stftObj_istft on each perturbed spectrum;
  4. the worst peak-relative and the worst L2-relative deviation from the unperturbed result.
bar = max(2 * worst, 1e-5), per case and per norm.  Pitch shift: the perturbed and the unperturbed stretched signals through
the reference's resampler (Fast, isScale 1, ratio = rate).  Prints the table DESIGN.md quotes."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resample_cases as rc  # noqa: E402
from tests import timestretch_cases as tc  # noqa: E402

SEEDS = 8


def window64(c):
    N = 1 << c["exp"]
    k = np.arange(N) / N
    return 0.54 - 0.46 * np.cos(2 * np.pi * k) if c.get("win") == tc.HAMM else 0.5 - 0.5 * np.cos(2 * np.pi * k)


def stft64(c, x, T1):
    N = 1 << c["exp"]
    w = window64(c)
    frames = np.stack([x[t * c["hop"]:t * c["hop"] + N].astype(np.float64) * w for t in range(T1)])
    return np.fft.fft(frames, axis=1)


def full(half, N):
    """[T, F] complex half spectrum -> re, im [T, N] float32 with the conjugate mirror"""
    F = N // 2 + 1
    z = np.concatenate([half, np.conj(half[:, F - 2:0:-1])], axis=1)
    return np.ascontiguousarray(z.real, np.float32), np.ascontiguousarray(z.imag, np.float32)


def synth(ref, stft, c, re, im, rate):
    """phase_vocoder + weighted overlap-add onto zeros: the inverse transform's samples"""
    re2, im2 = tc.ref_vocoder(ref, c, re, im, rate)
    out = np.zeros(tc.lengths(c, rate)[2], np.float32)
    ref.stftObj_istft(stft, tc.ptr(re2), tc.ptr(im2), re2.shape[0], 0, tc.ptr(out))
    return out


def resample(ref, y, n, rate):
    """pitchShift_algorithm.c:66-75 on a stretched signal y: capacity-sized zero buffer, roundf(n / rate) samples resampled"""
    rb = rc.ref_lib()
    obj = C.c_void_p(None)
    assert rb.resampleObj_new(C.byref(obj), C.pointer(C.c_int(rc.FAST)), C.pointer(C.c_int(1)), None) == 0
    rb.resampleObj_setSamplateRatio(obj, C.c_float(rate))
    stretched = tc.roundf(n, rate)
    buf = np.zeros(max(stretched, len(y)) + 8, np.float32)
    buf[:len(y)] = y
    out = np.zeros(2 * n + 64, np.float32)
    m = rb.resampleObj_resample(obj, tc.ptr(buf), stretched, tc.ptr(out))
    rb.resampleObj_free(obj)
    return out[:m]


def measure(ref, c, x, rate, post=None):
    """(unperturbed result, e, worst peak-relative, worst L2-relative deviation over the seeds)"""
    N = 1 << c["exp"]
    F = N // 2 + 1
    stft, re, im = tc.ref_stft(ref, c, x)
    T1 = re.shape[0]
    exact = stft64(c, x, T1)
    peak = np.abs(exact).max()
    e = np.abs((re.astype(np.float64) + 1j * im) - exact).max() / peak
    assert e < 1e-6, e
    post = post or (lambda y: y)
    y0 = post(synth(ref, stft, c, re, im, rate))
    worst = [0.0, 0.0]
    half = re[:, :F].astype(np.float64) + 1j * im[:, :F]
    for seed in range(SEEDS):
        g = np.random.default_rng(1000 + seed)
        nr, ni = g.standard_normal(half.shape) * e * peak, g.standard_normal(half.shape) * e * peak
        ni[:, 0] = ni[:, F - 1] = 0
        pr, pi = full(half + nr + 1j * ni, N)
        p, l2 = tc.errors(post(synth(ref, stft, c, pr, pi, rate)), y0)
        worst = [max(worst[0], p), max(worst[1], l2)]
    ref.stftObj_free(stft)
    return y0, e, worst


def main():
    ref = tc.ref_lib()
    assert ref is not None, "needs oracle/_ref/libaudioflux_ref.so (make -C oracle)"
    out, voc = {}, {}
    print("| case | frames in / out | e (STFT vs float64) | worst peak-rel | worst L2-rel | bar peak | bar L2 |")
    print("|---|---|---|---|---|---|---|")
    for name, c in tc.CASES.items():
        x = tc.case_input(name)
        ret, cap, got = tc.run_case(ref, name)
        T1, T2, L2 = tc.lengths(c, c["rate"])
        y0, e, worst = measure(ref, c, x, c["rate"])
        assert tc.same_bits(y0, got[:L2]) and not got[L2:].any(), name  # the object is STFT + phase_vocoder + istft
        bar = [max(2 * w, 1e-5) for w in worst]
        out[name + "/out"], out[name + "/meta"], out[name + "/bar"] = y0, np.array([ret, cap, L2]), np.array(bar)
        print(f"| {name} | {T1} / {T2} | {e:.1e} | {worst[0]:.1e} | {worst[1]:.1e} | {bar[0]:.1e} | {bar[1]:.1e} |")
        if name in tc.SMALL:
            for k, a in enumerate(tc.expected_vocoder(name)):
                voc[f"{name}/voc{k}"] = a
    for name, c in tc.PITCH.items():
        x = tc.case_input(name)
        rate = float(tc.semitone_rate(c["semi"]))
        m = tc.pitch_length(c["n"], c["semi"])
        want = tc.expected_pitch(name)
        y0, e, worst = measure(ref, c, x, rate, post=lambda y: resample(ref, y, c["n"], rate)[:m])
        assert tc.same_bits(y0, want), name  # the object is time stretch + resampler
        bar = [max(2 * w, 1e-5) for w in worst]
        out[name + "/out"], out[name + "/bar"] = want, np.array(bar)
        T1, T2, _ = tc.lengths(c, rate)
        print(f"| {name} | {T1} / {T2} | {e:.1e} | {worst[0]:.1e} | {worst[1]:.1e} | {bar[0]:.1e} | {bar[1]:.1e} |")
    seq = dict(exp=8, hop=64, n=3000)
    for k, y in enumerate(tc.expected_sequence()):
        y0, e, worst = measure(ref, seq, rc.signal(3000, seed=5), tc.SEQUENCE[k])
        assert tc.same_bits(y0, y), k
        bar = [max(2 * w, 1e-5) for w in worst]
        out[f"sequence/{k}"], out[f"sequence/{k}/bar"] = y, np.array(bar)
        print(f"| sequence {k}: rate {tc.SEQUENCE[k]} | {tc.lengths(seq, tc.SEQUENCE[k])[0]} / {tc.lengths(seq, tc.SEQUENCE[k])[1]} | {e:.1e} | "
              f"{worst[0]:.1e} | {worst[1]:.1e} | {bar[0]:.1e} | {bar[1]:.1e} |")
    # the drop-in flows: channel 0 is the input of DROPIN_CASE, channel 1 the same reversed
    c = tc.CASES[tc.DROPIN_CASE]
    for ch, x in enumerate((tc.case_input(tc.DROPIN_CASE), tc.case_input(tc.DROPIN_CASE)[::-1].copy())):
        for name, rate in tc.DROPIN_STRETCH.items():
            _, e, worst = measure(ref, c, x, rate)
            out[f"dropin/{name}/{ch}/bar"] = np.array([max(2 * w, 1e-5) for w in worst])
            print(f"| dropin {name}, channel {ch} | {tc.lengths(c, rate)[0]} / {tc.lengths(c, rate)[1]} | {e:.1e} | {worst[0]:.1e} | "
                  f"{worst[1]:.1e} | {max(2 * worst[0], 1e-5):.1e} | {max(2 * worst[1], 1e-5):.1e} |")
        for name, semi in tc.DROPIN_SHIFT.items():
            rate = float(tc.semitone_rate(semi))
            m = tc.pitch_length(c["n"], semi)
            _, e, worst = measure(ref, c, x, rate, post=lambda y: resample(ref, y, c["n"], rate)[:m])
            out[f"dropin/{name}/{ch}/bar"] = np.array([max(2 * w, 1e-5) for w in worst])
            print(f"| dropin {name}, channel {ch} | {tc.lengths(c, rate)[0]} / {tc.lengths(c, rate)[1]} | {e:.1e} | {worst[0]:.1e} | "
                  f"{worst[1]:.1e} | {max(2 * worst[0], 1e-5):.1e} | {max(2 * worst[1], 1e-5):.1e} |")
    # capacity of the reference over rates and lengths (tests/test_timestretch_cpu.py)
    rows = []
    for exp, hop in ((8, 64), (10, 256), (12, 1024)):
        st, obj = tc.new(ref, dict(exp=exp, hop=hop))
        for n in (4096, 4097, 5000, 7919, 12000, 20000, 22050, 30001, 44100, 65536, 100003, 1323000):
            for r in np.arange(10, 41) * np.float32(0.05):
                r = float(np.float32(r))
                cap = ref.timeStretchObj_calDataCapacity(obj, C.c_float(r), n)
                rows.append((exp, hop, n, r, cap))
        ref.timeStretchObj_free(obj)
    out["lengths"] = np.array(rows, np.float64)
    np.savez_compressed(tc.GOLDEN, **out)
    np.savez_compressed(tc.GOLDEN_VOCODER, **voc)
    print(f"wrote {tc.GOLDEN_VOCODER}: {os.path.getsize(tc.GOLDEN_VOCODER)} bytes")
    print(f"wrote {tc.GOLDEN}: {os.path.getsize(tc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
