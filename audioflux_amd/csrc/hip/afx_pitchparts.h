// afx_pitchparts.h -- the device pieces the pitch kernels share (afx_pitch_yin.hip, afx_pitch_hs.hip, afx_pitch_pef.hip), each
// written once: the decode of a row into (clip, frame, samples) and the first argmax of a curve -- thread-local, then over the
// workgroup.  Integer operations, comparisons and shuffles only: no arithmetic on a value.  What a kernel does with the winner
// (the fallback to minIndex, the stores of fre / value) differs from tracker to tracker and stays there.
//
// The argmax pieces are statement macros over the caller's (bv, bi), not functions.  The compiler inlines a __forceinline__
// function only after its first simplification passes have seen the kernel with the call in it, and these kernels' code is
// sensitive to that: with the pieces as functions -- by reference, or by value with the assignments left at the call site --
// the instruction streams of k_pitch_hs / k_pitch_pef differ from the hand-expanded kernels' in thousands of lines (other
// hoists out of the row loop, other unrolling), a result struct moves the register counts, and HPS / LHS at n_fft 1024 / 2048
// and PEF at 1024 measured 0.2 ... 0.5 % slower (profiles/pitch_family_ab_mi355x.txt).  Expanded as text they compile to the
// same instructions as before.
#ifndef AFX_PITCHPARTS_H
#define AFX_PITCHPARTS_H

#include <hip/hip_runtime.h>

#define AFX_PITCH_NONE 0x7fffffff  // the index of "no candidate yet"

// row = clip b * timeLength + frame t: the frame's samples
__device__ __forceinline__ const float *afx_pitch_row(const float *x, long long row, int timeLength, long long clipStride, int hop,
                                                      int &b, int &t) {
    b = (int)(row / timeLength);
    t = (int)(row - (long long)b * timeLength);
    return x + (long long)b * clipStride + (long long)t * hop;
}

// the workgroup of the kernels that transform L = 2^R complex points in LDS per frame (afx_pitch_lag.hip, afx_harmonic_ratio.hip)
template <int R>
struct AfxPitchLagCfg {
    static constexpr int L = 1 << R;
    // threads: one radix-4 butterfly each per pass up to L = 4096, two at 8192.  A workgroup holds up to 66 KB of LDS, so a
    // CU runs one or two of the large ones: the waves that hide LDS and barrier latency come from inside the workgroup
    static constexpr int NT = L / 4 < 64 ? 64 : (L / 4 > 1024 ? 1024 : L / 4);
};

// thread-local, indices visited in rising order: the FIRST maximum from minIndex on (a strict >)
#define AFX_PITCH_CANDIDATE(bv, bi, c, j, minIndex)                          \
    if ((j) >= (minIndex) && ((bi) == AFX_PITCH_NONE || (c) > (bv))) {       \
        (bv) = (c);                                                          \
        (bi) = (j);                                                          \
    }

// (ov, oi) against (bv, bi): the larger value, the smaller index among equal ones, so that rows of equal values (zeros, -inf)
// come out as their first index (__vmax, flux_vector.c:1536)
#define AFX_PITCH_FOLD(bv, bi, ov, oi)                                                                          \
    if ((oi) != AFX_PITCH_NONE && ((bi) == AFX_PITCH_NONE || (ov) > (bv) || ((ov) == (bv) && (oi) < (bi)))) {  \
        (bv) = (ov);                                                                                            \
        (bi) = (oi);                                                                                            \
    }

// First argmax over the workgroup's NT threads (a constant expression); every thread runs it, the result is valid in thread 0
// (AFX_PITCH_NONE: no thread had a candidate).  red: 32 dwords of LDS -- values at [wave], indices at [16 + wave] -- in use
// until the caller's next barrier.  tid, lane and wave are the call site's, as it holds them (the PEF kernel pins its tid per
// row).
#define AFX_PITCH_ARGMAX(NT, bv, bi, red, tid, lane, wave)                       \
    {                                                                            \
        _Pragma("unroll") for (int msk_ = 32; msk_ > 0; msk_ >>= 1) {            \
            const float ov_ = __shfl_xor((bv), msk_);                            \
            const int oi_ = __shfl_xor((bi), msk_);                              \
            AFX_PITCH_FOLD(bv, bi, ov_, oi_)                                     \
        }                                                                        \
        if ((lane) == 0) {                                                       \
            (red)[(wave)] = (bv);                                                \
            reinterpret_cast<int *>(red)[16 + (wave)] = (bi);                    \
        }                                                                        \
        __syncthreads();                                                         \
        if ((tid) == 0) {                                                        \
            _Pragma("unroll") for (int w_ = 1; w_ < (NT) / 64; ++w_) {           \
                const float ov_ = (red)[w_];                                     \
                const int oi_ = reinterpret_cast<int *>(red)[16 + w_];           \
                AFX_PITCH_FOLD(bv, bi, ov_, oi_)                                 \
            }                                                                    \
        }                                                                        \
    }

#endif  // AFX_PITCHPARTS_H
