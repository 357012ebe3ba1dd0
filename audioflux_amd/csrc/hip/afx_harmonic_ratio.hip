// afx_harmonic_ratio.hip -- the harmonic ratio (include/mir/harmonicRatio_algorithm.h), from samples to one value per frame.
//
// One workgroup per frame, the transform of afx_pitch_lag.hip: with N = windowLength and L = 2N = 2^R, one buffer of L complex
// points in LDS (afx_ldsfft.h) serves all of
//   1. f[n] = x[n] w[n], n < N, zeros up to L; each thread keeps the running sum of squares of ITS samples, and a workgroup
//      scan turns these into cum[n] = sum of f[m]^2, m <= n (a tree where the reference sums serially: other rounding);
//   2. one L-point transform, P[k] = |X[k]|^2 in place with the move back to natural order, the inverse as a second forward
//      transform: r[n] = Re s[bitrev(n)] / L, r[0] the frame's energy;
//   3. cum[n] goes into the imaginary half of s[n], which nobody reads any more: c[j] = cum[N - 2 - j];
//   4. minIndex = j - 1 for the first j in 2 ... maxLength with a sign change (or a zero) between r[j - 1] and r[j] -- a
//      min-index reduction;
//   5. g[j] = r[j] / sqrtf((float)(r[0] c[j] + 1e-16)) for j = minIndex + 1 ... maxLength - 1 in the reference's operation order
//      (harmonicRatio_algorithm.c:270-272), its first maximum (afx_pitchparts.h) and, away from the ends of the range,
//      util_qaudInterp (flux_util.c:771-780) in its mixed float / double order.
// The reference sets minIndex once per CALL, so a frame without a crossing inherits the value of the nearest earlier frame of
// its clip that had one (0 when there is none).  Frames stay independent here: launch 1 lets such a frame assume 0 and records
// NONE; k_harmonic_ratio_resolve walks each clip's records (one wave per clip, a "last valid value" scan) and lists the frames
// whose inherited value is not 0; launch 3 runs those frames again with minIndex given (the same kernel, the list as its
// rows).  Everything is ordered by the stream.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_pitchparts.h"

namespace {

// r[j] / L sits at the bit-reversed position's real half, cum[n] at position n's imaginary half
template <int R>
__device__ __forceinline__ float hr_lag(const float2 *s, int j, float invL) {
    return s[afx_lds_pad((int)(__brev((unsigned)j) >> (32 - R)))].x * invL;
}

// harmonicRatio_algorithm.c:271: the product in float32, the sum in double, rounded to float32 for sqrtf
template <int R>
__device__ __forceinline__ float hr_gamma(const float2 *s, int j, float r0, float invL) {
    const float c = s[afx_lds_pad((1 << (R - 1)) - 2 - j)].y;
    const float p = r0 * c;
    return hr_lag<R>(s, j, invL) / sqrtf((float)((double)p + 1e-16));
}

// util_qaudInterp (flux_util.c:771-780): float32 differences, the quotient and the correction in double
__device__ __forceinline__ float hr_interp(float v1, float v2, float v3) {
#pragma clang fp contract(off)
    const float num = v3 - v1;
    const float den = 2 * (2 * v2 - v3 - v1);
    const float p = (float)((double)num / ((double)den + 1e-16));
    const float d = v1 - v3;
    return (float)((double)v2 - 0.25 * (double)d * (double)p);
}

// one frame by the calling workgroup; given < 0: find the crossing and record it, else minIndex = given
template <int R>
__device__ __forceinline__ void hr_frame(const AfxHarmonicRatioArgs &a, long long row, int given, unsigned char *smem) {
    using C = AfxPitchLagCfg<R>;
    constexpr int L = C::L, N = L / 2, NT = C::NT, PER = N / NT;  // NT * PER == N: every thread holds PER samples
    float *red = reinterpret_cast<float *>(smem);                 // [0, 32): the scan's wave totals, then the argmax
    int *redi = reinterpret_cast<int *>(smem);                    // [32, 48): the crossing of each wave
    float2 *s = reinterpret_cast<float2 *>(smem + 256);           // transform buffer of L points, afx_lds_pad addressing
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);  // W_L^m, m < L / 2
    const int maxLength = a.maxLength;
    int b, t;
    const float *x = afx_pitch_row(a.x, row, a.timeLength, a.clipStride, a.hop, b, t);

    // 1. the windowed frame, its zero padding, the thread's running sum of squares
    float cum[PER];
    float run = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int j = tid * PER + k;
        const float v = x[j] * a.window[j];
        s[afx_lds_pad(j)] = make_float2(v, 0.f);
        s[afx_lds_pad(j + N)] = make_float2(0.f, 0.f);
        run += v * v;
        cum[k] = run;
    }
    float incl = run;  // over the wave, inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    float before = __shfl_up(incl, 1);
    if (lane == 0) before = 0.f;
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) before += red[w];
#pragma unroll
    for (int k = 0; k < PER; ++k) cum[k] += before;
    afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);  // X[k] at s[bitrev(k)]

    // 2. |X|^2 back in natural order: the pair (i, bitrev(i)) belongs to the thread that holds the smaller one
    for (int i = tid; i < L; i += NT) {
        const int j = (int)(__brev((unsigned)i) >> (32 - R));
        if (i <= j) {
            const float2 u = s[afx_lds_pad(i)], v = s[afx_lds_pad(j)];  // X[j], X[i]
            s[afx_lds_pad(i)] = make_float2(v.x * v.x + v.y * v.y, 0.f);
            s[afx_lds_pad(j)] = make_float2(u.x * u.x + u.y * u.y, 0.f);
        }
    }
    __syncthreads();
    afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);  // L r[n] = Re s[bitrev(n)]

    // 3. cum beside it, 4. the first crossing (reads real halves only)
#pragma unroll
    for (int k = 0; k < PER; ++k) s[afx_lds_pad(tid * PER + k)].y = cum[k];
    const float invL = 1.f / (float)L;
    if (given < 0) {
        int mine = AFX_PITCH_NONE;
        for (int j = 2 + tid; j <= maxLength; j += NT) {  // j <= maxLength <= N - 1
            const float u = hr_lag<R>(s, j, invL), v = hr_lag<R>(s, j - 1, invL);
            if ((u >= 0.f && v <= 0.f) || (u <= 0.f && v >= 0.f)) {
                mine = j;
                break;  // rising order: the thread's first
            }
        }
#pragma unroll
        for (int msk = 32; msk > 0; msk >>= 1) mine = min(mine, __shfl_xor(mine, msk));
        if (lane == 0) redi[32 + wave] = mine;
    }
    __syncthreads();
    int minIndex = given, found = AFX_HARMONIC_RATIO_NONE;
    if (given < 0) {
        int m = AFX_PITCH_NONE;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) m = min(m, redi[32 + w]);
        if (m != AFX_PITCH_NONE) found = m - 1;
        minIndex = m != AFX_PITCH_NONE ? m - 1 : 0;
    }

    // 5. g over minIndex + 1 ... maxLength - 1 (zeros below), the thread's first maximum
    const float r0 = s[afx_lds_pad(0)].x * invL;
    float bv = -__builtin_huge_valf();
    int bi = AFX_PITCH_NONE;
    for (int j = tid; j < maxLength; j += NT) {  // j <= N - 2: c[j] = cum[N - 2 - j] exists
        const float g = j > minIndex ? hr_gamma<R>(s, j, r0, invL) : 0.f;
        if (a.curve) a.curve[row * maxLength + j] = g;
        AFX_PITCH_CANDIDATE(bv, bi, g, j, minIndex + 1)
    }
    AFX_PITCH_ARGMAX(NT, bv, bi, red, tid, lane, wave)
    if (tid == 0) {
        float out = 0.f;  // an empty range: __vmax returns -1 and leaves the value 0
        int lag = -1;
        if (bi != AFX_PITCH_NONE) {
            lag = bi;
            out = bv;
            if (bi != minIndex + 1 && bi != maxLength - 1)  // minIndex + 2 <= bi <= maxLength - 2
                out = hr_interp(hr_gamma<R>(s, bi - 1, r0, invL), bv, hr_gamma<R>(s, bi + 1, r0, invL));
        }
        const long long at = (long long)b * a.outStride + t;
        if (a.value) a.value[at] = out;
        if (a.lag) a.lag[at] = lag;
        if (a.first) a.first[at] = minIndex;
        if (given < 0) a.scratch[row] = found;
    }
}

// REDO = false: every frame, row = workgroup.  REDO = true: the same grid, but workgroup i runs the i-th listed frame with the
// inherited minIndex and the workgroups beyond the list leave at once (an empty workgroup costs less than 1 % of a frame: the
// launch needs no count on the host and no loop, whose hoisted values cost a fifth of the occupancy)
template <int R, bool REDO>
__global__ void __launch_bounds__(AfxPitchLagCfg<R>::NT) k_harmonic_ratio(AfxHarmonicRatioArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const long long rows = (long long)a.batch * a.timeLength;
    if (REDO) {
        if ((int)blockIdx.x >= a.scratch[2 * rows]) return;
        const int row = a.scratch[rows + blockIdx.x];
        hr_frame<R>(a, row, a.scratch[row], smem_raw);
    } else {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.scratch[2 * rows] = 0;  // the list is empty
        hr_frame<R>(a, blockIdx.x, -1, smem_raw);
    }
}

// One wave per clip over its records: frames[t] >= 0 is the minIndex frame t found.  A frame without one (NONE) used 0; it
// inherits the last value found before it in the clip, and when that is not 0 the value replaces its record and its row joins
// the list (rows in any order: count is the only word two waves share).
__global__ void __launch_bounds__(64) k_harmonic_ratio_resolve(int *scratch, int batch, int timeLength) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long rows = (long long)batch * timeLength;
    int *frames = scratch + (long long)b * timeLength, *list = scratch + rows, *count = scratch + 2 * rows;
    int carry = 0;
    for (int t0 = 0; t0 < timeLength; t0 += 64) {
        const int t = t0 + lane;
        const int own = t < timeLength ? frames[t] : AFX_HARMONIC_RATIO_NONE;
        int v = own;  // the last record >= 0 at or before this lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d && v < 0) v = o;
        }
        if (v < 0) v = carry;
        carry = __shfl(v, 63);
        const int redo = t < timeLength && own < 0 && v != 0;
        if (redo) frames[t] = v;
        int incl = redo;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        const int total = __shfl(incl, 63);
        if (total) {
            int base = 0;
            if (lane == 63) base = atomicAdd(count, total);
            base = __shfl(base, 63);
            if (redo) list[base + incl - 1] = (int)((long long)b * timeLength + t);
        }
    }
}

template <int R>
int launch(const AfxHarmonicRatioArgs &a, long long rows, void *stream) {
    using C = AfxPitchLagCfg<R>;
    const size_t lds = (size_t)afx_pitch_lag_lds_bytes(R - 1);
    AFX_LAUNCH_DYN_LDS((k_harmonic_ratio<R, false>), dim3((unsigned)rows), dim3(C::NT), lds, stream, a);
    AFX_LAUNCH_CHECK("k_harmonic_ratio");
    hipLaunchKernelGGL(k_harmonic_ratio_resolve, dim3((unsigned)a.batch), dim3(64), 0, (hipStream_t)stream, a.scratch, a.batch,
                       a.timeLength);
    AFX_LAUNCH_CHECK("k_harmonic_ratio_resolve");
    AFX_LAUNCH_DYN_LDS((k_harmonic_ratio<R, true>), dim3((unsigned)rows), dim3(C::NT), lds, stream, a);
    AFX_LAUNCH_CHECK("k_harmonic_ratio (listed frames)");
    return AFX_OK;
}

}  // namespace

extern "C" int afxk_harmonic_ratio(const AfxHarmonicRatioArgs *a, void *stream) {
    if (!a || !a->x || !a->window || !a->twiddle || !a->scratch || a->batch <= 0 || a->timeLength <= 0 || a->hop <= 0) return AFX_ERR_ARG;
    if (a->radix2Exp < AFX_PITCH_LAG_MIN_EXP || a->radix2Exp > AFX_PITCH_LAG_MAX_EXP) return AFX_ERR_UNSUPPORTED;
    const int N = 1 << a->radix2Exp;
    // the limits the kernel's indexing rests on
    if (a->maxLength < 2 || a->maxLength > N - 1) return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    if (a->clipStride < a->dataLength && a->batch > 1) return AFX_ERR_ARG;
    if ((a->value || a->lag || a->first) && a->outStride < a->timeLength) return AFX_ERR_ARG;
    if (!a->value && !a->lag && !a->first && !a->curve) return AFX_OK;
    const long long rows = (long long)a->batch * a->timeLength;
    if (rows > 0x7fffffffLL) {
        afxdev_set_error("harmonic ratio: %lld frames in one launch", rows);
        return AFX_ERR_UNSUPPORTED;
    }
    switch (a->radix2Exp) {
        case 6: return launch<7>(*a, rows, stream);
        case 7: return launch<8>(*a, rows, stream);
        case 8: return launch<9>(*a, rows, stream);
        case 9: return launch<10>(*a, rows, stream);
        case 10: return launch<11>(*a, rows, stream);
        case 11: return launch<12>(*a, rows, stream);
        default: return launch<13>(*a, rows, stream);
    }
}
