// afx_pitch_hs.hip -- harmonic-product-spectrum and log-harmonic-sum pitch tracking (include/mir/_pitch_hps.h,
// include/mir/_pitch_lhs.h), one launch from samples to (fre, value[, curve]).
//
// One workgroup per frame; frames carry no state from one to the next (_pitch_hps.c:467-490, _pitch_lhs.c:453-504).  The
// reference transforms every frame zero-padded to M = roundPowerTwo(samplate) points and reads bins 0 ... maxIndex *
// harmonicCount of it.  Here, with N = fftLength, D = M / N and w = e^{-2 pi i / M}:
//   1. X[p D + q] = sum_n (x[n] w^{n q}) e^{-2 pi i n p / N}: the M-point spectrum of the padded frame is D modulated
//      N-point transforms, one per residue q, each run in LDS (afx_ldsfft.h).  x is real, so |X[p D + (D - q)]| =
//      |Y_q[N - 1 - p]| with Y_q the transform of residue q: residues 0 ... D / 2 give all D;
//   2. the modulator w^{n q} is read from a table of the M-th roots (evaluated in double on the host) at the exact integer
//      (n q) mod M -- no phase is accumulated in float32;
//   3. after each transform the magnitudes sqrtf(re^2 + im^2) (LHS: their logf) of the bins m <= maxIndex * harmonicCount
//      go into the spectrum slice: LDS when it fits beside the transform buffer and the frame, else this workgroup's slice
//      of the object's device scratch (the host plan decides; the workgroups then stride over the frames);
//   4. curve[j], j <= maxIndex: product / sum over k = 0 ... harmonicCount - 1 of slice[j (k + 1)] in that order, each
//      thread striding over j -- a function of the slice alone;
//   5. first argmax over minIndex ... maxIndex (afx_pitchparts.h): rows of zeros or of -inf come out as minIndex;
//   6. fre = (index + 1) * (1.0 * samplate / M), the factor in double as the reference computes it.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_pitchparts.h"

namespace {

template <int R>
struct HsCfg {
    static constexpr int N = 1 << R;
    // threads: one radix-4 butterfly each per pass of the transform.  The slice leaves room for one to three workgroups per
    // CU, so the waves that hide LDS and barrier latency have to come from inside the workgroup (YIN's N / 16 measured 2.3 to
    // 4.4 times below YIN's own rate per transform here: profiles/pitch_hs_mi355x.txt)
    static constexpr int NT = N / 4 < 64 ? 64 : (N / 4 > 1024 ? 1024 : N / 4);
    static constexpr int PER = N / NT;
};

__device__ __forceinline__ int hs_skew(int m) { return m + (m >> 5); }  // afx_pitch_hs_slice_floats

template <int R, bool LOG>
__global__ void __launch_bounds__(HsCfg<R>::NT) k_pitch_hs(AfxPitchHsArgs a, long long rows) {
    using C = HsCfg<R>;
    constexpr int N = C::N, NT = C::NT, PER = C::PER;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *red = reinterpret_cast<float *>(smem_raw);                 // [32]: cross-wave exchange of the reduction
    float2 *s = reinterpret_cast<float2 *>(smem_raw + 128);           // transform buffer, afx_lds_pad addressing
    float *xw = reinterpret_cast<float *>(s + afx_lds_padded_size(N));  // the windowed frame
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lastBin = a.maxIndex * a.harmonicCount;
    float *slice = a.slice ? a.slice + (long long)blockIdx.x * (hs_skew(lastBin) + 1) : xw + N;
    const int M = 1 << a.interpExp, D = M >> R;
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);
    const float2 *roots = reinterpret_cast<const float2 *>(a.roots);
    const int minIndex = a.minIndex, maxIndex = a.maxIndex, H = a.harmonicCount;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        int b, t;
        const float *x = afx_pitch_row(a.x, row, a.timeLength, a.clipStride, a.hop, b, t);

        // 1. the windowed frame (neighbouring frames overlap: re-read through L2)
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int n = tid + NT * i;
            xw[n] = x[n] * a.window[n];
        }
        __syncthreads();

        // 2. residues q = 0 ... D / 2 of the M-point spectrum; each fills its bins p D + q and their mirror images
        for (int q = 0; q <= (D >> 1); ++q) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int n = tid + NT * i;
                const float v = xw[n];
                const float2 w = roots[(n * q) & (M - 1)];  // n q < 2^13 2^17
                s[afx_lds_pad(n)] = make_float2(v * w.x, v * w.y);
            }
            __syncthreads();
            afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);  // Y_q[p] at s[bitrev(p)]
            const bool mirror = q > 0 && 2 * q < D;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int p = tid + NT * i;
                const float2 y = s[afx_lds_pad((int)(__brev((unsigned)p) >> (32 - R)))];
                float mag = sqrtf(y.x * y.x + y.y * y.y);
                if (LOG) mag = logf(mag);
                const int m = p * D + q;  // < M
                if (m <= lastBin) slice[hs_skew(m)] = mag;
                if (mirror) {
                    const int m2 = (N - 1 - p) * D + (D - q);
                    if (m2 <= lastBin) slice[hs_skew(m2)] = mag;
                }
            }
            __syncthreads();
        }

        // 3. the curve over 0 ... maxIndex in the reference's operation order, the thread's first maximum from minIndex on
        float bv = -__builtin_huge_valf();
        int bi = AFX_PITCH_NONE;
        for (int j = tid; j <= maxIndex; j += NT) {
            float c = LOG ? 0.f : 1.f;
            for (int k = 0; k < H; ++k) {
                const float v = slice[hs_skew(j * (k + 1))];
                c = LOG ? c + v : c * v;
            }
            if (a.curve) a.curve[row * (maxIndex + 1) + j] = c;
            AFX_PITCH_CANDIDATE(bv, bi, c, j, minIndex)
        }

        // 4. over the workgroup: the larger value, the smaller index among equal ones
        AFX_PITCH_ARGMAX(NT, bv, bi, red, tid, lane, wave)
        if (tid == 0) {
            if (bi == AFX_PITCH_NONE) bi = minIndex;  // no candidate at all (minIndex > maxIndex)
            const long long at = (long long)b * a.outStride + t;
            if (a.fre) a.fre[at] = (float)((double)(bi + 1) * a.freStep);
            if (a.value) a.value[at] = bv;
        }
        __syncthreads();  // red, xw and the slice are free for the next frame
    }
}

template <int R, bool LOG>
int launch2(const AfxPitchHsArgs &a, long long rows, void *stream) {
    using C = HsCfg<R>;
    const long long lds = afx_pitch_hs_lds_fixed(R) + (a.slice ? 0 : 4 * afx_pitch_hs_slice_floats(a.maxIndex * a.harmonicCount));
    const unsigned grid = (unsigned)(a.slice ? a.groups : rows);
    // the limit is raised once per instantiation and device: to the budget, since the slice differs from plan to plan
    if (const int st = afx_dyn_lds<k_pitch_hs<R, LOG>>(AFX_PITCH_HS_LDS_BUDGET)) return st;
    hipLaunchKernelGGL((k_pitch_hs<R, LOG>), dim3(grid), dim3(C::NT), (size_t)lds, (hipStream_t)stream, a, rows);
    AFX_LAUNCH_CHECK("k_pitch_hs");
    return AFX_OK;
}

template <int R>
int launch(const AfxPitchHsArgs &a, long long rows, void *stream) {
    return a.kind == AFX_PITCH_LHS ? launch2<R, true>(a, rows, stream) : launch2<R, false>(a, rows, stream);
}

}  // namespace

extern "C" int afxk_pitch_hs(const AfxPitchHsArgs *a, void *stream) {
    if (!a || !a->x || !a->window || !a->twiddle || !a->roots || a->batch <= 0 || a->timeLength <= 0 || a->hop <= 0)
        return AFX_ERR_ARG;
    if (a->kind != AFX_PITCH_HPS && a->kind != AFX_PITCH_LHS) return AFX_ERR_ARG;
    if (a->radix2Exp < 6 || a->radix2Exp > 13) return AFX_ERR_UNSUPPORTED;
    const int N = 1 << a->radix2Exp;
    // the limits the kernel's indexing rests on
    if (a->interpExp < a->radix2Exp || a->interpExp > 18 || a->minIndex < 0 || a->maxIndex < 0 || a->harmonicCount < 1 ||
        (long long)a->maxIndex * a->harmonicCount >= (1LL << a->interpExp))
        return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    if ((a->fre || a->value) && a->outStride < a->timeLength) return AFX_ERR_ARG;
    const long long rows = (long long)a->batch * a->timeLength;
    const long long sliceB = 4 * afx_pitch_hs_slice_floats((long long)a->maxIndex * a->harmonicCount);
    if (a->slice) {
        if (a->groups < 1 || a->groups > AFX_PITCH_HS_SCRATCH_GROUPS || a->groups > rows) return AFX_ERR_ARG;
    } else if (afx_pitch_hs_lds_fixed(a->radix2Exp) + sliceB > AFX_PITCH_HS_LDS_BUDGET) {
        return AFX_ERR_ARG;
    }
    if (!a->fre && !a->value && !a->curve) return AFX_OK;
    if (rows > 0x7fffffffLL) {
        afxdev_set_error("pitch: %lld frames in one launch", rows);
        return AFX_ERR_UNSUPPORTED;
    }
    switch (a->radix2Exp) {
        case 6: return launch<6>(*a, rows, stream);
        case 7: return launch<7>(*a, rows, stream);
        case 8: return launch<8>(*a, rows, stream);
        case 9: return launch<9>(*a, rows, stream);
        case 10: return launch<10>(*a, rows, stream);
        case 11: return launch<11>(*a, rows, stream);
        case 12: return launch<12>(*a, rows, stream);
        default: return launch<13>(*a, rows, stream);
    }
}
