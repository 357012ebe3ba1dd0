// afx_phasevocoder.hip -- the phase vocoder between a forward and an inverse STFT (include/mir/timeStretch_algorithm.h):
// output frame i of a clip sits at t = i * rate between the input frames k = floor(t) and k + 1; its magnitudes are
// interpolated, its phases are accumulated from the wrapped phase differences of those two frames
// (phase_vocoder.c:19-120).
//
// Three launches (AfxPhaseVocoderArgs, afx_device.h):
//   k_pv_polar      mag / ang of every input bin, once per input frame (the reference recomputes them per output frame)
//   k_pv_phase      one lane per (clip, bin): the float32 accumulator of the reference, serial over the output frames.  The
//                   increments phi + wrap(.) depend on the input angles alone, so their loads and the float64 wrap run ahead
//                   of the chain, which carries one float32 add per frame.  Neighbouring lanes own neighbouring bins: every
//                   load and store of a wave is one contiguous run.  The phases are parked in outRe[i][j], j <= N / 2.
//   k_pv_synthesis  (clip, i, j) in parallel: interpolated magnitude times (cosf, sinf)(phase), the phase word replaced by the
//                   real part in place, the imaginary part and the conjugate mirror N - j stored beside it.
// The accumulator is ill-conditioned by construction (it passes 1e5 rad, where one float32 ulp is 0.008 rad), so every
// operation keeps the reference's order and width: no fused multiply-add (the pragma below), no wrapped or float64
// accumulator, sincosf with full range reduction.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"

#pragma clang fp contract(off)

namespace {

constexpr int PV_NT = 256;
constexpr int PV_AHEAD = 8;  // steps of the phase chain whose increments are formed together

__global__ void __launch_bounds__(PV_NT) k_pv_polar(AfxPhaseVocoderArgs a, int F, long long total) {
    for (long long idx = (long long)blockIdx.x * PV_NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * PV_NT) {
        const long long row = idx / F;
        const int j = (int)(idx - row * F);
        const float re = a.re[row * a.inPitch + j], im = a.im[row * a.inPitch + j];
        a.mag[idx] = sqrtf(re * re + im * im);
        a.ang[idx] = atan2f(im, re);
    }
}

// the value of frame k of the clip whose frames start at `plane`; a frame at or beyond T1 is all zeros
__device__ __forceinline__ float frame_value(const float *plane, int k, int T1, int F, int j) {
    return k < T1 ? plane[(long long)k * F + j] : 0.f;
}

__global__ void __launch_bounds__(PV_NT) k_pv_phase(AfxPhaseVocoderArgs a, int F, int N) {
    const int j = blockIdx.x * PV_NT + threadIdx.x;
    if (j >= F) return;
    const long long b = blockIdx.y;
    // (restrict: the angles are never the output planes, so the loads of the next steps may pass the stores of these)
    const float *__restrict__ ang = a.ang + b * a.T1 * F;
    float *__restrict__ out = a.outRe + b * a.T2 * N + j;
    const float phi = 0.f + (float)j * afx_pv_phi_step(a.hop, F);
    float phase = ang[j];
    const int last = a.T1 - 1;
    for (int i0 = 0; i0 < a.T2; i0 += PV_AHEAD) {
        // the increments of PV_AHEAD steps: unconditional loads from clamped rows, so that all of them are in flight together
        float d[PV_AHEAD];
#pragma unroll
        for (int u = 0; u < PV_AHEAD; ++u) {
            float alpha;
            const int k = afx_pv_time(i0 + u, a.rate, &alpha);
            const float l1 = ang[(long long)(k < last ? k : last) * F + j], l2 = ang[(long long)(k + 1 < last ? k + 1 : last) * F + j];
            const float a1 = k < a.T1 ? l1 : 0.f, a2 = k + 1 < a.T1 ? l2 : 0.f;  // a frame at or beyond T1 is all zeros: angle 0
            float v = a2 - a1 - phi;
            v = (float)((double)v - 2 * M_PI * roundf((float)((double)v / (2 * M_PI))));
            d[u] = phi + v;
        }
        // the chain: one float32 add per step
#pragma unroll
        for (int u = 0; u < PV_AHEAD; ++u)
            if (i0 + u < a.T2) {
                out[(long long)(i0 + u) * N] = phase;
                phase += d[u];
            }
    }
}

__global__ void __launch_bounds__(PV_NT) k_pv_synthesis(AfxPhaseVocoderArgs a, int F, int N, long long total) {
    for (long long idx = (long long)blockIdx.x * PV_NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * PV_NT) {
        const long long row = idx / F;  // b * T2 + i
        const int j = (int)(idx - row * F);
        const long long b = row / a.T2;
        const int i = (int)(row - b * a.T2);
        float alpha;
        const int k = afx_pv_time(i, a.rate, &alpha);
        const float *mag = a.mag + b * a.T1 * F;
        const float m1 = frame_value(mag, k, a.T1, F, j) * (1 - alpha), m2 = frame_value(mag, k + 1, a.T1, F, j) * alpha;
        const float m = m1 + m2;
        float *re = a.outRe + row * N, *im = a.outIm + row * N;
        float s, c;
        sincosf(re[j], &s, &c);
        const float vr = m * c, vi = m * s;
        re[j] = vr;
        im[j] = vi;
        if (j > 0 && j < N - j) {
            re[N - j] = vr;
            im[N - j] = -vi;
        }
    }
}

__global__ void __launch_bounds__(PV_NT) k_rows_fit(const float *src, long long srcStride, int srcLength, float *dst, long long dstStride,
                                                    int length, long long total) {
    for (long long idx = (long long)blockIdx.x * PV_NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * PV_NT) {
        const long long b = idx / length;
        const int i = (int)(idx - b * length);
        dst[b * dstStride + i] = i < srcLength ? src[b * srcStride + i] : 0.f;
    }
}

// workgroups of a grid-stride launch over `total` elements
unsigned flat_grid(long long total) {
    const long long want = (total + PV_NT - 1) / PV_NT, cap = (long long)afx_cu_count() * 32;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace

extern "C" int afxk_phase_vocoder(const AfxPhaseVocoderArgs *a, void *stream) {
    if (!a || !a->re || !a->im || !a->mag || !a->ang || !a->outRe || !a->outIm) return AFX_ERR_ARG;
    if (a->radix2Exp < 1 || a->radix2Exp > 14 || a->hop <= 0 || a->batch <= 0 || a->batch > 65535 || a->T1 <= 0) return AFX_ERR_ARG;
    const int N = 1 << a->radix2Exp, F = N / 2 + 1;
    if (a->T2 <= 0 || a->T2 != afx_pv_frames(a->T1, a->rate) || a->inPitch < F) return AFX_ERR_ARG;
    const long long in = (long long)a->batch * a->T1 * F, out = (long long)a->batch * a->T2 * F;
    hipLaunchKernelGGL(k_pv_polar, dim3(flat_grid(in)), dim3(PV_NT), 0, (hipStream_t)stream, *a, F, in);
    AFX_LAUNCH_CHECK("k_pv_polar");
    hipLaunchKernelGGL(k_pv_phase, dim3((F + PV_NT - 1) / PV_NT, a->batch), dim3(PV_NT), 0, (hipStream_t)stream, *a, F, N);
    AFX_LAUNCH_CHECK("k_pv_phase");
    hipLaunchKernelGGL(k_pv_synthesis, dim3(flat_grid(out)), dim3(PV_NT), 0, (hipStream_t)stream, *a, F, N, out);
    AFX_LAUNCH_CHECK("k_pv_synthesis");
    return AFX_OK;
}

extern "C" int afxk_rows_fit(const float *src, long long srcStride, int srcLength, float *dst, long long dstStride, int length, int batch,
                             void *stream) {
    if (!src || !dst || srcLength < 0 || length <= 0 || batch <= 0) return AFX_ERR_ARG;
    if (batch > 1 && (srcStride < (srcLength < length ? srcLength : length) || dstStride < length)) return AFX_ERR_ARG;
    const long long total = (long long)batch * length;
    hipLaunchKernelGGL(k_rows_fit, dim3(flat_grid(total)), dim3(PV_NT), 0, (hipStream_t)stream, src, srcStride, srcLength, dst, dstStride,
                       length, total);
    AFX_LAUNCH_CHECK("k_rows_fit");
    return AFX_OK;
}
