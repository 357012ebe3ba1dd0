// afx_st.hip -- the rows of the S-transform (include/st_algorithm.h).
//
// The spectrum F of a chunk comes from afxk_nsgt_spectrum (afx_cwt.hip: transposed layout).  The reference (st_algorithm.c)
// computes, per requested bin k != 0,
//   row[n] = 1/N sum_j F[(k + j) mod N] W_k[j] e^{+2 pi i j n / N},   W_k[j] = exp(c_k j^2) + exp(c_k (j - N)^2)
// from an (N/2 + 1) x N table of W.  Here W is evaluated where it is used, from the one float c_k per bin and with the
// reference's float sequence (j^2 rounded to float, one multiply, expf, one add), so a row costs its 8 N bytes of spectrum
// -- the same for every row of a chunk: L2 -- and its 8 N bytes of output.
//   k_st_rows   one workgroup per (row, chunk): the spectrum is read in its memory order (coalesced) and lands, conjugated
//               and windowed, at its rotated position in LDS; the project's LDS FFT (afx_ldsfft.h, forward, bit-reversed
//               result); conjugate and 1/N on the way out, 4 consecutive columns of both planes per lane.  Bin 0 is the
//               mean of the chunk, Re F[0] / N, in every column.
// Threads per workgroup: a pass of the transform is N/4 four-point butterflies, and one butterfly per thread and pass is what
// the LDS transform ran fastest with elsewhere (profiles/pitch_hs_mi355x.txt: n_fft/4 threads against n_fft/16, 2.3-4.4x).  So
// N/4 threads, at least a wave (2^4 and 2^6 have fewer points than a wave has lanes), at most 1024: 2^12 runs two workgroups
// (34 KB of LDS each) = 32 waves a CU; at 2^14 the 135 KB buffer leaves one workgroup per CU, whose 16 waves are then all that
// keeps LDS reads in flight.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"

namespace {

constexpr int ST_MAX_THREADS = 1024;
constexpr int ST_MAX_LDS = (int)sizeof(float2) * afx_lds_padded_size(1 << AFX_FST_MAX_EXP);
// float expf is 0 below ln 2^-150 = -103.97...: such a term adds nothing to the reference's table either
constexpr float ST_EXP_ZERO = -104.0f;
typedef float st_f4 __attribute__((ext_vector_type(4)));

// one float multiply, never half of a fused multiply-add
__device__ __forceinline__ float st_mul(float a, float b) {
#ifdef AFX_HOST_EMULATION
    volatile float p = a * b;
    return p;
#else
    return __fmul_rn(a, b);
#endif
}

__device__ __forceinline__ float st_window(float c, int j, int N) {
    const float a = (float)j, b = (float)(j - N);
    const float xa = st_mul(st_mul(a, a), c), xb = st_mul(st_mul(b, b), c);
    return (xa < ST_EXP_ZERO ? 0.f : expf(xa)) + (xb < ST_EXP_ZERO ? 0.f : expf(xb));
}

template <bool VEC, bool STREAM>
__device__ __forceinline__ void st_store4(float *p, float v0, float v1, float v2, float v3) {
    if (VEC) {
        const st_f4 q = {v0, v1, v2, v3};
        if (STREAM) __builtin_nontemporal_store(q, reinterpret_cast<st_f4 *>(p));
        else *reinterpret_cast<st_f4 *>(p) = q;
    } else {
        p[0] = v0, p[1] = v1, p[2] = v2, p[3] = v3;
    }
}

template <bool VEC, bool STREAM>
__global__ __launch_bounds__(ST_MAX_THREADS) void k_st_rows(AfxStArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const int tid = threadIdx.x, nth = blockDim.x, row = blockIdx.x, chunk = blockIdx.y;
    const int r = a.r1 + a.r2, N = 1 << r, m2 = (1 << a.r2) - 1;
    const float2 *X = reinterpret_cast<const float2 *>(a.Xt) + (long long)chunk * N;
    const long long outAt = ((long long)chunk * a.rows + row) << r;
    float *oRe = a.outRe + outAt, *oIm = a.outIm + outAt;
    const int k = a.bins[row];
    const float invN = 1.0f / (float)N;
    if (k == 0) {
        const float mean = X[0].x * invN;
        for (int q = tid; q < (N >> 2); q += nth) {
            st_store4<VEC, STREAM>(oRe + 4 * q, mean, mean, mean, mean);
            st_store4<VEC, STREAM>(oIm + 4 * q, 0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const float c = a.coef[k];
    for (int m = tid; m < N; m += nth) {  // m = (k1 << r2) | k2 holds frequency k1 + (k2 << r1)
        const int f = (m >> a.r2) | ((m & m2) << a.r1);
        const int j = (f - k) & (N - 1);
        const float w = st_window(c, j, N);
        const float2 x = X[m];
        s[afx_lds_pad(j)] = make_float2(x.x * w, -x.y * w);  // inverse transform = conj(forward(conj))
    }
    __syncthreads();
    afx_lds_fft_dif_t<true>(s, r, reinterpret_cast<const float2 *>(a.twiddle), 1, tid, nth);
    for (int q = tid; q < (N >> 2); q += nth) {
        const int n = 4 * q;
        const float2 g0 = s[afx_lds_pad((int)(__brev((unsigned)n) >> (32 - r)))];
        const float2 g1 = s[afx_lds_pad((int)(__brev((unsigned)n + 1u) >> (32 - r)))];
        const float2 g2 = s[afx_lds_pad((int)(__brev((unsigned)n + 2u) >> (32 - r)))];
        const float2 g3 = s[afx_lds_pad((int)(__brev((unsigned)n + 3u) >> (32 - r)))];
        st_store4<VEC, STREAM>(oRe + n, g0.x * invN, g1.x * invN, g2.x * invN, g3.x * invN);
        st_store4<VEC, STREAM>(oIm + n, -g0.y * invN, -g1.y * invN, -g2.y * invN, -g3.y * invN);
    }
}

template <bool VEC, bool STREAM>
int st_launch(const AfxStArgs *a, int threads, size_t lds, void *stream) {
    if (const int st = afx_dyn_lds<k_st_rows<VEC, STREAM>>(ST_MAX_LDS)) return st;  // one latch: the largest size
    hipLaunchKernelGGL((k_st_rows<VEC, STREAM>), dim3(a->rows, a->chunks), dim3(threads), lds, (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_st_rows");
    return AFX_OK;
}

}  // namespace

extern "C" int afxk_st_rows(const AfxStArgs *a, void *stream) {
    if (!a || !a->Xt || !a->twiddle || !a->coef || !a->bins || !a->outRe || !a->outIm || a->rows <= 0) return AFX_ERR_ARG;
    const int r = a->r1 + a->r2;
    if (a->r1 < 1 || a->r2 < 1 || r < AFX_FST_MIN_EXP || r > AFX_FST_MAX_EXP) return AFX_ERR_ARG;
    if (a->chunks <= 0) return AFX_OK;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const int threads = r <= 8 ? 64 : r >= 12 ? ST_MAX_THREADS : 1 << (r - 2);
    const size_t lds = sizeof(float2) * (size_t)afx_lds_padded_size(1 << r);
    const bool vec = ((size_t)a->outRe | (size_t)a->outIm) % 16 == 0;
    const bool big = 8ll * a->chunks * ((long long)a->rows << r) > AFX_FST_STREAM_BYTES;
    if (!vec) return st_launch<false, false>(a, threads, lds, stream);
    if (big) return st_launch<true, true>(a, threads, lds, stream);
    return st_launch<true, false>(a, threads, lds, stream);
}
