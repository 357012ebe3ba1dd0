// afx_fst.hip -- the per-band half and the expansion of the fast S-transform (include/fst_algorithm.h).
//
// The spectrum F of a chunk comes from afxk_nsgt_spectrum (afx_cwt.hip: transposed layout).  The reference
// (fst_algorithm.c) works on X = fftshift(fft(ifftshift(x))) / sqrt(N): position p holds bin q = p - N/2 with the value
// (-1)^q F[q mod N] / sqrt(N).  A positive band of n = 2, 4, ..., N/4 points covers bins n ... 2n - 1 and becomes
// fftshift(ifft(ifftshift(seg))) sqrt(n).  With the shifts written out:
//   G[u]    = sum_j F[n + j] e^{+2 pi i j u / n},  u < n          the inverse DFT of the band's bins as they lie in F
//   cell[u] = (-1)^((u + n/2) mod n) G[u] / sqrt(N n)
// -- the (-1)^j of the shifted spectrum is a rotation of G by n/2, which the output fftshift undoes; what is left of both is
// one sign per output.  The three single bins -1, 0, +1 are -F[N-1], F[0], -F[1] over sqrt(N).
//   k_fst_cells   one workgroup per (band, chunk): gather (conjugated), the project's LDS FFT (afx_ldsfft.h, forward,
//                 bit-reversed result), conjugate + sign + scale on the way to the cell plane.  N/2 points per chunk.
//   k_fst_expand  matrix[k][l] = cell[first(minIndex + k) + (l >> shift(minIndex + k))]: each lane writes 4 consecutive
//                 columns of both planes.  Write-bound: 8 rows N bytes per chunk; the cells are read from L2.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"

namespace {

constexpr int FST_THREADS = 256, FST_UNROLL = 4;
typedef float fst_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(FST_THREADS) void k_fst_cells(AfxFstCellArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const int tid = threadIdx.x, b = blockIdx.x, chunk = blockIdx.y;
    const int r = a.r1 + a.r2, N = 1 << r, m1 = (1 << a.r1) - 1;
    const float2 *X = reinterpret_cast<const float2 *>(a.Xt) + (long long)chunk * N;
    const long long cellAt = (long long)chunk * (N / 2 + 1);
    const float scale = a.scale[b];
    if (b == 0) {  // bins -1, 0, +1
        if (tid < 3) {
            const int k = tid == 0 ? N - 1 : tid - 1;
            const float2 x = X[((k & m1) << a.r2) | (k >> a.r1)];
            const float sc = tid == 1 ? scale : -scale;
            a.cellRe[cellAt + tid] = x.x * sc;
            a.cellIm[cellAt + tid] = x.y * sc;
        }
        return;
    }
    const int n = 1 << b;
    for (int j = tid; j < n; j += FST_THREADS) {
        const int k = n + j;
        const float2 x = X[((k & m1) << a.r2) | (k >> a.r1)];
        s[afx_lds_pad(j)] = make_float2(x.x, -x.y);  // inverse transform = conj(forward(conj))
    }
    __syncthreads();
    afx_lds_fft_dif_t<true>(s, b, reinterpret_cast<const float2 *>(a.twiddle), N >> b, tid, FST_THREADS);
    for (int u = tid; u < n; u += FST_THREADS) {
        const float2 g = s[afx_lds_pad((int)(__brev((unsigned)u) >> (32 - b)))];
        const float sc = ((u + (n >> 1)) & 1) ? -scale : scale;
        a.cellRe[cellAt + n + 1 + u] = g.x * sc;
        a.cellIm[cellAt + n + 1 + u] = -g.y * sc;
    }
}

template <bool VEC, bool STREAM>
__device__ __forceinline__ void fst_store4(float *p, float v) {
    if (VEC) {
        const fst_f4 q = {v, v, v, v};
        if (STREAM) __builtin_nontemporal_store(q, reinterpret_cast<fst_f4 *>(p));
        else *reinterpret_cast<fst_f4 *>(p) = q;
    } else {
        p[0] = v, p[1] = v, p[2] = v, p[3] = v;
    }
}

template <bool VEC, bool STREAM>
__global__ __launch_bounds__(FST_THREADS) void k_fst_expand(AfxFstExpandArgs a) {
    const int r = a.radix2Exp, chunk = blockIdx.y;
    const long long items = (long long)a.rows << (r - 2);  // groups of 4 columns in a chunk's matrix
    const long long cellAt = (long long)chunk * ((1 << (r - 1)) + 1);
    const long long outAt = ((long long)chunk * a.rows) << r;
    const int2 *map = reinterpret_cast<const int2 *>(a.rowMap);
#pragma unroll
    for (int q = 0; q < FST_UNROLL; ++q) {
        const long long item = ((long long)blockIdx.x * FST_UNROLL + q) * FST_THREADS + threadIdx.x;
        if (item >= items) return;
        const int k = (int)(item >> (r - 2)), l = (int)(item & ((1 << (r - 2)) - 1)) << 2;
        const int2 m = map[a.minIndex + k];
        const long long c = cellAt + m.x + (l >> m.y);
        const long long at = outAt + ((long long)k << r) + l;
        fst_store4<VEC, STREAM>(a.outRe + at, a.cellRe[c]);
        fst_store4<VEC, STREAM>(a.outIm + at, a.cellIm[c]);
    }
}

}  // namespace

extern "C" int afxk_fst_cells(const AfxFstCellArgs *a, void *stream) {
    if (!a || !a->Xt || !a->twiddle || !a->cellRe || !a->cellIm) return AFX_ERR_ARG;
    const int r = a->r1 + a->r2;
    if (a->r1 < 1 || a->r2 < 1 || r < AFX_FST_MIN_EXP || r > AFX_FST_MAX_EXP) return AFX_ERR_ARG;
    if (a->chunks <= 0) return AFX_OK;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const size_t lds = sizeof(float2) * (size_t)afx_lds_padded_size(1 << (r - 2));
    hipLaunchKernelGGL(k_fst_cells, dim3(r - 1, a->chunks), dim3(FST_THREADS), lds, (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_fst_cells");
    return AFX_OK;
}

extern "C" int afxk_fst_expand(const AfxFstExpandArgs *a, void *stream) {
    if (!a || !a->rowMap || !a->cellRe || !a->cellIm || !a->outRe || !a->outIm) return AFX_ERR_ARG;
    const int r = a->radix2Exp;
    if (r < AFX_FST_MIN_EXP || r > AFX_FST_MAX_EXP || a->minIndex < 0 || a->rows <= 0 ||
        (long long)a->minIndex + a->rows > (1 << (r - 1)) + 1)
        return AFX_ERR_ARG;
    if (a->chunks <= 0) return AFX_OK;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const long long items = (long long)a->rows << (r - 2), perBlock = (long long)FST_THREADS * FST_UNROLL;
    const dim3 grid((unsigned)((items + perBlock - 1) / perBlock), a->chunks), block(FST_THREADS);
    const bool vec = ((size_t)a->outRe | (size_t)a->outIm) % 16 == 0;
    const bool big = 8ll * a->chunks * ((long long)a->rows << r) > AFX_FST_STREAM_BYTES;
    if (!vec) hipLaunchKernelGGL((k_fst_expand<false, false>), grid, block, 0, (hipStream_t)stream, *a);
    else if (big) hipLaunchKernelGGL((k_fst_expand<true, true>), grid, block, 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL((k_fst_expand<true, false>), grid, block, 0, (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_fst_expand");
    return AFX_OK;
}
