// afx_nsgt.hip -- the per-band half of the non-stationary Gabor transform (include/nsgt_algorithm.h).
//
// The spectrum X of a chunk comes from afxk_nsgt_spectrum (afx_cwt.hip: the CWT's forward pass, transposed layout).  For
// band i of length L, offset o and window w (nsgt_algorithm.c:545-604):
//   z[(L - L/2 + j) mod L] = X[clamp(o + j, 0, N - 1)] w[j],  j < L          window multiply + rotation
//   cell_i[n] = 1/L sum_k z[k] e^{+2 pi i k n / L},            n < L          inverse DFT of the band's OWN length
//   matrix[i][col] = cell_i[colMap[i][col]]                                   sample-and-hold onto maxLength columns
// L is arbitrary (1 ... N, mostly odd), so the inverse is a direct O(L^2) DFT -- what the reference does serially in double
// with an L x L table per length; here one wave per (band, chunk, block of AFX_NSGT_BLOCK outputs):
//   * the wave forms the band's z ONCE in its LDS share (tiles of AFX_NSGT_TILE for longer bands); in the k loop all 64
//     lanes read the same z[k] in the same step (a broadcast read);
//   * lane l owns outputs n = n0 + l + 64 a, a < A <= 4, accumulators in registers, float32;
//   * the phase index (k n) mod L is an INTEGER per output, advanced by add + conditional subtract, and the twiddle is
//     read from the length's table T_L (evaluated in double on the host) -- from LDS when L <= AFX_NSGT_TILE: no rotation
//     recurrence, no sinf of an unreduced argument, so the error is the float32 accumulation's alone;
//   * the block's cells go to LDS, then to the cell planes (lanes along n) and, through the column map, to the matrix row
//     (lanes along the column axis): block [n0, n1) owns the columns cellCol[n0] ... cellCol[n1] - 1.
// Four waves share a workgroup but nothing else: no workgroup barrier, a wave whose item index is past the list leaves.
// Items are listed long bands first.  Short bands use one accumulator and one pass; their cost is the launch's tail.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"

namespace {

constexpr int NSGT_TILE = AFX_NSGT_TILE, NSGT_BLOCK = AFX_NSGT_BLOCK, NSGT_WAVES = 4;

struct NsgtWaveLds {
    float2 z[NSGT_TILE];      // windowed, rotated spectrum values k0 ... k0 + TILE - 1
    float2 tw[NSGT_TILE];     // T_L when L <= TILE
    float2 cell[NSGT_BLOCK];  // the block's results
};

// a wave's own LDS stores before its later LDS loads of other lanes' data (and loads before later stores): DS operations
// of one wave execute in issue order; lgkmcnt(0) drains them, the wave barrier pins the compiler
__device__ __forceinline__ void nsgt_lds_order() {
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
}

template <int A>
__device__ __forceinline__ void nsgt_block(const AfxNsgtArgs &a, const AfxNsgtBand &b, int band, int n0, int chunk,
                                           NsgtWaveLds *s, int lane) {
    const int L = b.len, N = 1 << (a.r1 + a.r2), m1 = (1 << a.r1) - 1;
    const float2 *X = reinterpret_cast<const float2 *>(a.Xt) + (long long)chunk * N;
    const float *w = a.window + b.cell;
    const float2 *T = reinterpret_cast<const float2 *>(a.twiddle) + b.twiddle;
    const bool twLds = L <= NSGT_TILE;
    if (twLds)
        for (int m = lane; m < L; m += 64) s->tw[m] = T[m];
    int n[A], p[A];
    float2 acc[A];
#pragma unroll
    for (int q = 0; q < A; ++q) {
        n[q] = n0 + lane + 64 * q;
        if (n[q] >= L) n[q] = 0;  // a lane past the band: computes output 0 again, stores nothing
        acc[q] = make_float2(0.f, 0.f);
    }
    const int half = L / 2;
    for (int k0 = 0; k0 < L; k0 += NSGT_TILE) {
        const int kn = L - k0 < NSGT_TILE ? L - k0 : NSGT_TILE;
        nsgt_lds_order();
        for (int i = lane; i < kn; i += 64) {
            int j = k0 + i + half;  // k = (L - L/2 + j) mod L  <=>  j = (k + L/2) mod L
            if (j >= L) j -= L;
            int f = b.offset + j;
            f = f < 0 ? 0 : (f > N - 1 ? N - 1 : f);
            const float2 x = X[((f & m1) << a.r2) | (f >> a.r1)];
            const float wv = w[j];
            s->z[i] = make_float2(x.x * wv, x.y * wv);
        }
        nsgt_lds_order();
#pragma unroll
        for (int q = 0; q < A; ++q) p[q] = (int)(((unsigned long long)k0 * (unsigned)n[q]) % (unsigned)L);
        for (int i = 0; i < kn; ++i) {
            const float2 z = s->z[i];
#pragma unroll
            for (int q = 0; q < A; ++q) {
                const float2 t = twLds ? s->tw[p[q]] : T[p[q]];
                acc[q].x += z.x * t.x - z.y * t.y;
                acc[q].y += z.x * t.y + z.y * t.x;
                p[q] += n[q];
                if (p[q] >= L) p[q] -= L;
            }
        }
    }
    const float invL = 1.f / (float)L;
    const long long cellAt = (long long)chunk * a.totalLength + b.cell;
#pragma unroll
    for (int q = 0; q < A; ++q) {
        const int nn = n0 + lane + 64 * q;
        if (nn < L) {
            const float2 v = make_float2(acc[q].x * invL, acc[q].y * invL);
            s->cell[lane + 64 * q] = v;
            if (a.cellRe) {
                a.cellRe[cellAt + nn] = v.x;
                a.cellIm[cellAt + nn] = v.y;
            }
        }
    }
    nsgt_lds_order();
    const int n1 = n0 + NSGT_BLOCK < L ? n0 + NSGT_BLOCK : L;
    const int *cc = a.cellCol + b.cellCol;
    const int c0 = cc[n0], c1 = cc[n1];
    const int *map = a.colMap + (long long)band * a.maxLength;
    const long long row = ((long long)chunk * a.num + band) * a.maxLength;
    for (int col = c0 + lane; col < c1; col += 64) {
        int idx = map[col] - n0;
        idx = idx < 0 ? 0 : (idx > n1 - n0 - 1 ? n1 - n0 - 1 : idx);  // (the plan keeps it inside; never leave the block)
        const float2 v = s->cell[idx];
        a.outRe[row + col] = v.x;
        a.outIm[row + col] = v.y;
    }
}

__global__ __launch_bounds__(64 * NSGT_WAVES) void k_nsgt_bands(AfxNsgtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * NSGT_WAVES + wave;
    if (item >= a.nItems) return;  // the whole wave: waves of a workgroup share no barrier
    NsgtWaveLds *s = reinterpret_cast<NsgtWaveLds *>(smem_raw) + wave;
    const int band = a.items[2 * item], n0 = a.items[2 * item + 1];
    const AfxNsgtBand b = a.bands[band];
    const int left = b.len - n0;
    if (left <= 64) nsgt_block<1>(a, b, band, n0, blockIdx.y, s, lane);
    else if (left <= 128) nsgt_block<2>(a, b, band, n0, blockIdx.y, s, lane);
    else if (left <= 192) nsgt_block<3>(a, b, band, n0, blockIdx.y, s, lane);
    else nsgt_block<4>(a, b, band, n0, blockIdx.y, s, lane);
}

}  // namespace

extern "C" int afxk_nsgt_bands(const AfxNsgtArgs *a, void *stream) {
    if (!a || !a->bands || !a->items || !a->window || !a->twiddle || !a->colMap || !a->cellCol || !a->Xt || !a->outRe ||
        !a->outIm || (a->cellRe == nullptr) != (a->cellIm == nullptr) || a->num <= 0 || a->nItems <= 0 || a->maxLength <= 0)
        return AFX_ERR_ARG;
    if (a->chunks <= 0) return AFX_OK;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const dim3 grid((a->nItems + NSGT_WAVES - 1) / NSGT_WAVES, a->chunks);
    hipLaunchKernelGGL(k_nsgt_bands, grid, dim3(64 * NSGT_WAVES), sizeof(NsgtWaveLds) * NSGT_WAVES, (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_nsgt_bands");
    return AFX_OK;
}
