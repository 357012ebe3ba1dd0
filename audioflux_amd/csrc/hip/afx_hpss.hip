// afx_hpss.hip -- harmonic / percussive separation between the forward and the inverse STFT (afx_hpss.c), and the
// sliding-window median it is made of as a primitive of its own.
//
//   k_hpss_tile<HPSS, KH, KP>   a workgroup owns 64 frames x 128 bins of one clip.  It loads re / im of the tile plus a halo of
//                               hOrder/2 frames and pOrder/2 bins, keeps mag = sqrtf(re^2 + im^2) in an LDS tile (0 outside the
//                               clip's plane), runs the median along time (a lane per bin, window hOrder) and the median along
//                               frequency (a lane per frame, window pOrder; the odd row pitch keeps a wave's column read on 64
//                               different banks), then masks: H = h^2 / (h^2 + p^2) mag, P = p^2 / (h^2 + p^2) mag, phase
//                               re-applied, stored as full Hermitian spectra for the inverse and / or as magnitude planes.
//                               The magnitude plane and the two median planes never exist in memory
//                               (src/mir/hpss_algorithm.c:168-262, src/vector/flux_vector.c:2944-3012).
//   k_hpss_tile<AXIS0 | AXIS1>  the same tile, loads and walks for one median of a real plane (afx_medianFilterDevice).
//   k_median_rank               odd orders 65 ... 255: one output per thread by rank counting over its window.  Correct, not fast.
//
// The window of a lane lives SORTED in K registers (K a compile-time size; every index below is a constant after unrolling, so
// nothing is indexed at run time and nothing goes to scratch).  One step of the walk removes the sample that leaves and inserts the
// one that enters:
//     A[i] = w[i] < d ? w[i] : w[i + 1]          (i < K - 1)   the window without the FIRST element equal to d: d is in the window,
//                                                              bit for bit, because every element is a copy of a sample
//     w'[i] = med3(A[i - 1], A[i], n)            A[-1] = -inf, A[K - 1] = +inf: n clamped between its neighbours
// 3 K lane operations per output instead of a sort.  No arithmetic touches a sample, so the output is bit for bit the middle
// element of the sorted window.  An odd order k < K runs on the same registers with (K - k)/2 elements -inf and (K - k)/2 elements
// +inf that never leave: the middle does not move.  A walk starts from [-inf ... | +inf ...] and k - 1 insertions that each remove
// a +inf.  NaN samples: unspecified results (a comparison chain and a sort order them differently), no fault.
#include <hip/hip_runtime.h>

#include <math.h>

#include "afx_device.h"
#include "afx_hipcheck.h"

namespace {

constexpr int HP_FB = 128;   // bins of a tile (its frames, TT, are 64, or 32 where the halo of large orders would not fit the LDS)
constexpr int HP_NT = 256;   // threads: 4 waves
constexpr int HP_OP = HP_FB + 1;  // row pitch of the two median tiles
enum { HP_HPSS = 0, HP_AXIS0 = 1, HP_AXIS1 = 2 };

__device__ __forceinline__ float hp_med3(float a, float b, float c) {
#ifdef AFX_HOST_EMULATION
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
#else
    return __builtin_amdgcn_fmed3f(a, b, c);
#endif
}

// one delete-insert on the sorted window
template <int K>
__device__ __forceinline__ void hp_step(float (&w)[K], float d, float n) {
    float prev = -INFINITY;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float a = (i < K - 1) ? (w[i] < d ? w[i] : w[i + 1 < K ? i + 1 : i]) : INFINITY;
        w[i] = hp_med3(prev, a, n);
        prev = a;
    }
}

// medians of the windows src[j * ss ... (j + k - 1) * ss], j < nout -> dst[j * ds]
template <int K>
__device__ __forceinline__ void hp_walk(const float *src, int ss, int k, int nout, float *dst, int ds) {
    float w[K];
    const int pad = (K - k) >> 1;
#pragma unroll
    for (int i = 0; i < K; ++i) w[i] = i < pad ? -INFINITY : INFINITY;
    for (int i = 0; i < k - 1; ++i) hp_step<K>(w, INFINITY, src[i * ss]);
    float d = INFINITY, n = src[(k - 1) * ss];
    for (int j = 0; j < nout; ++j) {
        const float dNext = src[j * ss];
        const int jn = j + 1 < nout ? j + 1 : j;  // (the sample of the next step, fetched before this step's chain)
        const float nNext = src[(jn + k - 1) * ss];
        hp_step<K>(w, d, n);
        dst[j * ds] = w[K / 2];
        d = dNext;
        n = nNext;
    }
}

template <int MODE, int KH, int KP, int HP_TT>
__global__ __launch_bounds__(HP_NT) void k_hpss_tile(AfxHpssArgs a, int binTiles, int frameTiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *mag = reinterpret_cast<float *>(smem_raw);
    const int hh = MODE == HP_AXIS1 ? 0 : a.hOrder >> 1, ph = MODE == HP_AXIS0 ? 0 : a.pOrder >> 1;
    const int pitch = (HP_FB + 2 * ph) | 1;
    float *hm = mag + (HP_TT + 2 * hh) * pitch;  // [HP_TT][HP_OP] median along time
    float *pm = MODE == HP_HPSS ? hm + HP_TT * HP_OP : hm;  // median along frequency

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned blk = blockIdx.x;
    const int bt = (int)(blk % (unsigned)binTiles);
    const unsigned rest = blk / (unsigned)binTiles;
    const int ft = (int)(rest % (unsigned)frameTiles);
    const long long clip = rest / (unsigned)frameTiles;
    const long long row0 = clip * a.framesPerClip;            // first row of the clip
    const long long left = a.rows - row0;
    const int T = left < a.framesPerClip ? (int)left : a.framesPerClip;  // frames of this clip
    const int t0 = ft * HP_TT, b0 = bt * HP_FB;
    if (t0 >= T) return;  // (the last clip of a plane may be shorter)
    const int vt = T - t0 < HP_TT ? T - t0 : HP_TT;            // frames of the tile that exist
    const int vb = a.cols - b0 < HP_FB ? a.cols - b0 : HP_FB;  // bins of the tile that exist

    // the magnitude tile with its halo: tile row r = frame t0 - hh + r, tile column c = bin b0 - ph + c
    const int needR = vt + 2 * hh, needC = vb + 2 * ph;
    for (int r = wave; r < needR; r += HP_NT / 64) {
        const int t = t0 - hh + r;
        const bool rowIn = t >= 0 && t < T;
        const float *__restrict__ re = a.re + (row0 + t) * a.pitch;
        const float *__restrict__ im = MODE == HP_HPSS ? a.im + (row0 + t) * a.pitch : nullptr;
        for (int c = lane; c < needC; c += 64) {
            const int b = b0 - ph + c;
            float v = 0.f;
            if (rowIn && b >= 0 && b < a.cols) {
                if (MODE == HP_HPSS) {
                    const float x = re[b], y = im[b];
                    v = sqrtf(x * x + y * y);
                } else {
                    v = re[b];
                }
            }
            mag[r * pitch + c] = v;
        }
    }
    __syncthreads();

    // median along time: lane = (bin, half of the tile's frames)
    if constexpr (MODE != HP_AXIS1) {
        constexpr int SEG = HP_TT / (HP_NT / HP_FB);
        const int b = tid & (HP_FB - 1), j0 = (tid >> 7) * SEG;
        if (b < vb && j0 < vt)
            hp_walk<KH>(mag + j0 * pitch + ph + b, pitch, a.hOrder, vt - j0 < SEG ? vt - j0 : SEG, hm + j0 * HP_OP + b, HP_OP);
    }
    // median along frequency: lane = (frame, one of the NT / TT parts of the tile's bins)
    if constexpr (MODE != HP_AXIS0) {
        constexpr int SEG = HP_FB / (HP_NT / HP_TT);
        const int f = tid & (HP_TT - 1), j0 = (tid / HP_TT) * SEG;
        if (f < vt && j0 < vb)
            hp_walk<KP>(mag + (hh + f) * pitch + j0, 1, a.pOrder, vb - j0 < SEG ? vb - j0 : SEG, pm + f * HP_OP + j0, 1);
    }
    __syncthreads();

    const int N = a.fftLength;
    for (int r = wave; r < vt; r += HP_NT / 64) {
        const long long row = row0 + t0 + r;
        for (int c = lane; c < vb; c += 64) {
            const int b = b0 + c;
            if (MODE != HP_HPSS) {
                a.hMag[row * a.cols + b] = hm[r * HP_OP + c];
                continue;
            }
            const float m = mag[(hh + r) * pitch + ph + c];
            const float h = hm[r * HP_OP + c], p = pm[r * HP_OP + c];
            const float h2 = h * h, p2 = p * p;
            float den = h2 + p2;
            if (den < 1e-16f) den = 1e-16f;   // hpss_algorithm.c:236-239
            const float hv = h2 / den * m, pv = p2 / den * m;
            if (a.hMag) a.hMag[row * a.cols + b] = hv;
            if (a.pMag) a.pMag[row * a.cols + b] = pv;
            if (!a.hRe && !a.pRe) continue;
            const float mc = m < 1e-16f ? 1e-16f : m;  // :196-198
            const float ur = a.re[row * a.pitch + b] / mc, ui = a.im[row * a.pitch + b] / mc;
            const bool mirror = b > 0 && b < N / 2;    // :261-264
            if (a.hRe) {
                const float x = ur * hv, y = ui * hv;
                a.hRe[row * N + b] = x;
                a.hIm[row * N + b] = y;
                if (mirror) {
                    a.hRe[row * N + N - b] = x;
                    a.hIm[row * N + N - b] = -y;
                }
            }
            if (a.pRe) {
                const float x = ur * pv, y = ui * pv;
                a.pRe[row * N + b] = x;
                a.pIm[row * N + b] = y;
                if (mirror) {
                    a.pRe[row * N + N - b] = x;
                    a.pIm[row * N + N - b] = -y;
                }
            }
        }
    }
}

// the element of rank k/2 of the window of (row, col): v with #{< v} <= k/2 < #{<= v}
__global__ __launch_bounds__(256) void k_median_rank(const float *__restrict__ in, long long rows, int cols, int framesPerClip, int axis,
                                                      int k, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * cols) return;
    const long long row = e / cols;
    const int col = (int)(e - row * cols);
    const long long row0 = row / framesPerClip * framesPerClip;
    const long long left = rows - row0;
    const int T = left < framesPerClip ? (int)left : framesPerClip, t = (int)(row - row0);
    const int len = axis == 0 ? T : cols, at = axis == 0 ? t : col;
    const long long stride = axis == 0 ? cols : 1;
    const float *__restrict__ base = axis == 0 ? in + row0 * cols + col : in + row * cols;
    const int half = k >> 1;
    float res = 0.f;
    for (int i = -half; i <= half; ++i) {
        const int p = at + i;
        const float v = (p >= 0 && p < len) ? base[p * stride] : 0.f;
        int less = 0, lessEq = 0;
        for (int j = -half; j <= half; ++j) {
            const int q = at + j;
            const float u = (q >= 0 && q < len) ? base[q * stride] : 0.f;
            less += u < v;
            lessEq += u <= v;
        }
        if (less <= half && half < lessEq) res = v;
    }
    out[e] = res;
}

size_t tile_lds(int mode, int HP_TT, int hOrder, int pOrder) {
    const int hh = mode == HP_AXIS1 ? 0 : hOrder >> 1, ph = mode == HP_AXIS0 ? 0 : pOrder >> 1;
    const int pitch = (HP_FB + 2 * ph) | 1;
    return sizeof(float) * ((size_t)(HP_TT + 2 * hh) * pitch + (size_t)(mode == HP_HPSS ? 2 : 1) * HP_TT * HP_OP);
}

template <int MODE, int KH, int KP, int HP_TT>
int launch_tile(const AfxHpssArgs &a, void *stream) {
    const int binTiles = (a.cols + HP_FB - 1) / HP_FB, frameTiles = (a.framesPerClip + HP_TT - 1) / HP_TT;
    const long long clips = (a.rows + a.framesPerClip - 1) / a.framesPerClip;
    const long long blocks = clips * frameTiles * binTiles;
    if (blocks > 0x7fffffffLL) {
        afxdev_set_error("hpss: %lld tiles in one launch", blocks);
        return AFX_ERR_UNSUPPORTED;
    }
    const size_t lds = tile_lds(MODE, HP_TT, a.hOrder, a.pOrder);
    // the limit is raised once per instantiation and device: to what its largest orders need
    if (const int st = afx_dyn_lds<k_hpss_tile<MODE, KH, KP, HP_TT>>((int)tile_lds(MODE, HP_TT, KH, KP))) return st;
    hipLaunchKernelGGL((k_hpss_tile<MODE, KH, KP, HP_TT>), dim3((unsigned)blocks), dim3(HP_NT), lds, (hipStream_t)stream, a, binTiles,
                       frameTiles);
    AFX_LAUNCH_CHECK("k_hpss_tile");
    return AFX_OK;
}

}  // namespace

extern "C" int afxk_hpss_mask(const AfxHpssArgs *a, void *stream) {
    if (!a->re || !a->im || a->rows <= 0 || a->framesPerClip <= 0 || a->cols <= 0 || a->pitch < a->cols) return AFX_ERR_ARG;
    if (!(a->hOrder & 1) || !(a->pOrder & 1) || a->hOrder < 1 || a->pOrder < 1 || a->hOrder > AFX_MEDIAN_FAST_ORDER || a->pOrder > AFX_MEDIAN_FAST_ORDER) {
        afxdev_set_error("hpss: orders %d / %d are not odd numbers in 1 ... 63", a->hOrder, a->pOrder);
        return AFX_ERR_UNSUPPORTED;
    }
    if ((a->hRe || a->pRe) && a->cols != a->fftLength / 2 + 1) return AFX_ERR_ARG;
    if ((a->hRe && !a->hIm) || (a->pRe && !a->pIm)) return AFX_ERR_ARG;
    if (!a->hRe && !a->pRe && !a->hMag && !a->pMag) return AFX_OK;
    // the wrapper's defaults 21 / 31 on windows of their own size; everything else on 63 registers
    if (a->hOrder <= 21 && a->pOrder <= 31) return launch_tile<HP_HPSS, 21, 31, 64>(*a, stream);
    return launch_tile<HP_HPSS, 63, 63, 32>(*a, stream);
}

extern "C" int afxk_median_filter(const float *in, long long rows, int cols, int framesPerClip, int axis, int order, float *out,
                                  void *stream) {
    if (!in || !out || rows <= 0 || cols <= 0 || framesPerClip < 0 || (axis != 0 && axis != 1)) return AFX_ERR_ARG;
    if (order < 1 || !(order & 1) || order > AFX_MEDIAN_MAX_ORDER) {
        afxdev_set_error("median filter: order %d is not an odd number in 1 ... 255", order);
        return AFX_ERR_UNSUPPORTED;
    }
    if (rows > 0x7fffffffLL) {
        afxdev_set_error("median filter: %lld rows", rows);
        return AFX_ERR_UNSUPPORTED;
    }
    const int fpc = (framesPerClip == 0 || framesPerClip > rows) ? (int)rows : framesPerClip;
    if (order > AFX_MEDIAN_FAST_ORDER) {
        const long long blocks = (rows * cols + 255) / 256;
        if (blocks > 0x7fffffffLL) {
            afxdev_set_error("median filter: %lld elements in one launch", rows * cols);
            return AFX_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL(k_median_rank, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, rows, cols, fpc, axis, order,
                           out);
        AFX_LAUNCH_CHECK("k_median_rank");
        return AFX_OK;
    }
    AfxHpssArgs a = {};
    a.re = in;
    a.rows = rows;
    a.framesPerClip = fpc;
    a.cols = a.pitch = cols;
    a.hOrder = a.pOrder = order;
    a.hMag = out;
    if (axis == 0) {
        if (order <= 21) return launch_tile<HP_AXIS0, 21, 1, 64>(a, stream);
        if (order <= 31) return launch_tile<HP_AXIS0, 31, 1, 64>(a, stream);
        return launch_tile<HP_AXIS0, 63, 1, 64>(a, stream);
    }
    if (order <= 21) return launch_tile<HP_AXIS1, 1, 21, 64>(a, stream);
    if (order <= 31) return launch_tile<HP_AXIS1, 1, 31, 64>(a, stream);
    return launch_tile<HP_AXIS1, 1, 63, 64>(a, stream);
}
