// afx_onset.hip -- what onset detection (include/mir/onset_algorithm.h) adds to the descriptor kernels: the max filter along
// frequency, the per-clip normalisation with the peak picker, and the power -> dB map of util_powerToDB.
//
//   k_max_filter   out[r, j] = max of in[r, j - order / 2 ... j - 1 + order - order / 2] cut at the row's ends
//                  (flux_vector.c:3063-3081).  Rows of up to AFX_ONSET_FILTER_TILE bins: a workgroup stages a tile of whole
//                  rows -- one contiguous piece of memory -- in LDS and every thread takes the maximum of its window there;
//                  longer rows are read from global memory, the window's overlap from L2.  A maximum is exact.
//   k_onset_pick   one workgroup per clip.  normalise: min over the clip, max of (v - min), e = (v - min) / max when max > 0
//                  (onset_algorithm.c:379-385) -- one subtraction and one correctly rounded division per frame, the
//                  reference's float32 arithmetic bit for bit.  Then __peakPick (:423-460): per tile of 256 frames every
//                  thread decides its frame (maximum of its window by comparison; mean of its window as a float32 sum in
//                  index order divided by the count, plus delta), the candidates are compacted in frame order by a scan,
//                  and one lane applies the wait rule to the candidates alone.  The clip's envelope sits in LDS up to
//                  AFX_ONSET_LDS_FRAMES frames; a longer clip is picked from global memory.
//   k_db_max / k_db_map   util_powerToDB (flux_util.c:549-571): partial maxima per clip, then 10 log10f(p / max) clamped.
//
// Maxima and minima are taken as the reference takes them (__vmax / __vmin, flux_vector.c:1513-1557): the running value
// is replaced only by a strictly larger (smaller) one; among equal values (+0 and -0) any may come out.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"

namespace {

constexpr int NT = 256, NW = NT / 64;

__device__ __forceinline__ float ref_max(float m, float v) { return m < v ? v : m; }
__device__ __forceinline__ float ref_min(float m, float v) { return m > v ? v : m; }

// over the workgroup; red: [NW] floats of LDS, free again on return
template <bool MIN>
__device__ __forceinline__ float block_reduce(float v, float *red) {
#pragma unroll
    for (int msk = 32; msk > 0; msk >>= 1) {
        const float o = __shfl_xor(v, msk);
        v = MIN ? ref_min(v, o) : ref_max(v, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = MIN ? ref_min(r, red[w]) : ref_max(r, red[w]);
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(NT) k_max_filter(const float *in, long long rows, int cols, int left, int right, float *out,
                                                   int rowsPerTile) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *tile = reinterpret_cast<float *>(smem_raw);
    const int tid = threadIdx.x;
    if (rowsPerTile > 0) {
        const long long tiles = (rows + rowsPerTile - 1) / rowsPerTile;
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const long long r0 = t * rowsPerTile;
            const int nr = rows - r0 < rowsPerTile ? (int)(rows - r0) : rowsPerTile;
            const int cnt = nr * cols;
            const float *g = in + r0 * cols;
            for (int i = tid; i < cnt; i += NT) tile[i] = g[i];
            __syncthreads();
            for (int i = tid; i < cnt; i += NT) {
                const int r = i / cols, j = i - r * cols;
                const int s = j - left > 0 ? j - left : 0;
                const int e = j - 1 + right < cols - 1 ? j - 1 + right : cols - 1;
                const float *row = tile + r * cols;
                float m = row[s];
                for (int k = s + 1; k <= e; ++k) m = ref_max(m, row[k]);
                out[r0 * cols + i] = m;
            }
            __syncthreads();
        }
    } else {
        const long long total = rows * cols, stride = (long long)gridDim.x * NT;
        for (long long i = (long long)blockIdx.x * NT + tid; i < total; i += stride) {
            const long long r = i / cols;
            const int j = (int)(i - r * cols);
            const int s = j - left > 0 ? j - left : 0;
            const int e = j - 1 + right < cols - 1 ? j - 1 + right : cols - 1;
            const float *row = in + r * cols;
            float m = row[s];
            for (int k = s + 1; k <= e; ++k) m = ref_max(m, row[k]);
            out[i] = m;
        }
    }
}

// LDS: [0, 64) the reduction's exchange, [64, 128) candidates per wave, [128, 1152) the tile's candidates in frame order,
// then the envelope (LDS form only)
constexpr int PICK_LDS_FIXED = 128 + 4 * NT;

template <bool LDS>
__global__ void __launch_bounds__(NT) k_onset_pick(AfxOnsetPickArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *red = reinterpret_cast<float *>(smem_raw);
    int *wtot = reinterpret_cast<int *>(smem_raw + 64);
    int *cand = reinterpret_cast<int *>(smem_raw + 128);
    float *le = reinterpret_cast<float *>(smem_raw + PICK_LDS_FIXED);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.length;
    const long long b = blockIdx.x;
    const float *src = a.src + b * a.srcStride;
    const float *e = src;  // what the picker reads
    if (a.normalise) {
        float *evn = a.evn + b * a.evnStride;
        float mn = src[0];
        for (int i = tid; i < n; i += NT) mn = ref_min(mn, src[i]);
        mn = block_reduce<true>(mn, red);
        float mx = src[0] - mn;
        for (int i = tid; i < n; i += NT) mx = ref_max(mx, src[i] - mn);
        mx = block_reduce<false>(mx, red);
        for (int i = tid; i < n; i += NT) {
            float v = src[i] - mn;
            if (mx > 0.f) v = v / mx;
            evn[i] = v;
            if (LDS) le[i] = v;
        }
        e = evn;
    } else if (LDS) {
        for (int i = tid; i < n; i += NT) le[i] = src[i];
    }
    if (LDS) e = le;
    __syncthreads();  // the envelope, in LDS or as this workgroup's own stores to global memory
    if (!a.point && !a.count) return;

    const int preMax = a.preMax, postMax = a.postMax, preAvg = a.preAvg, postAvg = a.postAvg, wait = a.wait;
    const float delta = a.delta;
    int *point = a.point ? a.point + b * a.pointStride : nullptr;
    int pre = -wait - 1, cnt = 0;  // thread 0's
    for (int base = 0; base < n; base += NT) {
        const int i = base + tid;
        int is = 0;
        if (i < n) {
            const float v = e[i];
            const int s1 = i - preMax >= 0 ? i - preMax : 0;
            const int e1 = i + postMax < n ? i - 1 + postMax : n - 1;
            float m = e[s1];
            for (int k = s1 + 1; k <= e1; ++k) m = ref_max(m, e[k]);
            if (v == m) {
                const int s2 = i - preAvg >= 0 ? i - preAvg : 0;
                const int e2 = i + postAvg < n ? i - 1 + postAvg : n - 1;
                float s = 0.f;
                for (int k = s2; k <= e2; ++k) s += e[k];
                const float mean = s / (float)(e2 - s2 + 1);
                is = v >= mean + delta;
            }
        }
        // the tile's candidates in frame order: inclusive scan in the wave, waves one after the other
        int x = is;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        if (is) cand[off + x - 1] = i;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
            for (int w = 0; w < NW; ++w) total += wtot[w];
            for (int c = 0; c < total; ++c) {
                const int ci = cand[c];
                if (ci - pre > wait) {
                    if (point && cnt < a.pointStride) point[cnt] = ci;
                    pre = ci;
                    ++cnt;
                }
            }
        }
        __syncthreads();  // wtot and cand are free for the next tile
    }
    if (tid == 0 && a.count) a.count[b] = cnt;
}

// partial[b * parts + p] = max over part p of clip b (a part without elements repeats the clip's first value)
__global__ void __launch_bounds__(NT) k_db_max(const float *in, long long length, long long stride, int parts, float *partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *red = reinterpret_cast<float *>(smem_raw);
    const long long b = blockIdx.y;
    const int p = blockIdx.x;
    const float *x = in + b * stride;
    const long long per = (length + parts - 1) / parts, lo = p * per;
    const long long hi = lo + per < length ? lo + per : length;
    float m = x[0];
    for (long long i = lo + threadIdx.x; i < hi; i += NT) m = ref_max(m, x[i]);
    m = block_reduce<false>(m, red);
    if (threadIdx.x == 0) partial[b * parts + p] = m;
}

__global__ void __launch_bounds__(NT) k_db_map(const float *in, long long length, long long stride, int parts, const float *partial,
                                               float mn, float *out) {
    const long long b = blockIdx.y;
    float mx = partial[b * parts];
    for (int p = 1; p < parts; ++p) mx = ref_max(mx, partial[b * parts + p]);
    const float *x = in + b * stride;
    float *y = out + b * stride;
    const long long step = (long long)gridDim.x * NT;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < length; i += step) {
        const float v = 10.f * log10f(x[i] / mx);
        y[i] = v > mn ? v : mn;
    }
}

}  // namespace

extern "C" int afxk_max_filter(const float *in, long long rows, int cols, int order, float *out, void *stream) {
    if (!in || !out || in == out || rows < 0 || cols < 1 || order < 1) return AFX_ERR_ARG;
    if (rows == 0) return AFX_OK;
    // the window is cut at the row's ends: a side longer than the row changes nothing
    int left = order / 2, right = order - left;
    if (left > cols) left = cols;
    if (right > cols) right = cols;
    const int cap = afx_cu_count() * 8;
    if (cols <= AFX_ONSET_FILTER_TILE) {
        const int rpt = AFX_ONSET_FILTER_TILE / cols;
        const long long tiles = (rows + rpt - 1) / rpt;
        const unsigned grid = (unsigned)(tiles < cap ? tiles : cap);
        hipLaunchKernelGGL(k_max_filter, dim3(grid), dim3(NT), sizeof(float) * AFX_ONSET_FILTER_TILE, (hipStream_t)stream, in, rows,
                           cols, left, right, out, rpt);
    } else {
        const long long blocks = (rows * cols + NT - 1) / NT;
        const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
        hipLaunchKernelGGL(k_max_filter, dim3(grid), dim3(NT), 0, (hipStream_t)stream, in, rows, cols, left, right, out, 0);
    }
    AFX_LAUNCH_CHECK("k_max_filter");
    return AFX_OK;
}

extern "C" int afxk_onset_pick(const AfxOnsetPickArgs *a, void *stream) {
    if (!a || !a->src || a->batch <= 0 || a->length <= 0 || (a->normalise && !a->evn)) return AFX_ERR_ARG;
    if (a->batch > 1 && (a->srcStride < a->length || (a->normalise && a->evnStride < a->length))) return AFX_ERR_ARG;
    if (a->preMax < 0 || a->preAvg < 0 || a->wait < 0 || a->postMax < 1 || a->postAvg < 1) return AFX_ERR_ARG;
    if (a->point && (a->pointStride < 0 || (a->batch > 1 && a->pointStride < 1))) return AFX_ERR_ARG;
    if (!a->normalise && !a->point && !a->count) return AFX_OK;
    AfxOnsetPickArgs k = *a;
    // windows are cut at the clip's ends and no two frames are further apart than the clip is long
    const int n = a->length;
    if (k.preMax > n) k.preMax = n;
    if (k.postMax > n) k.postMax = n;
    if (k.preAvg > n) k.preAvg = n;
    if (k.postAvg > n) k.postAvg = n;
    if (k.wait > n) k.wait = n;
    if (n <= AFX_ONSET_LDS_FRAMES) {
        hipLaunchKernelGGL(k_onset_pick<true>, dim3((unsigned)a->batch), dim3(NT), PICK_LDS_FIXED + sizeof(float) * (size_t)n,
                           (hipStream_t)stream, k);
    } else {
        hipLaunchKernelGGL(k_onset_pick<false>, dim3((unsigned)a->batch), dim3(NT), PICK_LDS_FIXED, (hipStream_t)stream, k);
    }
    AFX_LAUNCH_CHECK("k_onset_pick");
    return AFX_OK;
}

extern "C" int afxk_power_to_db(const float *in, int batch, long long length, long long stride, float mn, float *out, void *stream) {
    if (!in || !out || batch <= 0 || batch > 65535 || length <= 0 || (batch > 1 && stride < length)) return AFX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    // enough workgroups for the maxima to fill the device whatever the batch, no part shorter than a workgroup's stride
    long long parts = (2048 + batch - 1) / batch;
    if (parts > 32) parts = 32;
    if (parts > (length + 4 * NT - 1) / (4 * NT)) parts = (length + 4 * NT - 1) / (4 * NT);
    float *partial = nullptr;
    AFX_HIP(hipMallocAsync(reinterpret_cast<void **>(&partial), sizeof(float) * (size_t)batch * (size_t)parts, s));
    hipLaunchKernelGGL(k_db_max, dim3((unsigned)parts, (unsigned)batch), dim3(NT), 64, s, in, length, stride, (int)parts, partial);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        long long blocks = (length + 4 * NT - 1) / (4 * NT);
        if (blocks > 64) blocks = 64;
        hipLaunchKernelGGL(k_db_map, dim3((unsigned)blocks, (unsigned)batch), dim3(NT), 0, s, in, length, stride, (int)parts, partial, mn,
                           out);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(partial, s);
    if (e != hipSuccess) {
        afxdev_set_error("launch of k_db_max / k_db_map failed: %s", hipGetErrorString(e));
        return AFX_ERR_HIP;
    }
    return AFX_OK;
}
