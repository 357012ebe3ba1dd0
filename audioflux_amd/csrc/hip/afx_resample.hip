// afx_resample.hip -- band-limited resampling (include/dsp/resample_algorithm.h): every output of every clip in one launch.
//
// Output i of a clip is a sum over the samples around n = floor(i / ratio), weighted by a windowed-sinc table that is
// read every `step` entries from a phase-dependent first entry and interpolated linearly between neighbouring entries
// (resample_algorithm.c:468-515).  The integers (n, the first entries, the tap counts) and the interpolation weights are
// the reference's: afx_resample_phase (afx_device.h) states them once for the kernel, the host and the tests.
//
// Shape: persistent workgroups of AFX_RESAMPLE_TILE threads.  A workgroup copies the table into LDS once (Best / Mid /
// Fast: 128 / 64 / 32 KB; the difference table is one subtraction of neighbours, so there is no second table), then takes
// work items (tile of AFX_RESAMPLE_TILE outputs) x (group of G clips).  A lane owns one output index: the weights of an
// index are the same for every clip, so each is computed once and multiplies G samples -- 2 table reads and G sample reads
// for G multiply-adds.  The input span under the tile is staged in LDS, one row per clip.  A table that does not fit LDS
// is read from global memory (TAB_LDS = false); a span that does not fit is read from global memory (a run-time,
// workgroup-uniform choice).  The taps of one output are summed in float32 in the reference's order, left side first.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"

namespace {

constexpr int NT = AFX_RESAMPLE_TILE;

// the clips' samples as the taps see them: rows of the staged span, or the clips in global memory
template <int G>
struct XLds {
    const float *xs;  // row g at xs + g * pitch, sample `lo` first
    int pitch, lo;
    __device__ __forceinline__ float at(int g, int idx) const { return xs[g * pitch + (idx - lo)]; }
};
template <int G>
struct XGlobal {
    const float *x[G];  // a clip beyond the batch repeats the group's last one: read, never stored
    __device__ __forceinline__ float at(int g, int idx) const { return x[g][idx]; }
};

// `count` taps from j0 on: table entry off + j step, sample first + dir j
template <int G, class X>
__device__ __forceinline__ void taps_side(const float *tab, int off, float delta, int step, int j0, int count, int first, int dir,
                                          const X &x, float (&acc)[G]) {
    for (int j = j0; j < count; ++j) {
        const int o = off + j * step;
        const float t0 = tab[o];
        const float w = fmaf(delta, tab[o + 1] - t0, t0);
        const int idx = first + dir * j;
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = fmaf(w, x.at(g, idx), acc[g]);
    }
}

template <int G, class X>
__device__ __forceinline__ void one_output(const float *tab, const AfxResamplePhase &p, int step, int L, int S, const X &x,
                                           float (&acc)[G]) {
    // left: x[n - j], j < min(n + 1, (L - offL) / step); samples at or beyond S count as 0
    const int cl = (L - p.offL) / step;
    const int jl = p.n - (S - 1) > 0 ? p.n - (S - 1) : 0;
    taps_side<G>(tab, p.offL, p.deltaL, step, jl, p.n + 1 < cl ? p.n + 1 : cl, p.n, -1, x, acc);
    // right: x[n + 1 + j], j < min(S - n - 1, (L - offR) / step)
    const int cr = (L - p.offR) / step;
    const long long room = (long long)S - p.n - 1;
    taps_side<G>(tab, p.offR, p.deltaR, step, 0, room < cr ? (int)room : cr, p.n + 1, 1, x, acc);
}

template <bool TAB_LDS, int G>
__global__ void __launch_bounds__(NT) k_resample(AfxResampleArgs a, int tabFloats, int spanFloats, int taps, long long tiles,
                                                 long long items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *tabS = reinterpret_cast<float *>(smem_raw);   // [interpLength + 1] when TAB_LDS
    float *xs = tabS + (TAB_LDS ? tabFloats : 0);         // [G][spanFloats]
    const int tid = threadIdx.x;
    const int L = a.interpLength, S = a.sourceLength;
    if (TAB_LDS)
        for (int k = tid; k <= L; k += NT) tabS[k] = a.table[k];  // (the first barrier of the loop below orders it)
    const float scale = afx_resample_scale(a.ratio);
    const int step = afx_resample_step(a.ratio, a.bitLength);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long tile = item % tiles, b0 = (item / tiles) * G;
        const int gc = a.batch - b0 < G ? (int)(a.batch - b0) : G;
        const long long i0 = tile * NT;
        const int cnt = a.targetLength - i0 < NT ? (int)(a.targetLength - i0) : NT;
        // the samples the tile's outputs can read: n is monotonic in i
        const long long nLo = afx_resample_phase(i0, a.ratio, scale, a.bitLength).n;
        const long long nHi = afx_resample_phase(i0 + cnt - 1, a.ratio, scale, a.bitLength).n;
        const long long lo = nLo - (taps - 1) > 0 ? nLo - (taps - 1) : 0;
        const long long hi = nHi + taps < S - 1 ? nHi + taps : S - 1;
        const long long len = hi >= lo ? hi - lo + 1 : 0;
        const bool staged = len <= spanFloats;  // workgroup-uniform
        __syncthreads();  // the previous item's readers are done with xs
        if (staged)
            for (int g = 0; g < G; ++g) {
                const float *src = a.x + (b0 + (g < gc ? g : 0)) * a.clipStride + lo;
                for (int k = tid; k < (int)len; k += NT) xs[g * spanFloats + k] = g < gc ? src[k] : 0.f;
            }
        __syncthreads();
        if (tid < cnt) {
            const long long i = i0 + tid;
            const AfxResamplePhase p = afx_resample_phase(i, a.ratio, scale, a.bitLength);
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.f;
            const float *tab;
            if constexpr (TAB_LDS) tab = tabS; else tab = a.table;
            if (staged) {
                const XLds<G> x{xs, spanFloats, (int)lo};
                one_output<G>(tab, p, step, L, S, x, acc);
            } else {
                XGlobal<G> x;
#pragma unroll
                for (int g = 0; g < G; ++g) x.x[g] = a.x + (b0 + (g < gc ? g : gc - 1)) * a.clipStride;
                one_output<G>(tab, p, step, L, S, x, acc);
            }
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < gc) a.out[(b0 + g) * a.outStride + i] = acc[g] / a.outScale;
        }
    }
}

template <bool TAB_LDS, int G>
int launch(const AfxResampleArgs &a, const AfxResampleLaunch &l, void *stream) {
    const long long tiles = ((long long)a.targetLength + NT - 1) / NT;
    const long long items = tiles * ((a.batch + G - 1) / G);
    int perCu = (int)(AFX_RESAMPLE_LDS_BUDGET / l.ldsBytes);
    perCu = perCu < 1 ? 1 : (perCu > 2048 / NT ? 2048 / NT : perCu);
    const long long resident = (long long)afx_cu_count() * perCu;
    const unsigned grid = (unsigned)(items < resident ? items : resident);
    const int tabFloats = (int)((((4ll * (a.interpLength + 1)) + 15) & ~15ll) / 4);
    // one instantiation serves every table and span: its limit is raised to the whole budget, once
    if (const int st = afx_dyn_lds<k_resample<TAB_LDS, G>>(AFX_RESAMPLE_LDS_BUDGET)) return st;
    hipLaunchKernelGGL((k_resample<TAB_LDS, G>), dim3(grid), dim3(NT), (size_t)l.ldsBytes, (hipStream_t)stream, a, tabFloats,
                       l.spanFloats, l.taps, tiles, items);
    AFX_LAUNCH_CHECK("k_resample");
    return AFX_OK;
}

template <bool TAB_LDS>
int dispatch(const AfxResampleArgs &a, const AfxResampleLaunch &l, void *stream) {
    switch (l.group) {
        case 4: return launch<TAB_LDS, 4>(a, l, stream);
        case 2: return launch<TAB_LDS, 2>(a, l, stream);
        default: return launch<TAB_LDS, 1>(a, l, stream);
    }
}

}  // namespace

extern "C" int afxk_resample(const AfxResampleArgs *a, void *stream) {
    if (!a || !a->x || !a->out || !a->table) return AFX_ERR_ARG;
    if (a->batch <= 0 || a->sourceLength <= 0 || a->targetLength <= 0 || a->bitLength <= 0) return AFX_ERR_ARG;
    if (a->interpLength < 2 || a->interpLength > AFX_RESAMPLE_MAX_TABLE + 1 || !(a->outScale > 0.f)) return AFX_ERR_ARG;
    if (a->batch > 1 && (a->clipStride < a->sourceLength || a->outStride < a->targetLength)) return AFX_ERR_ARG;
    AfxResampleLaunch l;
    const int st = afx_resample_launch_plan(a->batch, a->ratio, a->bitLength, a->interpLength, &l);
    if (st != AFX_OK) return st;
    return l.tableInLds ? dispatch<true>(*a, l, stream) : dispatch<false>(*a, l, stream);
}
