// afx_descriptors.hip -- the spectral-descriptor family on rows that already live in HBM: the device side of
// spectralObj_* / spectrogramObj_<descriptor> / spectralObj_computeDevice (reference: src/flux_spectral.c:21-833,
// src/feature/spectral_algorithm.c:236-1160).  The per-bin map of the spectrogram object is afx_spectral.hip; this file
// is the per-ROW reductions.
//
//   k_desc_rows<G, V, MODE>  row-local kinds (flatness, rolloff, centroid, spread, skewness, kurtosis, entropy, crest,
//       slope, decrease, bandwidth, rms, energy, hfc, eef, eer, max, mean, var), ANY subset in one launch.  A group of
//       G lanes owns a row and keeps it in registers, V values per lane (compile-time, fully unrolled: no indexed
//       register arrays); 64 / G rows per wave.  The row is fetched from HBM once -- 16 bytes per lane when pitch, start
//       and base allow it (MODE 0), dwords otherwise (MODE 1), dwords through the index table for index-list edges
//       (MODE 2) -- and the next row of the group is already in flight while this one is reduced.  Round 1 over the
//       registers: sum, sum f x, sum log, max + position, the energy / rms / hfc / decrease sums; round 2 over the same
//       registers, now that sum and centroid are known: the centred moments, the entropy, slope and variance terms and
//       the rolloff prefix.  The reference takes 2 - 4 passes over memory for these.  Reductions are four DPP steps
//       inside a row of 16 lanes and one ds_bpermute per doubling beyond; every lane of the group ends with the same
//       bits, whatever else was requested, so a list of requests equals the single requests bitwise.  A wave walks
//       blocks of 64 consecutive rows; lane g of a group keeps the sums of step g, so the per-row epilogue runs once
//       per block with a row per lane and every output slot is one store of 256 contiguous bytes.
//   k_desc_rows_long         the same two rounds for edges of more than 1024 bins (up to the 8193 columns of the STFT
//       sizes): one wave per row, the row is READ TWICE, the second time from L2 (a row is <= 32 KB and the same wave
//       asks for it microseconds later).  HBM traffic stays one fetch; the cost is a second trip through L2 / the
//       vector memory pipe, i.e. about half the rate of the register path.
//   k_desc_frames<G>         frame-difference kinds (flux, sd, sf, mkl, broadband, novelty, pd, wpd, nwpd, cd, rcd), any
//       subset in one launch: consecutive groups of a wave own consecutive frames, a request is one pass over frame i
//       and frame i - step (phase kinds: i, i - 1, i - 2), which the same or the neighbouring wave fetched a moment
//       earlier -- those re-reads are L2 / vector-L1 hits.  Frames whose predecessor lies before the start of their clip
//       (framesPerClip) are 0 and never read across the boundary.
//   k_desc_preprocess        spectrogramObj_preprocess (spectrogram_algorithm.c:2080-2120)
//
// Purely memory-bound: rows x len x 4 bytes in, 4 bytes per row and slot out.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "afx_device.h"
#include "afx_hipcheck.h"

namespace {

constexpr int DESC_NONE = 0x7fffffff;

// which sums a launch needs (uniform branches: a sum nobody asked for costs nothing)
enum : unsigned {
    N_F1 = 1u << 0, N_LOG = 1u << 1, N_MAX = 1u << 2, N_DEC = 1u << 3, N_RMS = 1u << 4, N_EN = 1u << 5, N_SQ = 1u << 6,
    N_HFC = 1u << 7, N_MOM = 1u << 8, N_BW = 1u << 9, N_ENT = 1u << 10, N_SLOPE = 1u << 11, N_VAR = 1u << 12,
    N_ROLL = 1u << 13
};

struct DescRowParams {
    const float *spec;
    float *out;
    const int *idx;
    const float *fre;
    long long rows, outStride;
    int num, start, len, idx0;
    float meanFre, slopeDen, varFre;
    int isPower;
    unsigned need;
    int slot[AFX_DESC_COUNT];  // first output slot of a kind, -1: not requested
    float rolloffThr, bwP, energyGamma, eerGamma;
    int entropyNorm, energyLog, eefNorm, eerNorm;
};

constexpr int DESC_MAX_FRAME_REQ = 11;
struct DescFrameParams {
    const float *spec, *phase;
    float *out;
    const int *idx;
    long long rows, outStride;
    int framesPerClip, num, start, len, idx0;
    int count;
    AfxDescReq req[DESC_MAX_FRAME_REQ];
};

// ---- cross-lane pieces: all lanes enabled, a lane reads a lane of its own row of 16 (row_mask / bank_mask 0xf)
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) {
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}

// sum over the G lanes of a group (G = 16, 32, 64, groups aligned to G): quad butterfly, half-row mirror, row mirror,
// then ds_bpermute across rows.  a + b == b + a, so every lane ends with the same bits.
template <int G>
__device__ __forceinline__ float gsum(float v) {
    v += dppf<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dppf<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dppf<0x141>(v);  // row_half_mirror
    v += dppf<0x140>(v);  // row_mirror
    if (G >= 32) v += __shfl_xor(v, 16);
    if (G >= 64) v += __shfl_xor(v, 32);
    return v;
}
template <int G>
__device__ __forceinline__ int gmin(int v) {
    v = min(v, dppi<0xB1>(v));
    v = min(v, dppi<0x4E>(v));
    v = min(v, dppi<0x141>(v));
    v = min(v, dppi<0x140>(v));
    if (G >= 32) v = min(v, __shfl_xor(v, 16));
    if (G >= 64) v = min(v, __shfl_xor(v, 32));
    return v;
}
// the larger value; of equal values the earlier position (spectralObj_max keeps the FIRST maximum, spectral_algorithm.c:946-958)
__device__ __forceinline__ void max_merge(float &v, int &p, float ov, int op) {
    const bool take = ov > v || (ov == v && op < p);
    v = take ? ov : v;
    p = take ? op : p;
}
// maximum of the group and the FIRST position that holds it: the value by fmaxf, then the smallest position among the
// lanes whose own maximum equals it -- two operations per cross-lane step instead of a compare-and-select of the pair
template <int G>
__device__ __forceinline__ void gmax(float &v, int &p) {
    float m = v;
    m = fmaxf(m, dppf<0xB1>(m));
    m = fmaxf(m, dppf<0x4E>(m));
    m = fmaxf(m, dppf<0x141>(m));
    m = fmaxf(m, dppf<0x140>(m));
    if (G >= 32) m = fmaxf(m, __shfl_xor(m, 16));
    if (G >= 64) m = fmaxf(m, __shfl_xor(m, 32));
    p = gmin<G>(v == m ? p : DESC_NONE);
    v = m;
}
// inclusive prefix sum over the lanes of a group, in lane order
template <int G>
__device__ __forceinline__ float gscan(float v, int g) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
        const float t = __shfl_up(v, d);
        v += g >= d ? t : 0.f;
    }
    return v;
}

// powf for the bandwidth exponent without the library routine's register appetite: exact products for p = 1, 2, 3, else
// 2^(p log2 |d|) on the transcendental unit (relative error ~ |p log2 d| 2^-23) with powf's sign rules -- a negative base
// is real for an integer p only (flux_spectral.c:414-421 hands f - centroid, which is negative below the centroid)
__device__ __forceinline__ float pow_p(float d, float p) {
    if (p == 1.f) return d;
    if (p == 2.f) return d * d;
    if (p == 3.f) return d * d * d;
    const float r = __builtin_amdgcn_exp2f(p * __log2f(fabsf(d)));
    if (d >= 0.f) return r;
    const float t = truncf(p);
    if (t != p) return NAN;
    return ((int)t & 1) ? -r : r;
}

// natural logarithm on the transcendental unit (v_log_f32, 1 ulp of log2): |error| <= ~1e-7 |log2 x|, which the mean of
// logs of the flatness carries into a relative error below 5e-6 even at the 2e-16 floor.  The library logf costs ~25
// instructions per bin and made the 19-descriptor launch compute-bound (0.87 ms against 0.18 ms for the centroid alone).
__device__ __forceinline__ float fast_ln(float x) { return __log2f(x) * 0.6931471805599453f; }

// ---- the two rounds of sums
struct Round1 {
    float S = 0.f, F1 = 0.f, L = 0.f, MX = -INFINITY, DEC = 0.f, RMS = 0.f, EN = 0.f, SQ = 0.f, HFC = 0.f;
    int MP = DESC_NONE;

    // x: the value, f: its frequency, j: its bin, p: its position in the edge, x0: the value at the edge's first bin
    __device__ __forceinline__ void add(const DescRowParams &P, float x, float f, int j, float rj, int p, bool valid, float x0) {
        const unsigned need = P.need;
        const float jf = (float)j;
        S += valid ? x : 0.f;
        if (need & N_F1) F1 += valid ? f * x : 0.f;                       // flux_spectral.c:153
        if (need & N_LOG) L += valid ? fast_ln(x + 2.0e-16f) : 0.f;       // :42
        if (need & N_MAX) {
            if (valid) max_merge(MX, MP, x, p);
        }
        if (need & N_DEC) DEC += valid && p >= 1 ? (x - x0) * rj : 0.f;   // :386: the ABSOLUTE bin divides (rj = 1 / bin)
        if (need & N_RMS) {                                                // :443-450
            const float w = (j == 0 || ((P.num & 1) == 0 && j == P.num - 1)) ? 0.5f : 1.f;
            RMS += valid ? x * x * w : 0.f;
        }
        if (need & N_EN) {                                                 // :812-826
            float v = P.isPower ? x : x * x;
            if (P.energyLog) v = logf(1.f + P.energyGamma * v);
            EN += valid ? v : 0.f;
        }
        if (need & N_SQ) SQ += valid ? x * x : 0.f;
        if (need & N_HFC) HFC += valid ? x * jf : 0.f;                     // :476
    }
    // the sums of another step become this lane's (take: this lane's row was reduced in that step)
    __device__ __forceinline__ void keep(const Round1 &o, bool take) {
        S = take ? o.S : S; F1 = take ? o.F1 : F1; L = take ? o.L : L; MX = take ? o.MX : MX; MP = take ? o.MP : MP;
        DEC = take ? o.DEC : DEC; RMS = take ? o.RMS : RMS; EN = take ? o.EN : EN; SQ = take ? o.SQ : SQ; HFC = take ? o.HFC : HFC;
    }
    template <int G>
    __device__ __forceinline__ void reduce(unsigned need) {
        S = gsum<G>(S);
        if (need & N_F1) F1 = gsum<G>(F1);
        if (need & N_LOG) L = gsum<G>(L);
        if (need & N_MAX) gmax<G>(MX, MP);
        if (need & N_DEC) DEC = gsum<G>(DEC);
        if (need & N_RMS) RMS = gsum<G>(RMS);
        if (need & N_EN) EN = gsum<G>(EN);
        if (need & N_SQ) SQ = gsum<G>(SQ);
        if (need & N_HFC) HFC = gsum<G>(HFC);
    }
};

struct Round2 {
    float M2 = 0.f, M3 = 0.f, M4 = 0.f, BW = 0.f, ENT = 0.f, SL = 0.f, VAR = 0.f;

    __device__ __forceinline__ void add(const DescRowParams &P, float x, float f, bool valid, float invS, float c, float meanV) {
        const unsigned need = P.need;
        const float d = f - c;
        if (need & N_MOM) {                                               // :183, :214, :245
            const float d2 = d * d;
            M2 += valid ? d2 * x : 0.f;
            M3 += valid ? d2 * d * x : 0.f;
            M4 += valid ? d2 * d2 * x : 0.f;
        }
        if (need & N_BW) {                                                // :414-421
            const float w = pow_p(d, P.bwP);
            BW += valid ? x * w : 0.f;
        }
        if (need & N_ENT) {                                               // :276-277
            const float v = x * invS;  // (a silent frame: 0 * inf = NaN, the reference's 0 / 0)
            ENT += valid ? v * __log2f(v + 1e-16f) : 0.f;
        }
        if (need & N_SLOPE) SL += valid ? (f - P.meanFre) * (x - meanV) : 0.f;  // :352-354
        if (need & N_VAR) {                                               // spectral_algorithm.c:1013-1014
            const float e = meanV - x;
            VAR += valid ? e * e : 0.f;
        }
    }
    __device__ __forceinline__ void keep(const Round2 &o, bool take) {
        M2 = take ? o.M2 : M2; M3 = take ? o.M3 : M3; M4 = take ? o.M4 : M4; BW = take ? o.BW : BW;
        ENT = take ? o.ENT : ENT; SL = take ? o.SL : SL; VAR = take ? o.VAR : VAR;
    }
    template <int G>
    __device__ __forceinline__ void reduce(unsigned need) {
        if (need & N_MOM) {
            M2 = gsum<G>(M2);
            M3 = gsum<G>(M3);
            M4 = gsum<G>(M4);
        }
        if (need & N_BW) BW = gsum<G>(BW);
        if (need & N_ENT) ENT = gsum<G>(ENT);
        if (need & N_SLOPE) SL = gsum<G>(SL);
        if (need & N_VAR) VAR = gsum<G>(VAR);
    }
};

__device__ __forceinline__ float guarded(float n, float m) { return m ? n / m : 0.f; }  // "if (m1) n1 / m1 else 0"

// the values of a row from its sums (one lane of the group stores)
__device__ __forceinline__ void desc_store(const DescRowParams &P, long long row, const Round1 &a, const Round2 &b, float c,
                                           float x0, int rollPos) {
    const float len = (float)P.len;
    float *o = P.out + row;
    const long long st = P.outStride;
    const int *s = P.slot;
    const float c2 = a.S ? sqrtf(b.M2 / a.S) : 0.f;  // spread (:186-191)
    if (s[AFX_DESC_FLATNESS] >= 0) o[s[AFX_DESC_FLATNESS] * st] = guarded(expf(a.L / len), a.S / len);  // :46-55
    if (s[AFX_DESC_ROLLOFF] >= 0) {  // :113-137: fre at the FIRST position whose running |x| reaches threshold * sum
        const int pos = rollPos == DESC_NONE ? P.len - 1 : rollPos;
        o[s[AFX_DESC_ROLLOFF] * st] = P.fre[P.idx ? P.idx[pos] : P.start + pos];
    }
    if (s[AFX_DESC_CENTROID] >= 0) o[s[AFX_DESC_CENTROID] * st] = c;
    if (s[AFX_DESC_SPREAD] >= 0) o[s[AFX_DESC_SPREAD] * st] = c2;
    if (s[AFX_DESC_SKEWNESS] >= 0) o[s[AFX_DESC_SKEWNESS] * st] = guarded(b.M3, c2 * c2 * c2 * a.S);       // :206-224
    if (s[AFX_DESC_KURTOSIS] >= 0) o[s[AFX_DESC_KURTOSIS] * st] = guarded(b.M4, c2 * c2 * c2 * c2 * a.S);  // :237-255
    const float l2 = log2f(len);
    if (s[AFX_DESC_ENTROPY] >= 0) o[s[AFX_DESC_ENTROPY] * st] = P.entropyNorm ? guarded(-b.ENT, l2) : -b.ENT;  // :280-292
    if (s[AFX_DESC_CREST] >= 0) o[s[AFX_DESC_CREST] * st] = guarded(a.MX, a.S / len);                     // :305-321
    if (s[AFX_DESC_SLOPE] >= 0) o[s[AFX_DESC_SLOPE] * st] = guarded(b.SL, P.slopeDen);                     // :357-362
    if (s[AFX_DESC_DECREASE] >= 0) o[s[AFX_DESC_DECREASE] * st] = guarded(a.DEC, a.S - x0);                // :380-395
    if (s[AFX_DESC_BANDWIDTH] >= 0) o[s[AFX_DESC_BANDWIDTH] * st] = P.bwP != 1.f ? pow_p(b.BW, 1.f / P.bwP) : b.BW;  // :426-429
    if (s[AFX_DESC_RMS] >= 0) o[s[AFX_DESC_RMS] * st] = sqrtf(2.f * a.RMS / (float)(P.num * P.num));       // :455: num, not the edge
    if (s[AFX_DESC_ENERGY] >= 0) o[s[AFX_DESC_ENERGY] * st] = a.EN / len;                                 // :829
    if (s[AFX_DESC_HFC] >= 0) o[s[AFX_DESC_HFC] * st] = a.HFC;
    // eef / eer (spectral_algorithm.c:858-906): a silent frame has entropy 0 / 0 = NaN, and so have these
    const float e = a.SQ / len;
    if (s[AFX_DESC_EEF] >= 0) {
        const float ent = P.eefNorm ? guarded(-b.ENT, l2) : -b.ENT;
        o[s[AFX_DESC_EEF] * st] = sqrtf(1.f + fabsf(e * ent));
    }
    if (s[AFX_DESC_EER] >= 0) {
        const float ent = P.eerNorm ? guarded(-b.ENT, l2) : -b.ENT;
        o[s[AFX_DESC_EER] * st] = sqrtf(1.f + fabsf(logf(1.f + e * P.eerGamma) / ent));
    }
    if (s[AFX_DESC_MAX] >= 0) {
        o[s[AFX_DESC_MAX] * st] = a.MX;
        const int pos = a.MP == DESC_NONE ? 0 : a.MP;
        o[(s[AFX_DESC_MAX] + 1) * st] = P.fre[P.idx ? P.idx[pos] : P.start + pos];
    }
    if (s[AFX_DESC_MEAN] >= 0) {
        o[s[AFX_DESC_MEAN] * st] = a.S / len;
        o[(s[AFX_DESC_MEAN] + 1) * st] = P.meanFre;
    }
    if (s[AFX_DESC_VAR] >= 0 && P.len >= 2) {  // spectral_algorithm.c:986-988: nothing is written for an edge of one bin
        o[s[AFX_DESC_VAR] * st] = b.VAR / (float)(P.len - 1);
        o[(s[AFX_DESC_VAR] + 1) * st] = P.varFre;
    }
}

// position of slot v of lane g: MODE 0 four neighbours per lane and chunk of G lanes, else one per lane and chunk
template <int G, int MODE>
__device__ __forceinline__ int slot_pos(int g, int v) {
    return MODE == 0 ? 4 * (g + G * (v >> 2)) + (v & 3) : g + G * v;
}

template <int G, int V, int MODE>
__device__ __forceinline__ void load_row(float (&x)[V], const float *row, const DescRowParams &P, int g, const int (&jj)[V]) {
    if (MODE == 0) {
        // a 16-byte block that holds one bin of the edge lies inside the row: start and the pitch are multiples of 4
        const float4 *r4 = reinterpret_cast<const float4 *>(row + P.start);
#pragma unroll
        for (int c = 0; c < V / 4; ++c) {
            const int q = g + G * c;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * q < P.len) t = r4[q];
            x[4 * c] = t.x;
            x[4 * c + 1] = t.y;
            x[4 * c + 2] = t.z;
            x[4 * c + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = slot_pos<G, MODE>(g, v) < P.len ? row[jj[v]] : 0.f;
    }
}

// rolloff over one chunk of the edge: `own` values of the lane at consecutive positions from p0
template <int G, int OWN>
__device__ __forceinline__ void rolloff_chunk(const float (&ax)[OWN], int p0, int len, int g, int lane, float thr, float &carry,
                                              int &found) {
    float pre[OWN];
    float run = 0.f;
#pragma unroll
    for (int e = 0; e < OWN; ++e) {
        run += ax[e];
        pre[e] = run;
    }
    const float inc = gscan<G>(run, g);
    float before = __shfl_up(inc, 1);
    before = g >= 1 ? before : 0.f;
    const float base = carry + before;
#pragma unroll
    for (int e = 0; e < OWN; ++e)
        if (p0 + e < len && base + pre[e] >= thr && found == DESC_NONE) found = p0 + e;
    carry += __shfl(inc, lane | (G - 1));
}

template <int G, int V, int MODE>
__device__ __forceinline__ void desc_rows_body(const DescRowParams &P) {
    constexpr int RPW = 64 / G;  // rows per wave
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned need = P.need;

    // the lane's bins and their frequencies: loaded once
    int jj[V];
    float ff[V], rj[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int p = slot_pos<G, MODE>(g, v);
        const bool valid = p < P.len;
        jj[v] = valid ? (MODE == 2 ? P.idx[p] : P.start + p) : P.idx0;
        ff[v] = P.fre[jj[v]];
        rj[v] = 1.f / (float)jj[v];
    }

    // A wave walks blocks of 64 consecutive rows, 64 / G rows per step: group `sub` has row 64 blk + RPW i + sub in step i.
    // Lane g of a group KEEPS the sums of step i == g, so after G steps the 64 lanes of the wave hold the sums of the
    // block's 64 rows, one row each: the per-row epilogue (divisions, roots, exp) then runs once per block with every lane
    // doing a row of its own, and each output slot is one store of 256 contiguous bytes -- not a store of 8 bytes by one
    // lane per group and step, which cost 0.011 ms per slot at the headline size.
    const long long blocks = (P.rows + 63) / 64;
    float x[V];
    long long blk = wave;
    if (blk < blocks) {
        const long long r = blk * 64 + sub < P.rows ? blk * 64 + sub : P.rows - 1;
        load_row<G, V, MODE>(x, P.spec + r * P.num, P, g, jj);
    }
    for (; blk < blocks; blk += waves) {
        Round1 ka;
        Round2 kb;
        float kx0 = 0.f;
        int kfound = DESC_NONE;
        for (int i = 0; i < G; ++i) {
            if (blk * 64 + (long long)i * RPW >= P.rows) break;  // (the last block of the call; uniform over the wave)
            // (every lane runs every step: a group beyond the last row repeats it, and nobody keeps its sums)
            const long long at = blk * 64 + (long long)i * RPW + sub;
            const long long row = at < P.rows ? at : P.rows - 1;
            const float *rp = P.spec + row * P.num;
            float xn[V];
            const bool wrap = i + 1 == G || blk * 64 + (long long)(i + 1) * RPW >= P.rows;
            const long long nfirst = wrap ? (blk + waves) * 64 : blk * 64 + (long long)(i + 1) * RPW;
            const bool more = wrap ? blk + waves < blocks : true;
            if (more) {
                const long long r = nfirst + sub < P.rows ? nfirst + sub : P.rows - 1;
                load_row<G, V, MODE>(xn, P.spec + r * P.num, P, g, jj);
            }
            const float x0 = (need & N_DEC) ? rp[P.idx0] : 0.f;

            Round1 a;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int p = slot_pos<G, MODE>(g, v);
                a.add(P, x[v], ff[v], jj[v], rj[v], p, p < P.len, x0);
            }
            a.reduce<G>(need);
            const float c = guarded(a.F1, a.S);  // centroid (:157-162)
            const float meanV = a.S / (float)P.len, invS = 1.f / a.S;

            Round2 b;
#pragma unroll
            for (int v = 0; v < V; ++v) b.add(P, x[v], ff[v], slot_pos<G, MODE>(g, v) < P.len, invS, c, meanV);
            b.reduce<G>(need);

            int found = DESC_NONE;
            if (need & N_ROLL) {
                const float thr = a.S * P.rolloffThr;
                float carry = 0.f;
                if (MODE == 0) {
#pragma unroll
                    for (int ch = 0; ch < V / 4; ++ch) {
                        const float ax[4] = {fabsf(x[4 * ch]), fabsf(x[4 * ch + 1]), fabsf(x[4 * ch + 2]), fabsf(x[4 * ch + 3])};
                        rolloff_chunk<G, 4>(ax, slot_pos<G, MODE>(g, 4 * ch), P.len, g, lane, thr, carry, found);
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const float ax[1] = {fabsf(x[v])};
                        rolloff_chunk<G, 1>(ax, slot_pos<G, MODE>(g, v), P.len, g, lane, thr, carry, found);
                    }
                }
                found = gmin<G>(found);
            }
            const bool mine = g == i;
            ka.keep(a, mine);
            kb.keep(b, mine);
            kx0 = mine ? x0 : kx0;
            kfound = mine ? found : kfound;
            if (more) {
#pragma unroll
                for (int v = 0; v < V; ++v) x[v] = xn[v];
            }
        }
        const long long myRow = blk * 64 + (long long)g * RPW + sub;
        if (myRow < P.rows) desc_store(P, myRow, ka, kb, guarded(ka.F1, ka.S), kx0, kfound);
    }
}

// up to 4 values per lane.  (4 waves per SIMD: forcing 64 registers for 8 waves spills 50 - 130 bytes per lane, and a
// spill is worse than the lost waves here -- the next row's load is in flight during the reductions anyway)
template <int G, int V, int MODE>
__global__ void __launch_bounds__(256) k_desc_rows(DescRowParams P) {
    desc_rows_body<G, V, MODE>(P);
}
// 16 values per lane (edges of 257 ... 1024 bins)
template <int G, int V, int MODE>
__global__ void __launch_bounds__(256) k_desc_rows_wide(DescRowParams P) {
    desc_rows_body<G, V, MODE>(P);
}

// edges of more than 1024 bins: one wave per row, two reads of the row (HBM, then L2)
__global__ void __launch_bounds__(256) k_desc_rows_long(DescRowParams P) {
    constexpr int G = 64;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned need = P.need;
    const int chunks = (P.len + G - 1) / G;
    for (long long row = wave; row < P.rows; row += waves) {
        const float *rp = P.spec + row * P.num;
        const float x0 = (need & N_DEC) ? rp[P.idx0] : 0.f;
        Round1 a;
        for (int k = 0; k < chunks; ++k) {
            const int p = lane + G * k;
            const bool valid = p < P.len;
            const int j = valid ? (P.idx ? P.idx[p] : P.start + p) : P.idx0;
            a.add(P, rp[j], P.fre[j], j, 1.f / (float)j, p, valid, x0);
        }
        a.reduce<G>(need);
        const float c = guarded(a.F1, a.S);
        const float meanV = a.S / (float)P.len, invS = 1.f / a.S;
        Round2 b;
        int found = DESC_NONE;
        const float thr = a.S * P.rolloffThr;
        float carry = 0.f;
        for (int k = 0; k < chunks; ++k) {
            const int p = lane + G * k;
            const bool valid = p < P.len;
            const int j = valid ? (P.idx ? P.idx[p] : P.start + p) : P.idx0;
            const float x = rp[j];
            b.add(P, x, P.fre[j], valid, invS, c, meanV);
            if (need & N_ROLL) {
                const float ax[1] = {valid ? fabsf(x) : 0.f};
                rolloff_chunk<G, 1>(ax, p, P.len, lane, lane, thr, carry, found);
            }
        }
        b.reduce<G>(need);
        if (need & N_ROLL) found = gmin<G>(found);
        if (lane == 0) desc_store(P, row, a, b, c, x0, found);
    }
}

// ---- frame-difference kinds
// sum over the edge of term(bin), every lane of the group gets it
template <int G, class F>
__device__ __forceinline__ float frame_sum(const DescFrameParams &P, int g, F term) {
    float acc = 0.f;
    for (int p = g; p - g < P.len; p += G) {
        const bool valid = p < P.len;
        const int j = valid ? (P.idx ? P.idx[p] : P.start + p) : P.idx0;
        const float v = term(j);
        acc += valid ? v : 0.f;
    }
    return gsum<G>(acc);
}

template <int G>
__global__ void __launch_bounds__(256) k_desc_frames(DescFrameParams P) {
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const float len = (float)P.len;
    for (long long base = wave * RPW; base < P.rows; base += waves * RPW) {
        const bool live = base + sub < P.rows;
        const long long row = live ? base + sub : P.rows - 1;
        // frame number inside its clip: frames before `step` have no predecessor in the clip and are 0
        const long long t = P.framesPerClip > 0 ? row % P.framesPerClip : row;
        const float *cur = P.spec + row * P.num;
        for (int q = 0; q < P.count; ++q) {
            const AfxDescReq &R = P.req[q];
            const int kind = R.kind;
            float value = 0.f;
            int zeros = 1;  // leading frames of a clip that are 0
            if (kind == AFX_DESC_FLUX || kind == AFX_DESC_SD || kind == AFX_DESC_SF || kind == AFX_DESC_NOVELTY) {
                const int step = R.iarg[0] < 1 ? 1 : R.iarg[0];
                zeros = step;
                // (a frame without predecessor reads itself: the result is dropped below, nothing before the clip is touched)
                const float *pre = t >= step ? cur - (long long)step * P.num : cur;
                if (kind == AFX_DESC_FLUX) {  // flux_spectral.c:62-103; iarg: step, isPostive, isExp, type; farg: p
                    const int positive = R.iarg[1], isExp = R.iarg[2], type = R.iarg[3];
                    const float p = R.farg[0];
                    value = frame_sum<G>(P, g, [&](int j) {
                        float v = cur[j] - pre[j];
                        v = positive ? (v > 0.f ? v : 0.f) : fabsf(v);
                        return p == 2.f ? v * v : powf(v, p);
                    });
                    if (type) value /= len;
                    if (isExp) value = powf(value, 1.f / p);
                } else if (kind == AFX_DESC_SD || kind == AFX_DESC_SF) {  // :490-560; iarg: step, isPostive
                    const int positive = R.iarg[1];
                    const bool square = kind == AFX_DESC_SF;
                    value = frame_sum<G>(P, g, [&](int j) {
                        float v = cur[j] - pre[j];
                        v = positive ? (v > 0.f ? v : 0.f) : fabsf(v);
                        return square ? v * v : v;
                    });
                } else {  // novelty, :747-810; iarg: step, methodType, dataType; farg: threshold
                    const int method = R.iarg[1], number = R.iarg[2];
                    const float thr = R.farg[0];
                    value = frame_sum<G>(P, g, [&](int j) {
                        const float c = cur[j], b = pre[j];
                        float v;
                        if (method == 0) v = c - b;
                        else {
                            const float ratio = c / (b + 1e-16f);
                            const float lg = logf(ratio);
                            v = method == 1 ? lg : method == 2 ? c * lg : ratio - lg - 1.f;
                        }
                        return v > thr ? (number ? 1.f : v) : 0.f;
                    });
                }
            } else if (kind == AFX_DESC_MKL || kind == AFX_DESC_BROADBAND) {
                const float *pre = t >= 1 ? cur - P.num : cur;
                if (kind == AFX_DESC_MKL) {  // :564-590; iarg: type
                    value = frame_sum<G>(P, g, [&](int j) { return logf(1.f + cur[j] / (pre[j] + 1e-16f)); });
                    if (R.iarg[0]) value /= len;
                } else {  // broadband, :720-738: a count; farg: threshold
                    const float thr = R.farg[0];
                    value = frame_sum<G>(P, g, [&](int j) { return 10.f * log10f(cur[j] / pre[j]) > thr ? 1.f : 0.f; });
                }
            } else if (kind == AFX_DESC_PD || kind == AFX_DESC_WPD || kind == AFX_DESC_NWPD) {  // :592-640
                zeros = 2;
                const float *ph0 = P.phase + row * P.num;
                const float *ph1 = t >= 2 ? ph0 - P.num : ph0;
                const float *ph2 = t >= 2 ? ph0 - 2LL * P.num : ph0;
                const bool weight = kind != AFX_DESC_PD;
                value = frame_sum<G>(P, g, [&](int j) {
                    const float v = fabsf(ph0[j] - 2.f * ph1[j] + ph2[j]);
                    return weight ? v * cur[j] : v;
                }) / len;
                if (kind == AFX_DESC_NWPD) {
                    const float m = frame_sum<G>(P, g, [&](int j) { return cur[j]; }) / len;
                    value = value / (m + 1e-16f);
                }
            } else {  // cd / rcd, :672-718: frame 1 has no predicted bin, later frames subtract it
                const float *ph0 = P.phase + row * P.num;
                const bool two = t >= 2;
                const float *pre = t >= 1 ? cur - P.num : cur;
                const float *ph1 = two ? ph0 - P.num : ph0;
                const float *ph2 = two ? ph0 - 2LL * P.num : ph0;
                const bool rectify = kind == AFX_DESC_RCD;
                value = frame_sum<G>(P, g, [&](int j) {
                    const float s = cur[j], sp = pre[j];
                    const float a0 = ph0[j];
                    float re = s * cosf(a0), im = s * sinf(a0);
                    if (two) {
                        const float a1 = 2.f * ph1[j] - ph2[j];
                        re -= sp * cosf(a1);
                        im -= sp * sinf(a1);
                    }
                    const float v = sqrtf(re * re + im * im);
                    return rectify && s <= sp ? 0.f : v;
                });
            }
            if (live && g == 0) P.out[(long long)R.slot * P.outStride + row] = t >= zeros ? value : 0.f;
        }
    }
}

__global__ void __launch_bounds__(256) k_desc_preprocess(const float *in, float *out, long long total, int num, float value, int halfBin) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int j = (int)(i % num);
        float v = in[i] / value;
        if (j == 0 || j == halfBin) v *= 0.5f;
        out[i] = v;
    }
}

bool is_frame_kind(int k) { return k == AFX_DESC_FLUX || (k >= AFX_DESC_SD && k <= AFX_DESC_NOVELTY); }
bool is_phase_kind(int k) { return k >= AFX_DESC_PD && k <= AFX_DESC_RCD; }

int launch_rows_wide(const DescRowParams &P, int mode, unsigned blocks, hipStream_t s) {
    if (mode == 0) hipLaunchKernelGGL((k_desc_rows_wide<64, 16, 0>), dim3(blocks), dim3(256), 0, s, P);
    else if (mode == 1) hipLaunchKernelGGL((k_desc_rows_wide<64, 16, 1>), dim3(blocks), dim3(256), 0, s, P);
    else hipLaunchKernelGGL((k_desc_rows_wide<64, 16, 2>), dim3(blocks), dim3(256), 0, s, P);
    AFX_LAUNCH_CHECK("k_desc_rows_wide");
    return AFX_OK;
}

template <int G, int V>
int launch_rows(const DescRowParams &P, int mode, unsigned blocks, hipStream_t s) {
    if (mode == 0) hipLaunchKernelGGL((k_desc_rows<G, V, 0>), dim3(blocks), dim3(256), 0, s, P);
    else if (mode == 1) hipLaunchKernelGGL((k_desc_rows<G, V, 1>), dim3(blocks), dim3(256), 0, s, P);
    else hipLaunchKernelGGL((k_desc_rows<G, V, 2>), dim3(blocks), dim3(256), 0, s, P);
    AFX_LAUNCH_CHECK("k_desc_rows");
    return AFX_OK;
}

// persistent waves: enough workgroups of 4 waves for `units` wave-sized pieces of work, at most the `resident` workgroups a
// CU holds at the kernel's register count (more would only queue behind the first ones with a share of the work fixed
// in advance): k_desc_rows 4, k_desc_rows_wide 2, k_desc_rows_long / k_desc_frames / k_desc_preprocess 6
unsigned desc_blocks(long long units, int resident) {
    const long long want = (units + 3) / 4, cap = (long long)afx_cu_count() * resident;
    return (unsigned)(want < cap ? (want < 1 ? 1 : want) : cap);
}

}  // namespace

extern "C" int afxk_descriptors(const AfxDescArgs *a, void *stream) {
    if (!a || !a->spec || !a->out || !a->fre || !a->req || a->count <= 0 || a->rows < 0 || a->num < 1 || a->len < 1 ||
        a->start < 0 || (!a->idx && a->start + a->len > a->num) || a->idx0 < 0 || a->idx0 >= a->num) {
        afxdev_set_error("afxk_descriptors: bad argument");
        return AFX_ERR_ARG;
    }
    if (a->rows == 0) return AFX_OK;
    DescRowParams R = {};
    DescFrameParams F = {};
    for (int k = 0; k < AFX_DESC_COUNT; ++k) R.slot[k] = -1;
    bool seen[AFX_DESC_COUNT] = {};
    int rowKinds = 0;
    for (int i = 0; i < a->count; ++i) {
        const AfxDescReq &q = a->req[i];
        if (q.kind < 0 || q.kind >= AFX_DESC_COUNT || seen[q.kind] || q.slot < 0) {
            afxdev_set_error("afxk_descriptors: request %d: kind %d is out of range or asked for twice", i, q.kind);
            return AFX_ERR_ARG;
        }
        seen[q.kind] = true;
        if (is_phase_kind(q.kind) && !a->phase) {
            afxdev_set_error("afxk_descriptors: kind %d needs the phase rows", q.kind);
            return AFX_ERR_ARG;
        }
        if (is_frame_kind(q.kind)) {
            F.req[F.count++] = q;
            continue;
        }
        ++rowKinds;
        R.slot[q.kind] = q.slot;
        switch (q.kind) {
            case AFX_DESC_FLATNESS: R.need |= N_LOG; break;
            case AFX_DESC_ROLLOFF: R.need |= N_ROLL; R.rolloffThr = q.farg[0]; break;
            case AFX_DESC_CENTROID: R.need |= N_F1; break;
            case AFX_DESC_SPREAD: case AFX_DESC_SKEWNESS: case AFX_DESC_KURTOSIS: R.need |= N_F1 | N_MOM; break;
            case AFX_DESC_ENTROPY: R.need |= N_ENT; R.entropyNorm = q.iarg[0]; break;
            case AFX_DESC_CREST: R.need |= N_MAX; break;
            case AFX_DESC_SLOPE: R.need |= N_SLOPE; break;
            case AFX_DESC_DECREASE: R.need |= N_DEC; break;
            case AFX_DESC_BANDWIDTH: R.need |= N_F1 | N_BW; R.bwP = q.farg[0]; break;
            case AFX_DESC_RMS: R.need |= N_RMS; break;
            case AFX_DESC_ENERGY:
                R.need |= N_EN;
                R.energyLog = q.iarg[0];
                R.energyGamma = q.farg[0] <= 0.f ? 10.f : q.farg[0];  // flux_spectral.c:820-822
                break;
            case AFX_DESC_HFC: R.need |= N_HFC; break;
            case AFX_DESC_EEF: R.need |= N_ENT | N_SQ; R.eefNorm = q.iarg[0]; break;
            case AFX_DESC_EER: R.need |= N_ENT | N_SQ; R.eerNorm = q.iarg[0]; R.eerGamma = q.farg[0]; break;
            case AFX_DESC_MAX: R.need |= N_MAX; break;
            case AFX_DESC_VAR: R.need |= N_VAR; break;
            default: break;  // mean: the sum alone
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (rowKinds) {
        R.spec = a->spec; R.out = a->out; R.idx = a->idx; R.fre = a->fre;
        R.rows = a->rows; R.outStride = a->outStride;
        R.num = a->num; R.start = a->start; R.len = a->len; R.idx0 = a->idx0;
        R.meanFre = a->meanFre; R.slopeDen = a->slopeDen; R.varFre = a->varFre;
        R.isPower = a->isPower;
        const int len = a->len;
        if (len > 1024) {
            hipLaunchKernelGGL(k_desc_rows_long, dim3(desc_blocks(a->rows, 6)), dim3(256), 0, s, R);
            AFX_LAUNCH_CHECK("k_desc_rows_long");
        } else {
            const bool vec = !a->idx && a->num % 4 == 0 && a->start % 4 == 0 && (reinterpret_cast<uintptr_t>(a->spec) & 15) == 0;
            const int mode = a->idx ? 2 : vec ? 0 : 1;
            int st;
            const long long blocks64 = (a->rows + 63) / 64;  // a wave's unit of work: 64 consecutive rows
            if (len <= 64) st = launch_rows<16, 4>(R, mode, desc_blocks(blocks64, 4), s);
            else if (len <= 128) st = launch_rows<32, 4>(R, mode, desc_blocks(blocks64, 4), s);
            else if (len <= 256) st = launch_rows<64, 4>(R, mode, desc_blocks(blocks64, 4), s);
            else st = launch_rows_wide(R, mode, desc_blocks(blocks64, 2), s);
            if (st != AFX_OK) return st;
        }
    }
    if (F.count) {
        F.spec = a->spec; F.phase = a->phase; F.out = a->out; F.idx = a->idx;
        F.rows = a->rows; F.outStride = a->outStride;
        F.framesPerClip = a->framesPerClip; F.num = a->num; F.start = a->start; F.len = a->len; F.idx0 = a->idx0;
        if (a->len <= 16) hipLaunchKernelGGL(k_desc_frames<16>, dim3(desc_blocks((a->rows + 3) / 4, 6)), dim3(256), 0, s, F);
        else if (a->len <= 32) hipLaunchKernelGGL(k_desc_frames<32>, dim3(desc_blocks((a->rows + 1) / 2, 6)), dim3(256), 0, s, F);
        else hipLaunchKernelGGL(k_desc_frames<64>, dim3(desc_blocks(a->rows, 6)), dim3(256), 0, s, F);
        AFX_LAUNCH_CHECK("k_desc_frames");
    }
    return AFX_OK;
}

extern "C" int afxk_desc_preprocess(const float *in, float *out, long long rows, int num, float value, int halfBin, void *stream) {
    if (!in || !out || rows < 0 || num < 1) return AFX_ERR_ARG;
    const long long total = rows * num;
    if (total == 0) return AFX_OK;
    hipLaunchKernelGGL(k_desc_preprocess, dim3(desc_blocks((total + 255) / 256, 6)), dim3(256), 0, (hipStream_t)stream, in, out, total,
                       num, value, halfBin);
    AFX_LAUNCH_CHECK("k_desc_preprocess");
    return AFX_OK;
}
