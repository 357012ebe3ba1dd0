// afx_melfused2.hip -- the headline kernel, round-2 form: framed STFT -> |S|^2 (or |S|,
// |S|^2p) -> banded filter bank (-> log10 -> DCT-II cepstra), one 64-lane wave per 2048-sample
// frame, real results.  Same algorithm and summation orders as k_stft_mel_banded
// (afx_melfused.hip, which keeps the complex-result instantiations); what changed is how the
// wave talks to the LDS and what it no longer computes twice:
//
//   * every constant table is laid out for 16-byte reads: window and W_1024 twiddles as
//     [(n1 >> 1)][lane][n1 & 1] (one ds_read_b128 = two rows), the W_2048 split twiddles per lane
//     [s][lane][m]                                                      (46 -> 22 table reads)
//   * the W_64 twiddles are applied by the READER of exchange 2 (round 10): the second radix-16 stores its outputs as they
//     are, and the lane that takes a base q into the last radix-4 multiplies V[q][1..3] by row j1 = q >> 4 of a 16-row
//     table {W^j1, W^2j1 | W^3j1, pad} -- one ds_read_b128 + one ds_read_b64 per base, requested with the image rows; 12
//     complex products per lane and frame where the writer had 15, 4 + 4 table reads (24 LDS cycles) where it had 8 x 16
//     bytes (32) and a drain of its own.  The products are the same products: no power bin moves by a bit
//   * exchange 1: row pitch 72 float2, writer lane 4 m1 + m2 stores at column
//     8 (m1 >> 1) + 2 m2 + (m1 & 1): the reader takes (m1, m1 + 1) with one ds_read_b128;
//     exchange 2: image V[q][m2] (m2 fastest; 16-byte halves swapped when bit 3 of q is set:
//     conflict-free without padding), a lane's four radix-4 inputs are two ds_read_b128;
//     rows are written two at a time with ds_write2_b64            (64 -> 32 exchange ops)
//   * 513 conjugate pairs on 512 slots: lane 0's mirror side reads the self-mirrored base
//     q = 128 instead of q = 0, its slots 2 / 3 become the pairs (128, 896) / (384, 640) and
//     bin 512 is |Z[512]|^2 directly -- no lane runs the "centre" butterflies any more
//     (28 VALU + 6 LDS reads per frame that only lane 0's results were kept of)
//   * the power row goes out with ds_write2st64_b32 (bins k, k + 256 in one instruction), its
//     zero pad sits behind the exchange images and is written once per launch
//   * cepstra in the same launch (CC): every 16 frames the wave re-reads its own 16 mel rows
//     (L2-resident), takes log10 and runs 32 v_mfma_f32_16x16x4_f32 against the DCT rows held
//     in LDS -- the matrix pipe is otherwise idle in this kernel, the second launch and its
//     478 MB re-read of mel from HBM disappear (xxcc_algorithm.c:124-155).  CC = 1: the headline
//     form (num = 128, log10, whole-row plan); CC = 2: afx_ccblock.h's general form (any num <= 128
//     that is a multiple of 4, split plans, cube-root rectification; DCT operand from memory)
//   * temporal features (TEMPORAL): energy / rms / zero-crossing rate of the windowed frame
//     as wave reductions (temporal_algorithm.c:138-144), so isTemporal objects stay on this kernel
//
// Index algebra and LDS bank behaviour of every access class: tools/proto_fft1024_v2.py; the W_64 table and its stage-3
// reads: tools/proto_fft1024_v3.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "afx_melplan.h"
#include "afx_melparts.h"  // (also the knock-out switches AFX_KO of the measurement builds: RD128_S ... KO_ON)
#include "afx_ccblock.h"

// measurement switches of round 6 (profiles/r06_ab_headline.txt): AFX_V2_NTIN -- the samples are read with the streaming (nt) policy, so
// that the bank rows a wave re-reads for its cepstra 16 frames later are not pushed out of the L2 by them; AFX_V2_CCEVERY -- frames per
// cepstrum block (16: one full MFMA tile; 8: the rows are half as old when they are re-read)
#ifdef AFX_V2_NTIN
#define AFX_V2_LOAD(p) __builtin_nontemporal_load(p)
#define AFX_V2_NT true   // (the hand-issued fetch of the new rows, rows_fetch_new_s, takes the policy as a template argument)
#else
#define AFX_V2_LOAD(p) (*(p))
#define AFX_V2_NT false
#endif
#ifndef AFX_V2_CCEVERY
#define AFX_V2_CCEVERY 16
#endif
// measurement switches of round 7 (profiles/r07_ab_headline.txt): AFX_V2_STAMPS -- every wave records s_memtime at its first frame, at
// every 16th frame and after its last one, with its workgroup, wave index, frame count and hardware id, in a debug buffer of its own
// that the launcher writes to the file AFX_V2_STAMPS_FILE names (tools/v2_stamps.py reads it)
#ifdef AFX_V2_STAMPS
#include <cstdio>
#include <vector>
#endif

namespace {

constexpr int NFFT = 2048;
constexpr int MC = 1024;
constexpr int WAVES = 12;                    // one workgroup per CU, 3 waves per SIMD (8: - 5 %, profiles/r02_ab_headline.txt)
constexpr int WAVES_CPLX = 12;               // complex results (8 while the imaginary parts waited in registers for their pass)
__host__ __device__ constexpr int waves_of(bool cplx) { return cplx ? WAVES_CPLX : WAVES; }
constexpr int P1 = 72;                       // float2 per row of the exchange-1 image
constexpr int PROW_OFF = 5120;               // byte offset of the power row in a wave's region
constexpr int PROW_F = 1104;                 // 1025 bins + zero pad for the fixed-length band loops
constexpr int WAVE_LDS = PROW_OFF + PROW_F * 4;  // 9536: pad [9220, 9536) lies behind both images
constexpr int CLAIM_LDS = 16;                // behind the waves' regions: the workgroup's claim counter (one word)
static_assert(16 * P1 * 8 <= PROW_OFF + 1025 * 4, "exchange image must end before the zero pad");
// table blob, byte offsets (built on the host by fill_tables + afxk_melfused_create, copied to LDS per workgroup)
constexpr int T_WIN = 0;                     // [8][64] float4: (w[2n], w[2n+1]) of rows n1 = 2j, 2j + 1
constexpr int T_TW1 = 8192;                  // [8][64] float4: W_1024^(lane k1), k1 = 2j, 2j + 1
constexpr int T_TW2 = 16384;                 // [16] rows j1 of 4 float2, TW2_PITCH bytes apart: W_64^(j1), W_64^(2 j1) | W_64^(3 j1), pad
constexpr int TW2_PITCH = 32;                // (a row = 8 banks of 64; the lanes of one read group meet at most three rows, all within
                                             //  one run of 8 consecutive rows: conflict-free, tools/proto_fft1024_v3.py)
constexpr int T_TW3 = 16960;                 // [2][64][4] float2: 0.5 W_2048^bin of slot (s, lane, m)
static_assert(TW2_PITCH % 16 == 0 && T_TW2 + 16 * TW2_PITCH <= T_TW3, "W_64 table: 16-byte rows, ends before the split twiddles");
constexpr int T_BAND = 21056;                // [64][WP] floats: lane-major band weights, A then B taps (packed form: a | b | c)
// (pc: the third partition of the packed form, 0 otherwise; the pitch stays an odd number of 16-byte units: conflict-free b128)
__host__ __device__ constexpr int wpitch(int ta, int tb, int pc = 0) { return ta + tb + pc + 4; }
__host__ __device__ constexpr int tab_bytes(int ta, int tb, int pc = 0) { return T_BAND + 64 * wpitch(ta, tb, pc) * 4; }
constexpr int DCT_PITCH = 36;                // floats per lane of the DCT operand table (9 x 16 B: conflict-free b128)
__host__ __device__ constexpr int block_lds_bytes(int ta, int tb, bool cc, int pc = 0) {
    return tab_bytes(ta, tb, pc) + (cc ? 64 * DCT_PITCH * 4 : 0) + WAVES * WAVE_LDS + CLAIM_LDS;  // (complex results: fewer waves, less)
}

// Frames of a workgroup's range that one claim takes when `left` remain (guided: about left / (2 waves)): whole 16-frame cepstrum
// blocks while every wave can still have one, then multiples of 4 down to `minRun`, so that the waves of a workgroup end within a few
// frame times of each other
__host__ __device__ constexpr int claim_length(int left, int waves, int minRun) {
    const int g = left / (2 * waves);
    if (left >= 16 * waves) return g >= 16 ? g & ~15 : 16;
    return (g & ~3) > minRun ? g & ~3 : minRun;
}

struct KArgs2 {
    const float *x;
    long long clipStride;
    long long totalFrames;
    int timeLength, hop;
    long long framesPerWg; // workgroup b owns frames [b framesPerWg, (b + 1) framesPerWg) (< 2^30); its waves claim runs of them
    int aligned;           // frame starts are 8-byte aligned -> float2 loads
    const float4 *tab;     // table blob
    const int *meta;       // [6][64]: startA, startB, rowA, rowB, segIdx lo / hi; packed form [8][64]: base a / b / c, row a / b / c,
                           // b continues a, c continues b (AfxBandPack)
    int specMap, postPow;
    float normValue;
    float *out;            // [totalFrames, num]
    float *outIm;          // CPLX: imaginary parts, same shape
    int num;
    // CC
    const float *dct;      // device [num, num] orthonormal DCT-II (row = coefficient)
    int ccNum, ccCbrt;     // (ccCbrt: powf(x, 1/3) instead of log10, CC = 2 only)
    float *cc;             // [totalFrames, ccNum]
    // TEMPORAL
    float *energy, *rms, *zcr;  // [totalFrames]
    // STFT: the mapped spectrum rows themselves (afxk_stft2k): bins binLo .. binLo + binCount - 1 of every frame to out + f * outPitch
    const float *win;      // device window [2048], natural order, 8-byte aligned (the blob's window table is not used)
    int binLo, binCount;
    long long outPitch;
    int vecOut;            // binLo == 0, all 1025 bins, 16-byte aligned rows of >= 1028 floats: 16-byte stores (the pad gets zeros)
#ifdef AFX_V2_STAMPS
    unsigned long long *stamps;  // [workgroups * waves][STAMP_WORDS]
#endif
};
#ifdef AFX_V2_STAMPS
constexpr int STAMP_WORDS = 64, STAMP_HEAD = 8;  // t0, t1, workgroup | wave << 32, frames, HW_ID, XCC_ID, -, -, then a stamp per 16 frames
#endif

// (lds_addr, RD64 / RD128, WR2_64, WR2ST_32, PIN, LDS_WAIT_N and the L1-bypassing load: afx_asm.h; wave_lds_sync, split_pair,
// split_pair_c, cplx_map, lo2 / hi2: afx_melparts.h)

// Wave priority by phase of the frame (s_setprio): phases 0 window, 1 first radix-16 + twiddles + exchange writes, 2 exchange
// reads, 3 second radix-16, 4 last radix-4 + split, 5 band, 6 store / cepstra; bit p of AFX_PRIO_MASK raises phase p to
// AFX_PRIO_LEVEL.  The three waves of a SIMD are in different phases of their frames; with the transform's phases (1-4,
// dense packed arithmetic between short LDS exchanges) above the window / band / store phases (LDS- and memory-latency
// bound) a wave that can keep the vector unit busy wins the issue port: 1.53-1.56 -> 1.47-1.48 ms per step, measured
// interleaved against masks 0x0A, 0x1F, 0x3E, 0x20, 0x61 and levels 1 / 2 / 3 (profiles/r04_ab_headline.txt).  Round 10: phase 3
// lost its table reads and their drain to phase 4 and is plain arithmetic + exchange stores now; with it at the base priority
// (0x16) the step is 1.3 % shorter than with 0x1E, which the same mask on the round-9 kernel is not (profiles/r10_ab_headline.txt (e))
#ifndef AFX_PRIO_MASK
#define AFX_PRIO_MASK 0x16
#endif
#ifndef AFX_PRIO_LEVEL
#define AFX_PRIO_LEVEL 1
#endif
#define MEL_PHASE(p)                                                                                       \
    do {                                                                                                   \
        if (AFX_PRIO_MASK != 0) __builtin_amdgcn_s_setprio(((AFX_PRIO_MASK >> (p)) & 1) ? AFX_PRIO_LEVEL : 0); \
    } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// SHIFT: hop = 128 * SHIFT samples -> the next frame's register image is this one moved down by
//   SHIFT registers, only SHIFT new float2 per lane are fetched (0: every frame fetched whole)
// SPLIT: the plan's slots hold row SEGMENTS (afx_bandplan_build_split)
// CC: cepstra of the rows in the same launch, ccNum <= 16 (1: num = 128, log10 rectification, DCT operand in LDS; 2: afx_ccblock.h)
// TEMPORAL: energy / rms / zcr of the windowed frame
// CPLX: complex results (specMap 3: S, 4: S^2): a second row in LDS holds the imaginary parts for a second pass of the bank
// STFT: no bank -- the frame's mapped spectrum row (|S|^2, |S|, |S|^2p) goes to memory as it stands in the LDS (afxk_stft2k: the
//   producer of the dense-bank route's [T, F] rows and the STFT object's real results at n_fft 2048)
// PC: > 0 the packed band plan (afx_bandplan.c): every lane runs ONE stream of TA | TB | PC taps that holds one, two or three whole
//   rows -- 48 slots per lane where the (48, 16) variant runs 64; a row's multiply-adds and their order are those of the plain form
template <int TA, int TB, int SHIFT, bool SPLIT, int CC, bool TEMPORAL, bool CPLX = false, bool STFT = false, int PC = 0>
__global__ __launch_bounds__(waves_of(CPLX) * 64, 3) void k_stft_mel_v2(KArgs2 a) {
    constexpr int NWV = waves_of(CPLX);
    static_assert(!(CPLX && (CC || TEMPORAL)), "complex results: the bank only");
    static_assert(!STFT || (TA == 0 && TB == 0 && !SPLIT && CC == 0 && !TEMPORAL && !CPLX), "STFT instantiations: real rows, no bank");
    static_assert(PC == 0 || (!SPLIT && !STFT), "packed plans hold whole rows");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int WP = wpitch(TA, TB, PC);
    constexpr int TABB = tab_bytes(TA, TB, PC);
    constexpr int DCTB = CC == 1 ? 64 * DCT_PITCH * 4 : 0;
    unsigned char *wreg = smem + TABB + DCTB + wave * WAVE_LDS;
    float *prow = reinterpret_cast<float *>(wreg + PROW_OFF);

    // ---- workgroup-shared tables -> LDS (once) -------------------------------------------
    {
        float4 *s4 = reinterpret_cast<float4 *>(smem);
        for (int i = threadIdx.x + (STFT ? T_TW1 / 16 : 0); i < TABB / 16; i += NWV * 64) s4[i] = a.tab[i];
        if constexpr (STFT) {
            // the caller's window in the pair layout of fill_tables: entry (n1, lane) = (w[2n], w[2n+1]), n = 64 n1 + lane,
            // at float2 index 128 (n1 >> 1) + 2 lane + (n1 & 1)
            v2 *tw = reinterpret_cast<v2 *>(smem + T_WIN);
            const v2 *w2 = reinterpret_cast<const v2 *>(a.win);
            for (int at = threadIdx.x; at < 1024; at += NWV * 64) {
                const int n1 = 2 * (at >> 7) + (at & 1), l = (at & 127) >> 1;
                tw[at] = w2[64 * n1 + l];
            }
        }
        if constexpr (CC == 1) {
            // B operand of the cepstrum MFMAs: lane (coefficient fi = lane & 15, k-slot g = lane >> 4)
            // holds dct[fi][16 u + 4 g + c] at [lane][4 u + c]
            float *tabD = reinterpret_cast<float *>(smem + TABB);
            for (int i = threadIdx.x; i < 64 * 32; i += NWV * 64) {
                const int l = i >> 5, e = i & 31;
                const int fi = l & 15, g = l >> 4;
                tabD[l * DCT_PITCH + e] =
                    fi < a.ccNum ? a.dct[(long long)fi * a.num + 16 * (e >> 2) + 4 * g + (e & 3)] : 0.f;
            }
        }
        for (int i = 1025 + lane; i < PROW_F; i += 64) prow[i] = 0.f;  // zero pad, never overwritten
        if (threadIdx.x == 0) *reinterpret_cast<int *>(smem + TABB + DCTB + NWV * WAVE_LDS) = 0;  // frames of the range claimed so far
    }
    __syncthreads();

    // ---- per-lane constants (loop-invariant LDS byte addresses) -----------------------------
    const int k1 = lane >> 2, m2 = lane & 3;
    const unsigned T0 = lds_addr(smem), W0 = lds_addr(wreg);
    const unsigned aWin = T0 + T_WIN + 16 * lane;                      // + 1024 j; W_1024 at + T_TW1
    const unsigned aE1w = W0 + 8 * (8 * (k1 >> 1) + 2 * m2 + (k1 & 1));  // writer m1 = lane >> 2; row k: + 576 k
    const unsigned aE1r = W0 + 576 * k1 + 16 * m2;                     // pair jj: + 64 jj
    const unsigned aE2w = W0 + 32 * k1 + 16 * ((m2 >> 1) ^ ((k1 >> 3) & 1)) + 8 * (m2 & 1);  // j1: + 512 j1
    const int b3l = (lane >> 3) & 1;
    const unsigned aAlo = W0 + 32 * lane + 16 * b3l, aAhi = W0 + 32 * lane + 16 * (1 - b3l);  // s = 1: + 2048
    const int qm0 = lane == 0 ? 128 : 256 - lane, qm1 = 192 - lane;
    const unsigned aB0lo = W0 + 32 * qm0 + 16 * ((qm0 >> 3) & 1), aB0hi = W0 + 32 * qm0 + 16 * (1 - ((qm0 >> 3) & 1));
    const unsigned aB1lo = W0 + 32 * qm1 + 16 * ((qm1 >> 3) & 1), aB1hi = W0 + 32 * qm1 + 16 * (1 - ((qm1 >> 3) & 1));
    // W_64 rows of the four bases (row j1 = q >> 4): own bases lane, lane + 64 (s = 1: + 4 rows), mirror bases qm0, qm1
    const unsigned aTwA = T0 + T_TW2 + TW2_PITCH * (lane >> 4);
    const unsigned aTwB0 = T0 + T_TW2 + TW2_PITCH * (qm0 >> 4), aTwB1 = T0 + T_TW2 + TW2_PITCH * (qm1 >> 4);
    const unsigned aT3lo = T0 + T_TW3 + 32 * lane + 16 * b3l, aT3hi = T0 + T_TW3 + 32 * lane + 16 * (1 - b3l);
    const unsigned R = W0 + PROW_OFF;
    const unsigned aP01 = R + 4 * lane;                                // bins k, k + 256 | 64 + k ... by offsets
    const unsigned aP23 = R + 4 * (lane == 0 ? 128 : lane + 512);      // (k + 512, k + 768) | lane 0: (128, 384)
    const unsigned aQs1 = R + 4 * (192 - lane);                        // 1024 - bin of s = 1 slots; s = 0 slots 1, 0 at + 9, + 13
    const unsigned aQ23 = R + 4 * (lane == 0 ? 640 : 256 - lane);      // s = 0 slots 3, 2 | lane 0: (640, 896)
    const bool lane0 = (lane == 0);

    constexpr int MROW = PC ? 192 : 128;  // the rows' numbers stand behind the starts
    const int startA = STFT ? 0 : a.meta[lane], startB = STFT ? 0 : a.meta[64 + lane], startC = PC ? a.meta[128 + lane] : 0;
    const int rowA = STFT ? -1 : a.meta[MROW + lane], rowB = STFT ? -1 : a.meta[MROW + 64 + lane], rowC = PC ? a.meta[MROW + 128 + lane] : -1;
    const unsigned seg0 = SPLIT ? (unsigned)a.meta[256 + lane] : 0u, seg1 = SPLIT ? (unsigned)a.meta[320 + lane] : 0u;
    const bool contB = PC ? a.meta[384 + lane] != 0 : false, contC = PC ? a.meta[448 + lane] != 0 : false;
    const unsigned apa = R + 4 * startA, apb = R + 4 * startB, apc = R + 4 * startC;
    const unsigned awr = T0 + T_BAND + 4 * WP * lane;
    // global memory, per lane and loop-invariant: byte offsets from wave-uniform (scalar) bases -- the frame loop forms no 64-bit
    // address on the vector unit.  vRaw: the lane's float2 in a 512-byte row of samples; vRowA / vRowB: its two bank rows' slots
    // in an output row (okA / okB: the lane has such a row); rowPitch: floats from one output row to the next
    const unsigned vRaw = 8u * (unsigned)lane, vLane = 4u * (unsigned)lane;
    const bool okA = rowA >= 0, okB = rowB >= 0, okC = rowC >= 0;
    const unsigned vRowA = okA ? 4u * (unsigned)rowA : 0u, vRowB = okB ? 4u * (unsigned)rowB : 0u, vRowC = okC ? 4u * (unsigned)rowC : 0u;
    const long long rowPitch = STFT ? a.outPitch : (long long)a.num;

    // ---- frame runs: no wave owns a share of the workgroup's range [wgBeg, wgBeg + wgN) -- a wave that runs out of frames claims
    //      the next run from the counter in LDS (lane 0: fetch-add; the length from a read just before it, which may be stale:
    //      runs never overlap, they are only a little longer than the guide asks for), and leaves when the range is used up.
    //      A frame's values do not depend on the wave that computes it.  minRun: a range shorter than 4 frames per wave (small
    //      launches: one round of workgroups cannot be filled) is still spread over all waves
    const long long wgBeg = (long long)blockIdx.x * a.framesPerWg;
    const int wgN = (int)(a.totalFrames - wgBeg < a.framesPerWg ? a.totalFrames - wgBeg : a.framesPerWg);
    const int minRun = wgN >= 4 * NWV ? 4 : wgN > NWV ? (wgN + NWV - 1) / NWV : 1;
    int *claimed = reinterpret_cast<int *>(smem + TABB + DCTB + NWV * WAVE_LDS);
    // a run's clip and frame index (locate) come from its 32-bit offset in the range and the range's own clip and frame index: one
    // 64-bit divide per wave, before the frame loop
    const int wgClip = (int)(wgBeg / a.timeLength);
    const unsigned wgT = (unsigned)(wgBeg - (long long)wgClip * a.timeLength);
    auto locate = [&](long long fr, int &c, int &tt) {
        const unsigned at = wgT + (unsigned)(fr - wgBeg);  // < 2^31 + 2^30
        c = wgClip + (int)(at / (unsigned)a.timeLength);
        tt = (int)(at % (unsigned)a.timeLength);
    };
    auto claim = [&](long long &rb, long long &re) -> bool {
        int s = wgN, l = 0;
        if (lane0) {
            const int left = wgN - __atomic_load_n(claimed, __ATOMIC_RELAXED);
            if (left > 0) {
                l = claim_length(left, NWV, minRun);
                s = __atomic_fetch_add(claimed, l, __ATOMIC_RELAXED);
            }
        }
        s = __builtin_amdgcn_readfirstlane(s);
        l = __builtin_amdgcn_readfirstlane(l);
        if (s >= wgN) return false;
        rb = wgBeg + s;
        re = wgBeg + (s + l < wgN ? s + l : wgN);
        return true;
    };
    int ccN = 0;  // frames of this run whose cepstra are still to be formed
#ifdef AFX_V2_STAMPS
    unsigned long long *stamp = a.stamps + ((long long)blockIdx.x * NWV + wave) * STAMP_WORDS;
    int stampN = 0;  // frames done
    if (lane0) {
        stamp[0] = __builtin_amdgcn_s_memtime();
        stamp[2] = (unsigned long long)blockIdx.x | ((unsigned long long)wave << 32);
        stamp[4] = (unsigned)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));   // HW_REG_HW_ID, all 32 bits
        stamp[5] = (unsigned)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
    }
#endif

    // raw samples of the frame about to be transformed: raw[n1] = (x[2n], x[2n+1]), n = 64 n1 + lane
    v2 raw[16];
    auto fetch = [&](const float *px, int first) {
        if (a.aligned) {
            const v2 *p2 = reinterpret_cast<const v2 *>(px);
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1)
                if (n1 >= first) raw[n1] = AFX_V2_LOAD(&p2[64 * n1 + lane]);
        } else {
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1)
                if (n1 >= first) {
                    const int n = 64 * n1 + lane;
                    raw[n1] = v2{px[2 * n], px[2 * n + 1]};
                }
        }
    };

    // the next frame's new rows were requested by hand behind the first radix-16 (rows_fetch_new_s): they landed long ago,
    // and they are waited for where the wait cannot meet a store that was issued a moment ago -- before the frame's row stores
    // (k_stft_band_4k2 does the same).  The registers' first use is pinned behind the wait
    auto raw_landed = [&]() {
        if constexpr (SHIFT > 0) {
            VM_WAIT_ALL();
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) PIN(raw[n1]);
        }
    };

    // ---- cepstra of `cnt` (<= 16) consecutive rows fb.. of this wave: C[16 frames, 16 coefficients] =
    //      log10(max(rows, 1e-8)) . D^T with v_mfma_f32_16x16x4_f32.  Lane (fi = lane & 15, g = lane >> 4)
    //      loads float4 row[fb + fi][16 u + 4 g ..] (k-slot g of MFMA (u, c) stands for band 16 u + 4 g + c),
    //      the matching DCT elements come from the LDS table.  Called one frame AFTER the 16th row was
    //      stored, so the s_waitcnt finds those stores long complete; reads bypass the CU's L1.
    // fb: the first row's frame per lane (CC == 2); fbS: the same number, wave-uniform, from the run's scalar row offset / 128
    // (CC == 1, where num is 128; not used otherwise)
    auto cc_block = [&](long long fb, long long fbS, int cnt) {
        if constexpr (CC == 2) {  // the general form: runtime num / rectification, DCT operand from memory
            ccb_rows<SPLIT ? 2 : 4>(a.out, a.cc, a.dct, a.num, a.ccNum, a.ccCbrt, fb, cnt, lane);
        } else {
        VM_WAIT_ALL();  // own stores -> L2 (vmcnt counts stores on gfx9)
        int ln = lane;
        PIN(ln);  // keep this block's per-lane values out of the frame loop's registers
        const int fi = ln & 15, g = ln >> 4;
        // row fb + fi (tail: duplicate the last row, not stored), bands 4 g ..: one scalar base + this lane offset + immediates
        fbS = uniform64(fbS);  // (the run's last block is reached under a per-lane condition: say that the number is the wave's)
        const float *const srows = a.out + fbS * 128;
        const unsigned vsrc = 512u * (unsigned)(fi < cnt ? fi : cnt - 1) + 16u * (unsigned)g;
        const unsigned ad = T0 + TABB + 4 * DCT_PITCH * ln;
        v4f acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        constexpr float LOG10_2 = 0.30102999566398120f;
        // two halves of the 128 bands: 32 + 16 live registers instead of 64 + 16 (the frame loop
        // keeps the next frame's 32 prefetch registers alive across this block)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v4f av[4], dv[4];
            // (served by the L2, never by this CU's L1; bands 16 (4 h + u) + 4 g ..: 64 (4 h + u) bytes)
            GLD128X4_L2_S(av[0], av[1], av[2], av[3], vsrc, srows, 256 * h, 256 * h + 64, 256 * h + 128, 256 * h + 192);
#pragma unroll
            for (int u = 0; u < 4; ++u) RD128(dv[u], ad, 16 * (4 * h + u));
            VM_LGKM_WAIT_ALL();
#pragma unroll
            for (int u = 0; u < 4; ++u) PIN(av[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) PIN(dv[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const v4f fl = max4_floor(av[u]);  // one v_max_f32 per value; a NaN row value gives 1e-8 as with fmaxf (afx_frameops.h)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    // log10f(max(x, 1e-8)) (xxcc_algorithm.c:131-137) as v_log_f32 * log10(2); four
                    // independent accumulator chains (a dependent f32 MFMA waits 40 cycles)
                    const float lg = __log2f(fl[c]) * LOG10_2;
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(lg, dv[u][c], acc[c], 0, 0, 0);
                }
            }
        }
        const v4f sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        // C layout: column (coefficient) = lane & 15, row (frame) = 4 (lane >> 4) + reg
        if (fi < a.ccNum) {
            const unsigned vcc = 4u * (unsigned)(4 * g * a.ccNum + fi);
            float *const scc = a.cc + fbS * a.ccNum;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int rr = 4 * g + reg;
                if (rr < cnt) GST32_S(vcc, sum[reg], scc + reg * a.ccNum);
            }
        }
        }  // CC == 1
        ccN -= cnt;
    };

    // one run after the other; between two runs every LDS operation of the wave has returned and the claim's own are waited for at
    // once, so the hand-counted waits of the frame loop see the counts they always saw.  The frame loop itself is the loop of a
    // fixed share, and f is kept per lane in it (laneZero) as it was when it came from the wave's index: with f in scalar
    // registers, or with the next run's first frame fetched from inside this loop (one frame ahead, like every other frame), the
    // compiler kept two or three register images of the overlapping frames, moved one onto the other once per frame and spilled
    // 40-140 bytes per lane in every SHIFT > 0 instantiation.  So a run's first frame is fetched in the open, once per run
    long long fClaim, fEndClaim;
    while (claim(fClaim, fEndClaim)) {
    int laneZero = 0;
    PIN(laneZero);
    long long f = fClaim + laneZero;
    const long long fEnd = fEndClaim;
    int clip, t;
    locate(fClaim, clip, t);
    fetch(a.x + (long long)clip * a.clipStride + (long long)t * a.hop, 0);
    long long rowOff = fClaim * rowPitch;  // floats from the output's start to frame f's row: wave-uniform, advanced per frame
    for (; f < fEnd; ++f) {
        v2 v[16];
        MEL_PHASE(0);
        // ---- 1. window: 8 x 16 bytes per lane, the first half is used while the second lands ----
        {
            v4f wv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) RD128_S(2, wv[j], aWin, T_WIN + 1024 * j);
            LDS_WAIT_N(4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                PIN(wv[j]);
                v[2 * j] = raw[2 * j] * lo2(wv[j]);
                v[2 * j + 1] = raw[2 * j + 1] * hi2(wv[j]);
            }
            LDS_WAIT_N(0);
#pragma unroll
            for (int j = 4; j < 8; ++j) {
                PIN(wv[j]);
                v[2 * j] = raw[2 * j] * lo2(wv[j]);
                v[2 * j + 1] = raw[2 * j + 1] * hi2(wv[j]);
            }
        }
        // ---- 1c. temporal features of the windowed frame (temporal_algorithm.c:138-144) -------
        if constexpr (TEMPORAL) {
            // sample order: n = 64 n1 + lane, (x, y) = samples 2n, 2n + 1; the sample before 2n is the
            // y of the previous lane (n1 unchanged) or, for lane 0, the y of lane 63 at n1 - 1
            float e = 0.f, z = 0.f;
            float prevTop = 0.f;  // y of lane 63 at n1 - 1, wave-uniform
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                e = fmaf(v[n1].x, v[n1].x, e);
                e = fmaf(v[n1].y, v[n1].y, e);
                float py = __shfl_up(v[n1].y, 1, 64);
                if (lane0) py = prevTop;
                const bool first = (n1 == 0) && lane0;  // sample 0 has no predecessor
                if (!first && v[n1].x * py < 0.f) z += 1.f;
                if (v[n1].y * v[n1].x < 0.f) z += 1.f;
                prevTop = __shfl(v[n1].y, 63, 64);
            }
            e = wave_sum(e);
            z = wave_sum(z);
            if (lane0) {
                a.energy[f] = e;
                a.rms[f] = sqrtf(e / (float)NFFT);
                a.zcr[f] = (float)((double)z / (double)NFFT);
            }
        }

        // ---- 2a. radix-16 over n1, twiddle W_1024^(lane k1), transpose through LDS -----------
        MEL_PHASE(1);
        dft16(v);
        {
            v4f tq[8];  // requested after the butterflies: held across them they would spill
#pragma unroll
            for (int j = 0; j < 8; ++j) RD128_S(2, tq[j], aWin, T_TW1 + 1024 * j);
            LDS_WAIT_N(0);
#pragma unroll
            for (int j = 0; j < 8; ++j) PIN(tq[j]);
            v2 o[16];
            o[0] = v[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) o[k] = cmul(v[rev4(k)], (k & 1) ? hi2(tq[k >> 1]) : lo2(tq[k >> 1]));
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned b = aE1w + 2304 * g;  // rows 4g .. 4g+3, 576 bytes = 72 units apart
                WR2_64_S(0, b, o[4 * g], o[4 * g + 1], 0, 72);
                WR2_64_S(0, b, o[4 * g + 2], o[4 * g + 3], 144, 216);
            }
        }
        // ---- 1b. start fetching the next frame: in flight under the rest of the transform.  Behind the first radix-16 and its
        //      exchange writes (only hand-issued instructions stand between: the compiler's arithmetic is not cut in two), not
        //      in front of it: the compiler folds the window products of rows 0 .. 7 into the first butterflies (fma: these are the
        //      bits every result has had since round 2), so the image is read until then -- moved in place before its last
        //      use, the compiler kept the old image beside the new one and copied it, 16 v_mov_b64 per frame
        if (f + 1 < fEnd) {
            int tn = t + 1, cn = clip;
            if (tn == a.timeLength) {
                tn = 0;
                ++cn;
            }
            const float *pn = a.x + (long long)cn * a.clipStride + (long long)tn * a.hop;
            bool whole = true;
            if constexpr (SHIFT > 0) {
                if (tn != 0) {
                    // in place; aligned frames: the SHIFT new rows are requested by hand from the scalar address of row
                    // 16 - SHIFT (afx_frameops.h) and waited for by hand before this frame's row stores
                    shift_rows_inplace<SHIFT>(raw);  // (afx_asm.h)
                    if (a.aligned) {
                        rows_fetch_new_s<SHIFT, AFX_V2_NT>(raw, vRaw, pn + 128 * (16 - SHIFT));
                    } else {
                        // (nothing is in flight here -- this frame's hand-issued loads are in the other arm, the last frame's
                        //  were waited for before its row stores -- but the compiler uses the image's registers for this arm's
                        //  addresses, and the linear scan of tests/test_isa_forms.py reads the arms one after the other: the
                        //  wait says so there, and costs nothing; the addresses are formed behind it: they have its zero added)
                        int z = 0;
                        VM_WAIT_ALL_AT(z);
                        fetch(pn + z, 16 - SHIFT);
                    }
                    whole = false;
                }
            }
            if (whole) {
                int z = 0;
                if constexpr (SHIFT > 0) VM_WAIT_ALL_AT(z);  // (as above)
                fetch(pn + z, 0);
            }
        }
        wave_lds_sync();
        MEL_PHASE(2);
        {
            v4f rq[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) RD128_S(1, rq[jj], aE1r, 64 * jj);
            wave_lds_sync();
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                PIN(rq[jj]);
                v[2 * jj] = lo2(rq[jj]);
                v[2 * jj + 1] = hi2(rq[jj]);
            }
        }

        // ---- 2b. radix-16 over m1 -> image V[q = k1 + 16 j1][m2], NOT yet multiplied by W_64^(m2 j1): the reader of a base
        //      q applies the three twiddles of its row j1 = q >> 4 (stage 3: 12 products per lane where the writer had 15) ----
        MEL_PHASE(3);
        if (!KO_ON(5)) dft16(v);
        {
            v2 o[16];
#pragma unroll
            for (int j1 = 0; j1 < 16; ++j1) o[j1] = v[rev4(j1)];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned b = aE2w + 2048 * g;  // j1 = 4g .. 4g+3, 512 bytes = 64 units apart
                WR2_64_S(0, b, o[4 * g], o[4 * g + 1], 0, 64);
                WR2_64_S(0, b, o[4 * g + 2], o[4 * g + 3], 128, 192);
            }
        }
        wave_lds_sync();

        // ---- 3. last radix-4 + real-input split -> spectrum values in registers --------------
        MEL_PHASE(4);
        float pk[2][4], pq[2][4], p512;  // |X|^2 (CPLX: real parts)
        float ik[CPLX ? 2 : 1][4], iq[CPLX ? 2 : 1][4], i512 = 0.f;  // CPLX: imaginary parts
        {
            // per s: the two bases' image rows, their W_64 rows (16 + 8 bytes each: W^j1, W^2j1 | W^3j1) and the split twiddles --
            // ten reads, all requested up front; s = 0 is waited for by count.  TAB_LATE (the STFT instantiations, whose
            // stage 3 is their register peak: up front they spilled): the six table reads of s = 1 are requested behind the
            // twiddle products of s = 0, whose W_64 rows are dead by then
#ifdef AFX_V2_TABLATE  // (measurement: every instantiation; the headline is the same with it, profiles/r10_ab_headline.txt (e))
            constexpr bool TAB_LATE = true;
#else
            constexpr bool TAB_LATE = STFT;
#endif
            v4f zalo[2], zahi[2], zblo[2], zbhi[2], wlo[2], whi[2], ta12[2], tb12[2];
            v2 ta3[2], tb3[2];
            auto tables_s1 = [&]() {
                RD128_S(2, ta12[1], aTwA, 4 * TW2_PITCH);
                RD64_S(2, ta3[1], aTwA, 4 * TW2_PITCH + 16);
                RD128_S(2, tb12[1], aTwB1, 0);
                RD64_S(2, tb3[1], aTwB1, 16);
                RD128_S(2, wlo[1], aT3lo, 2048);
                RD128_S(2, whi[1], aT3hi, 2048);
            };
            RD128_S(1, zalo[0], aAlo, 0);
            RD128_S(1, zahi[0], aAhi, 0);
            RD128_S(1, zblo[0], aB0lo, 0);
            RD128_S(1, zbhi[0], aB0hi, 0);
            RD128_S(2, ta12[0], aTwA, 0);
            RD64_S(2, ta3[0], aTwA, 16);
            RD128_S(2, tb12[0], aTwB0, 0);
            RD64_S(2, tb3[0], aTwB0, 16);
            RD128_S(2, wlo[0], aT3lo, 0);
            RD128_S(2, whi[0], aT3hi, 0);
            RD128_S(1, zalo[1], aAlo, 2048);
            RD128_S(1, zahi[1], aAhi, 2048);
            RD128_S(1, zblo[1], aB1lo, 0);
            RD128_S(1, zbhi[1], aB1hi, 0);
            if constexpr (!TAB_LATE) tables_s1();
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s == 0) LDS_WAIT_N(TAB_LATE ? 4 : 10);
                else LDS_WAIT_N(0);
                PIN(zalo[s]); PIN(zahi[s]); PIN(zblo[s]); PIN(zbhi[s]); PIN(wlo[s]); PIN(whi[s]);
                PIN(ta12[s]); PIN(ta3[s]); PIN(tb12[s]); PIN(tb3[s]);
                v2 za0 = lo2(zalo[s]), za1 = hi2(zalo[s]), za2 = lo2(zahi[s]), za3 = hi2(zahi[s]);
                v2 zb0 = lo2(zblo[s]), zb1 = hi2(zblo[s]), zb2 = lo2(zbhi[s]), zb3 = hi2(zbhi[s]);
                if (!KO_ON(5)) {
                    // V[q][m2] W_64^(m2 (q >> 4)), m2 = 1, 2, 3 (lane 0: row 0 of its base 0 holds (1, -0), base 128 has row 8)
                    za1 = cmul(za1, lo2(ta12[s]));
                    za2 = cmul(za2, hi2(ta12[s]));
                    za3 = cmul(za3, ta3[s]);
                    zb1 = cmul(zb1, lo2(tb12[s]));
                    zb2 = cmul(zb2, hi2(tb12[s]));
                    zb3 = cmul(zb3, tb3[s]);
                }
                if constexpr (TAB_LATE) {
                    if (s == 0) {
                        PIN(za1); PIN(za2); PIN(za3); PIN(zb1); PIN(zb2); PIN(zb3);  // (the products stand before the requests)
                        tables_s1();
                    }
                }
                dft4(za0, za1, za2, za3);  // Z[q + 256 j]
                dft4(zb0, zb1, zb2, zb3);  // Z[q' + 256 j], q' the mirror base (lane 0, s = 0: 128)
                v2 A0 = za0, A1 = za1, A2 = za2, A3 = za3;
                v2 B0 = zb3, B1 = zb2, B2 = zb1, B3 = zb0;  // partner of Z[q + 256 j] is Z[q' + 256 (3 - j)]
                if (s == 0) {
                    // lane 0: q = 0 mirrors itself and q' = 128 mirrors itself:
                    // (Z0, Z0) -> bins 0, 1024; (Z256, Z768); (Z128, Z896); (Z384, Z640); bin 512 below
                    if constexpr (CPLX) cplx_map(v2{za2.x, -za2.y}, a.specMap == 4, p512, i512);  // X[512] = conj(Z[512])
                    else p512 = za2.x * za2.x + za2.y * za2.y;
                    A2 = lane0 ? zb0 : za2;
                    A3 = lane0 ? zb1 : za3;
                    B0 = lane0 ? za0 : zb3;
                    B1 = lane0 ? za3 : zb2;
                    B2 = lane0 ? zb3 : zb1;
                    B3 = lane0 ? zb2 : zb0;
                }
                if constexpr (CPLX) {
                    const bool sq = a.specMap == 4;
                    const v2 AA[4] = {A0, A1, A2, A3}, BB[4] = {B0, B1, B2, B3};
                    const v2 ww[4] = {lo2(wlo[s]), hi2(wlo[s]), lo2(whi[s]), hi2(whi[s])};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v2 x, y;
                        split_pair_c(AA[j], BB[j], ww[j], x, y);
                        cplx_map(x, sq, pk[s][j], ik[CPLX ? s : 0][j]);
                        cplx_map(v2{y.x, -y.y}, sq, pq[s][j], iq[CPLX ? s : 0][j]);
                    }
                } else {
                    split_pair(A0, B0, lo2(wlo[s]), pk[s][0], pq[s][0]);
                    split_pair(A1, B1, hi2(wlo[s]), pk[s][1], pq[s][1]);
                    split_pair(A2, B2, lo2(whi[s]), pk[s][2], pq[s][2]);
                    split_pair(A3, B3, hi2(whi[s]), pk[s][3], pq[s][3]);
                }
            }
        }
        // every read of the images has returned (lgkmcnt(0) above): the power row may overwrite their tail.
        // CPLX: the imaginary parts' row goes to the START of the wave's region, dead until the next frame's first exchange
        // (held in registers for a second pass over one row they cost 17 registers across the first pass: two waves per
        // SIMD); its zero pad lies inside the images and is rewritten with it
        if constexpr (CPLX) {
            WR2ST_32(aP01 - PROW_OFF, ik[0][0], ik[0][1], 0, 4);
            WR2ST_32(aP23 - PROW_OFF, ik[0][2], ik[0][3], 0, 4);
            WR2ST_32(aP01 - PROW_OFF, ik[1][0], ik[1][1], 1, 5);
            WR2ST_32(aP01 - PROW_OFF, ik[1][2], ik[1][3], 9, 13);
            WR2ST_32(aQs1 - PROW_OFF, iq[0][1], iq[0][0], 9, 13);
            WR2ST_32(aQ23 - PROW_OFF, iq[0][3], iq[0][2], 0, 4);
            WR2ST_32(aQs1 - PROW_OFF, iq[1][3], iq[1][2], 0, 4);
            WR2ST_32(aQs1 - PROW_OFF, iq[1][1], iq[1][0], 8, 12);
            float *prowI = reinterpret_cast<float *>(wreg);
            if (lane0) prowI[512] = i512;
            prowI[1025 + lane] = 0.f;
            if (lane < PROW_F - 1025 - 64) prowI[1025 + 64 + lane] = 0.f;
        }
        WR2ST_32_S(4, aP01, pk[0][0], pk[0][1], 0, 4);
        WR2ST_32_S(4, aP23, pk[0][2], pk[0][3], 0, 4);
        WR2ST_32_S(4, aP01, pk[1][0], pk[1][1], 1, 5);
        WR2ST_32_S(4, aP01, pk[1][2], pk[1][3], 9, 13);
        WR2ST_32_S(4, aQs1, pq[0][1], pq[0][0], 9, 13);
        WR2ST_32_S(4, aQ23, pq[0][3], pq[0][2], 0, 4);
        WR2ST_32_S(4, aQs1, pq[1][3], pq[1][2], 0, 4);
        WR2ST_32_S(4, aQs1, pq[1][1], pq[1][0], 8, 12);
        if (lane0) prow[512] = p512;
        wave_lds_sync();
#pragma unroll
        for (int pass = 0; pass < (CPLX ? 2 : 1); ++pass) {
        const unsigned bpa = (CPLX && pass) ? apa - PROW_OFF : apa, bpb = (CPLX && pass) ? apb - PROW_OFF : apb;
        const unsigned bpc = (CPLX && pass) ? apc - PROW_OFF : apc;
        if (!CPLX && a.specMap) {
            // magnitude / norm exponent (rare modes): one pass over the row in LDS.  (Applied to the 17 register values
            // before the stores, the two branches' results met the plain path's in different registers and the plain
            // path paid 17 moves per frame for it.)
            for (int k = lane; k < 1025; k += 64) {
                const float p = prow[k];
                prow[k] = a.specMap == 1 ? sqrtf(p) : powf(p, a.normValue);
            }
            wave_lds_sync();
        }

        if constexpr (STFT) {
            // ---- 4'. the row itself: 16-byte reads of the natural-order row, 1 KB per store instruction of the wave ----
            MEL_PHASE(6);
            raw_landed();
            float *orow = a.out + rowOff;
            if (a.vecOut) {
                const float4 *p4 = reinterpret_cast<const float4 *>(prow);
                float4 *o4 = reinterpret_cast<float4 *>(orow);
                float4 q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = p4[lane + 64 * i];
#pragma unroll
                for (int i = 0; i < 4; ++i) o4[lane + 64 * i] = q[i];
                if (lane0) o4[256] = p4[256];  // bin 1024 and three words of the zero pad
            } else {
                for (int k = lane; k < a.binCount; k += 64) orow[k] = prow[a.binLo + k];
            }
        } else {
        MEL_PHASE(5);
        // ---- 4. banded filter bank: weights by ds_read_b128, power row by immediate-offset
        //         ds_read_b64 (conflict-free by the plan's bank-aware lane assignment); the NEXT
        //         block of four quads is requested before this block's values are waited for --------
        float accA, accB, accC = 0.f;
        if constexpr (PC > 0) {
            v2 sA, sB, sC;
            band_stage3<TA, TB, PC, 4, CPLX>(awr, bpa, bpb, bpc, contB, contC, sA, sB, sC);
            accA = sA.x + sA.y;
            accB = sB.x + sB.y;
            accC = sC.x + sC.y;
        } else {
            v2 sA, sB;
            band_stage<TA, TB, 4, CPLX>(awr, bpa, bpb, sA, sB);
            accA = sA.x + sA.y;
            accB = sB.x + sB.y;
        }
        if (!CPLX && !SPLIT && a.postPow) {
            accA = powf(accA, a.normValue);
            accB = powf(accB, a.normValue);
            if constexpr (PC > 0) accC = powf(accC, a.normValue);
        }
        MEL_PHASE(6);
        // ---- 5. store (first the cepstra of the 16 rows stored before this one, if that many wait) ----
        if (pass == 0) raw_landed();  // (in front of the cepstrum block's own wait and of the row stores)
        if constexpr (CC != 0 && !SPLIT) {
            if (ccN == AFX_V2_CCEVERY) cc_block(f - AFX_V2_CCEVERY, (rowOff >> 7) - AFX_V2_CCEVERY, AFX_V2_CCEVERY);
        }
        float *const srow = ((CPLX && pass) ? a.outIm : a.out) + rowOff;  // wave-uniform
        if constexpr (SPLIT) {
            // slot results -> LDS (start of the wave's region: the image there is dead since stage 3),
            // then every row is the sum of its segments in ascending bins
            float *part = reinterpret_cast<float *>(wreg + (CPLX ? PROW_F * 4 : 0));  // (CPLX: behind the imaginary parts' row)
            static_assert(PROW_F * 4 + 129 * 4 <= PROW_OFF, "segment sums must fit between the two rows");
            part[lane] = accA;
            part[64 + lane] = accB;
            if (lane0) part[128] = 0.f;
            wave_lds_sync();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned u = h ? seg1 : seg0;
                float sum = part[u & 255u] + part[(u >> 8) & 255u];
                sum += part[(u >> 16) & 255u];
                sum += part[u >> 24];
                if (!CPLX && a.postPow) sum = powf(sum, a.normValue);
                if (lane + 64 * h < a.num) GST32_S(vLane, sum, srow + 64 * h);
            }
        } else {
            if (okA) GST32_S(vRowA, accA, srow);
            if (okB) GST32_S(vRowB, accB, srow);
            if constexpr (PC > 0) {
                if (okC) GST32_S(vRowC, accC, srow);
            }
        }
        if constexpr (CC != 0) {
            ++ccN;
            // the wave's last rows (drains its last stores).  Split plans: ONE call site, behind the row's stores where the
            // band stage's values are dead (beside them the block spilled 336-656 bytes per lane); its wait then covers the
            // stores of the 16th row as well, once per 16 frames
            if (f + 1 == fEnd || (SPLIT && ccN == 16)) cc_block(f + 1 - ccN, (rowOff >> 7) + 1 - ccN, ccN);
        }
        }  // !STFT
        wave_lds_sync();  // the next frame overwrites the images / the power row

        }  // pass

#ifdef AFX_V2_STAMPS
        ++stampN;
        if (lane0 && (stampN & 15) == 0 && STAMP_HEAD + (stampN >> 4) <= STAMP_WORDS) stamp[STAMP_HEAD - 1 + (stampN >> 4)] = __builtin_amdgcn_s_memtime();
#endif
        rowOff += rowPitch;
        if (++t == a.timeLength) {
            t = 0;
            ++clip;
        }
    }
    }  // runs
#ifdef AFX_V2_STAMPS
    if (lane0) {
        stamp[1] = __builtin_amdgcn_s_memtime();
        stamp[3] = (unsigned long long)stampN;
    }
#endif
}

// window (hWindow != nullptr) and twiddle tables of the blob, byte offsets T_WIN / T_TW1 / T_TW2 / T_TW3
void fill_tables(float *tab, const float *hWindow) {
    const double PI = 3.14159265358979323846;
    // window and W_1024^(lane k1) in pair layout: entry (n1, lane) at float2 index 128 (n1 >> 1) + 2 lane + (n1 & 1)
    float *win = tab + T_WIN / 4, *tw1 = tab + T_TW1 / 4, *tw2 = tab + T_TW2 / 4, *tw3 = tab + T_TW3 / 4;
    for (int n1 = 0; n1 < 16; ++n1)
        for (int l = 0; l < 64; ++l) {
            const int at = 2 * (128 * (n1 >> 1) + 2 * l + (n1 & 1));
            const int n = 64 * n1 + l;
            if (hWindow) {
                win[at] = hWindow[2 * n];
                win[at + 1] = hWindow[2 * n + 1];
            }
            const double ang = -2.0 * PI * (double)(n1 * l) / MC;  // twiddles in double, rounded once
            tw1[at] = (float)cos(ang);
            tw1[at + 1] = (float)sin(ang);
        }
    // W_64^(m j), m = 1, 2, 3, of the image rows V[q][m] with j = q >> 4: row j holds m = 1, 2 in its first 16 bytes, m = 3 and a
    // pad in its second (row 0: (1, -0) three times, the values the writer-side table had in its column j = 0)
    for (int j = 0; j < 16; ++j) {
        for (int m = 1; m < 4; ++m) {
            const double ang = -2.0 * PI * (double)(m * j) / 64.0;
            tw2[(TW2_PITCH / 4) * j + 2 * (m - 1)] = (float)cos(ang);
            tw2[(TW2_PITCH / 4) * j + 2 * (m - 1) + 1] = (float)sin(ang);
        }
        tw2[(TW2_PITCH / 4) * j + 6] = tw2[(TW2_PITCH / 4) * j + 7] = 0.f;
    }
    // 0.5 W_2048^bin of the P-bin of slot (s, lane, m); 16-byte halves swapped when bit 3 of lane is set
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l < 64; ++l)
            for (int m = 0; m < 4; ++m) {
                int bin = l + 64 * s + 256 * m;
                if (s == 0 && l == 0 && m >= 2) bin = m == 2 ? 128 : 384;  // lane 0 carries the self-mirrored base
                const double ang = -2.0 * PI * (double)bin / NFFT;
                const int at = 2 * (4 * (64 * s + l) + 2 * ((m >> 1) ^ ((l >> 3) & 1)) + (m & 1));
                tw3[at] = (float)(0.5 * cos(ang));
                tw3[at + 1] = (float)(0.5 * sin(ang));
            }
}

constexpr AfxMelVariant kVariants[] = {{48, 16}, {72, 32}};

// Workgroups of a launch and the frames each owns: afx_frame_split's shape (afx_device.h) with ONE round of workgroups -- the waves
// of a workgroup claim their runs, so a second round only adds a second set of tails (profiles/r07_ab_headline.txt); a call that
// cannot fill the round with 16-frame runs is spread over all CUs as before.  AFX_MEL_CUS=N sizes the grid as if the device had N CUs
// (the tests' way to long ranges per workgroup on few frames; read per launch)
long long wg_ranges(long long total, int waves, long long *framesPerWg) {
    const char *e = getenv("AFX_MEL_CUS");
    const int asked = e ? atoi(e) : 0;
    const int cus = asked > 0 ? asked : afx_cu_count();
    long long fpw;
    long long blocks = afx_frame_split(total, cus, waves, 1, &fpw);
    *framesPerWg = fpw * waves;
    if (*framesPerWg > (1ll << 30)) {  // the claim counter is one 32-bit word
        *framesPerWg = 1ll << 30;
        blocks = (total + *framesPerWg - 1) / *framesPerWg;
    }
    return blocks;
}

#ifdef AFX_V2_STAMPS
// diagnostic builds: a fresh stamp buffer per launch; after the launch it is waited for and written to AFX_V2_STAMPS_FILE
unsigned long long *stamps_begin(long long blocks, int waves) {
    unsigned long long *d = nullptr;
    const size_t n = (size_t)blocks * waves * STAMP_WORDS * 8;
    if (hipMalloc(&d, n) != hipSuccess || hipMemset(d, 0, n) != hipSuccess) return nullptr;
    return d;
}
void stamps_end(unsigned long long *d, long long blocks, int waves, void *stream) {
    const size_t n = (size_t)blocks * waves * STAMP_WORDS;
    std::vector<unsigned long long> h(n);
    (void)hipStreamSynchronize((hipStream_t)stream);
    if (hipMemcpy(h.data(), d, n * 8, hipMemcpyDeviceToHost) == hipSuccess)
        if (const char *name = getenv("AFX_V2_STAMPS_FILE"))
            if (FILE *fp = fopen(name, "wb")) {
                fwrite(h.data(), 8, n, fp);
                fclose(fp);
            }
    (void)hipFree(d);
}
#endif

template <int TA, int TB, int SHIFT, bool SPLIT, int CC, bool TEMPORAL, bool CPLX = false, int PC = 0>
int launch_variant(const AfxMelPlan *p, const AfxMelFusedArgs *a, void *stream) {
    const long long total = (long long)a->batch * a->timeLength;
    if (total <= 0) return AFX_OK;
    constexpr int NWV = waves_of(CPLX);
    long long fpg;
    const long long blocks = wg_ranges(total, NWV, &fpg);

    KArgs2 k;
    memset(&k, 0, sizeof(k));
    k.x = a->x;
    k.clipStride = a->clipStride;
    k.totalFrames = total;
    k.timeLength = a->timeLength;
    k.hop = a->hop;
    k.framesPerWg = fpg;
    k.aligned = ((a->clipStride & 1) == 0) && ((a->hop & 1) == 0) && ((reinterpret_cast<uintptr_t>(a->x) & 7) == 0);
    k.tab = reinterpret_cast<const float4 *>(p->dTab);
    k.meta = p->dMeta;
    k.specMap = a->specMap;
    k.postPow = a->postPow;
    k.normValue = a->normValue;
    k.out = a->out;
    k.outIm = a->outIm;
    k.num = p->num;
    k.dct = a->dct;
    k.ccNum = a->ccNum;
    k.ccCbrt = a->ccRectify == 1;
    k.cc = a->cc;
    k.energy = a->energy;
    k.rms = a->rms;
    k.zcr = a->zcr;
    constexpr size_t lds = (size_t)block_lds_bytes(TA, TB, CC == 1, PC);
    static_assert(lds <= 163840, "workgroup LDS budget");
#ifdef AFX_V2_STAMPS
    if (!(k.stamps = stamps_begin(blocks, NWV))) return AFX_ERR_HIP;
#endif
    AFX_LAUNCH_DYN_LDS((k_stft_mel_v2<TA, TB, SHIFT, SPLIT, CC, TEMPORAL, CPLX, false, PC>), dim3((unsigned)blocks), dim3(NWV * 64), lds, stream, k);
    AFX_LAUNCH_CHECK("k_stft_mel_v2");
#ifdef AFX_V2_STAMPS
    stamps_end(k.stamps, blocks, NWV, stream);
#endif
    return AFX_OK;
}

template <int TA, int TB, bool SPLIT, int CC, bool TEMPORAL, int PC = 0>
int launch_hop(const AfxMelPlan *p, const AfxMelFusedArgs *a, void *stream) {
    // register re-use of the overlapping frames for hop = 128 * SHIFT: N/8, N/4, N/2
#ifdef AFX_EXPERIMENTS  // measurement builds only (make EXTRA=-DAFX_EXPERIMENTS): AFX_EXP_MEL=noshift fetches every frame whole
    if (const char *e = getenv("AFX_EXP_MEL"))
        if (strstr(e, "noshift")) return launch_variant<TA, TB, 0, SPLIT, CC, TEMPORAL, false, PC>(p, a, stream);
#endif
    switch (a->hop) {
        case 256: return launch_variant<TA, TB, 2, SPLIT, CC, TEMPORAL, false, PC>(p, a, stream);
        case 512: return launch_variant<TA, TB, 4, SPLIT, CC, TEMPORAL, false, PC>(p, a, stream);
        case 1024: return launch_variant<TA, TB, 8, SPLIT, CC, TEMPORAL, false, PC>(p, a, stream);
        default: return launch_variant<TA, TB, 0, SPLIT, CC, TEMPORAL, false, PC>(p, a, stream);
    }
}

template <int TA, int TB>
int launch(const AfxMelPlan *p, const AfxMelFusedArgs *a, void *stream) {
    const bool cc = a->cc != nullptr, tmp = a->energy != nullptr;
    if (a->specMap >= 3) {  // complex results: S (3) or S^2 (4); hop N/4 with register re-use, any other hop plain
        if (cc || tmp) return AFX_ERR_UNSUPPORTED;
        if (!a->outIm) return AFX_ERR_ARG;
        if (a->hop == 512)
            return p->split ? launch_variant<TA, TB, 4, true, 0, false, true>(p, a, stream)
                            : launch_variant<TA, TB, 4, false, 0, false, true>(p, a, stream);
        return p->split ? launch_variant<TA, TB, 0, true, 0, false, true>(p, a, stream)
                        : launch_variant<TA, TB, 0, false, 0, false, true>(p, a, stream);
    }
    if (cc && tmp) return AFX_ERR_UNSUPPORTED;  // callers run the cepstra separately for temporal objects
    if (cc) {
        if (a->ccNum < 1 || a->ccNum > 16 || !a->dct || !a->out || p->num > 128 || (p->num & 3)) return AFX_ERR_UNSUPPORTED;
        if (a->ccRectify != 0 && a->ccRectify != 1) return AFX_ERR_UNSUPPORTED;
        if constexpr (block_lds_bytes(TA, TB, true) <= 163840)  // the headline form: DCT operand in LDS
            if (!p->split && p->num == 128 && a->ccRectify == 0) return launch_hop<TA, TB, false, 1, false>(p, a, stream);
        // the general form (afx_ccblock.h): hop N/4 with the register re-use of the overlapping frames, any other hop plain
        if (a->hop == 512)
            return p->split ? launch_variant<TA, TB, 4, true, 2, false>(p, a, stream) : launch_variant<TA, TB, 4, false, 2, false>(p, a, stream);
        return p->split ? launch_variant<TA, TB, 0, true, 2, false>(p, a, stream) : launch_variant<TA, TB, 0, false, 2, false>(p, a, stream);
    }
    if (tmp) {
        if (!a->rms || !a->zcr) return AFX_ERR_ARG;
        return p->split ? launch_hop<TA, TB, true, 0, true>(p, a, stream)
                        : launch_hop<TA, TB, false, 0, true>(p, a, stream);
    }
    return p->split ? launch_hop<TA, TB, true, 0, false>(p, a, stream)
                    : launch_hop<TA, TB, false, 0, false>(p, a, stream);
}

// the routes of launch() for a packed plan (whole rows only): same checks, same choices
template <int PA, int PB, int PC>
int launch_packed(const AfxMelPlan *p, const AfxMelFusedArgs *a, void *stream) {
    const bool cc = a->cc != nullptr, tmp = a->energy != nullptr;
    if (a->specMap >= 3) {
        if (cc || tmp) return AFX_ERR_UNSUPPORTED;
        if (!a->outIm) return AFX_ERR_ARG;
        if (a->hop == 512) return launch_variant<PA, PB, 4, false, 0, false, true, PC>(p, a, stream);
        return launch_variant<PA, PB, 0, false, 0, false, true, PC>(p, a, stream);
    }
    if (cc && tmp) return AFX_ERR_UNSUPPORTED;
    if (cc) {
        if (a->ccNum < 1 || a->ccNum > 16 || !a->dct || !a->out || p->num > 128 || (p->num & 3)) return AFX_ERR_UNSUPPORTED;
        if (a->ccRectify != 0 && a->ccRectify != 1) return AFX_ERR_UNSUPPORTED;
        static_assert(block_lds_bytes(PA, PB, true, PC) <= 163840, "the headline form: DCT operand in LDS");
        if (p->num == 128 && a->ccRectify == 0) return launch_hop<PA, PB, false, 1, false, PC>(p, a, stream);
        if (a->hop == 512) return launch_variant<PA, PB, 4, false, 2, false, false, PC>(p, a, stream);
        return launch_variant<PA, PB, 0, false, 2, false, false, PC>(p, a, stream);
    }
    if (tmp) {
        if (!a->rms || !a->zcr) return AFX_ERR_ARG;
        return launch_hop<PA, PB, false, 0, true, PC>(p, a, stream);
    }
    return launch_hop<PA, PB, false, 0, false, PC>(p, a, stream);
}

// the compiled layouts (a, b, c) of the packed plan: 48 slots per lane.  (24, 12, 8) and (20, 12, 12), 44 slots, hold mel-128 at
// 16 kHz too, but the planner places them only with 5 and 3 lane pairs on one bank pair (afx_bandplan.c)
constexpr int kPacks[][3] = {{24, 12, 12}};

int run(const AfxMelPlan *p, const AfxMelFusedArgs *a, void *stream) {
    if (p->pack == 1) return launch_packed<24, 12, 12>(p, a, stream);
    return p->variant == 0 ? launch<48, 16>(p, a, stream) : launch<72, 32>(p, a, stream);
}

void fill_stft_tables(float *tab) { fill_tables(tab, nullptr); }  // the twiddle blob of the STFT instantiations (afx_device_table)

template <int SHIFT>
int launch_stft2k(const AfxStftArgs *a, const float *tab, void *stream) {
    const long long total = (long long)a->batch * a->timeLength;
    long long fpg;
    const long long blocks = wg_ranges(total, WAVES, &fpg);
    KArgs2 k;
    memset(&k, 0, sizeof(k));
    k.x = a->x;
    k.clipStride = a->clipStride;
    k.totalFrames = total;
    k.timeLength = a->timeLength;
    k.hop = a->hop;
    k.framesPerWg = fpg;
    k.aligned = ((a->clipStride & 1) == 0) && ((a->hop & 1) == 0) && ((reinterpret_cast<uintptr_t>(a->x) & 7) == 0);
    k.tab = reinterpret_cast<const float4 *>(tab);
    k.specMap = a->mode == AFX_SPEC_POWER ? 0 : a->mode == AFX_SPEC_MAG ? 1 : 2;
    k.normValue = a->normValue;
    k.out = a->outRe;
    k.win = a->window;
    k.binLo = a->binLo;
    k.binCount = a->binCount;
    k.outPitch = a->outPitch ? a->outPitch : (long long)a->binCount;
    k.vecOut = a->binLo == 0 && a->binCount == NFFT / 2 + 1 && k.outPitch >= 1028 && (k.outPitch & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(a->outRe) & 15) == 0;
    constexpr size_t lds = (size_t)block_lds_bytes(0, 0, false);
#ifdef AFX_V2_STAMPS
    if (!(k.stamps = stamps_begin(blocks, WAVES))) return AFX_ERR_HIP;
#endif
    AFX_LAUNCH_DYN_LDS((k_stft_mel_v2<0, 0, SHIFT, false, 0, false, false, true>), dim3((unsigned)blocks), dim3(WAVES * 64), lds, stream, k);
    AFX_LAUNCH_CHECK("k_stft_mel_v2 (stft)");
#ifdef AFX_V2_STAMPS
    stamps_end(k.stamps, blocks, WAVES, stream);
#endif
    return AFX_OK;
}

}  // namespace

const AfxMelSize *afx_mel_size2k() {
    static const AfxMelSize size = {11, 0, kVariants, 2, T_BAND, fill_tables, run, kPacks, 1, PROW_F};
    return &size;
}

// The transform's tables as the kernel copies them to LDS (no window): T_BAND bytes at `tab`, which holds `bytes`; returns T_BAND.
// Host code, no device call.  Nothing on the host side calls it: tests/test_mel_tw2_cpu.py reads the W_64 rows at T_TW2 through it
extern "C" int afxk_mel2k_tables(float *tab, int bytes) {
    if (tab && bytes >= T_BAND) {
        memset(tab, 0, T_BAND);
        fill_tables(tab, nullptr);
    }
    return T_BAND;
}

// The n_fft 2048 wave transform storing its mapped spectrum rows (real results: |S|^2, |S|, |S|^2p) -- the [T, F] rows of the
// dense-bank route and of the STFT / linear-scale objects (stft_algorithm.c:717-803, bft_algorithm.c:489-504); every frame inside
// its clip.  AFX_ERR_UNSUPPORTED: not this kernel's case (afxk_stft then runs k_stft_wave / the size-generic kernel)
extern "C" int afxk_stft2k(const AfxStftArgs *a, void *stream) {
    if (a->radix2Exp != 11 || a->bandStart || a->energy || a->padLeft != 0 || a->hop < 1 || a->binLo < 0 || a->binCount < 1 ||
        a->binLo + a->binCount > NFFT / 2 + 1 || (long long)(a->timeLength - 1) * a->hop + NFFT > a->dataLength ||
        (reinterpret_cast<uintptr_t>(a->window) & 7) != 0)
        return AFX_ERR_UNSUPPORTED;
    if (a->mode != AFX_SPEC_POWER && a->mode != AFX_SPEC_MAG && a->mode != AFX_SPEC_POWER_NORM) return AFX_ERR_UNSUPPORTED;
    if (!a->outRe) return AFX_ERR_ARG;
    const long long total = (long long)a->batch * a->timeLength;
    if (total <= 0) return AFX_OK;
    if (total > 0x7fffffffLL) return AFX_ERR_UNSUPPORTED;
    const float *tab = afx_device_table<fill_stft_tables>((size_t)tab_bytes(0, 0));
    if (!tab) return AFX_ERR_UNSUPPORTED;
    switch (a->hop) {
        case 256: return launch_stft2k<2>(a, tab, stream);
        case 512: return launch_stft2k<4>(a, tab, stream);
        case 1024: return launch_stft2k<8>(a, tab, stream);
        default: return launch_stft2k<0>(a, tab, stream);
    }
}
