// afx_melparts.h -- device pieces shared by the fused STFT -> filter-bank kernels (afx_melfused{512,1k,2,4k2}.hip): one
// definition each.  The wave transforms, the frame loops and the power-row layouts stay in their files; what is here is what
// those files had word for word.  Only what both afx_asm.h and its host stand-in (tests/emu/hip/afx_asm.h) provide is used,
// and afx_frameops.h, which carries its own C twins for the emulated builds.
// (stft_map, which the STFT kernels without hand-issued LDS accesses share too, is in afx_pkmath.h.)
#ifndef AFX_MELPARTS_H
#define AFX_MELPARTS_H

#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_pkmath.h"
#include "afx_frameops.h"

typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v2 lo2(v4f q) { return v2{q.x, q.y}; }
__device__ __forceinline__ v2 hi2(v4f q) { return v2{q.z, q.w}; }

// Orders this wave's LDS stores before its later LDS loads of other lanes' data: DS operations of
// one wave execute in issue order, lgkmcnt(0) drains them, the wave barrier pins the compiler.
// Deliberately NOT a fence (that would also drain vmcnt: the prefetch and the previous stores).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
}

// Real-input split of the packed transform Z (M complex points of 2 M real samples): |X|^2 of the conjugate pair
// (k, M - k) from A = Z[k], B = Z[M - k], w = 0.5 W_2M^k
__device__ __forceinline__ void split_pair(v2 A, v2 B, v2 w, float &pk, float &pq) {
    const v2 e2 = pk_add_conj(A, B);   // 2 E
    const v2 d = pk_sub_conj(A, B);    // 2 i O
    const v2 wo = cmul_mi(d, w);       // W O
    const v2 p = pair_power(e2, wo);   // (|x|^2, |y|^2) of x = e2 / 2 + wo = X[k], y = e2 / 2 - wo = conj(X[M - k]) (afx_frameops.h)
    pk = p.x;
    pq = p.y;
}
// complex results: the spectrum values themselves, x = X[k], y = conj(X[M - k])
__device__ __forceinline__ void split_pair_c(v2 A, v2 B, v2 w, v2 &x, v2 &y) {
    const v2 e2 = pk_add_conj(A, B);
    const v2 d = pk_sub_conj(A, B);
    const v2 wo = cmul_mi(d, w);
    x = e2 * 0.5f + wo;
    y = e2 * 0.5f - wo;
}
// (re, im) of the requested complex result from a spectrum value c: S (sq = false) or S^2 (bft_algorithm.c:457-485)
__device__ __forceinline__ void cplx_map(v2 c, bool sq, float &re, float &im) {
    re = sq ? c.x * c.x - c.y * c.y : c.x;
    im = sq ? 2.f * (c.x * c.y) : c.y;
}
// the two in one, as n_fft 512 / 1024 have it: (kr, ki) = X[k] or its square, (qr, qi) = X[M - k] or its square
__device__ __forceinline__ void split_pair_cmap(v2 A, v2 B, v2 w, bool sq, float &kr, float &ki, float &qr, float &qi) {
    const v2 e2 = pk_add_conj(A, B);
    const v2 d = pk_sub_conj(A, B);
    const v2 wo = cmul_mi(d, w);
    const v2 x = e2 * 0.5f + wo;
    const v2 y = e2 * 0.5f - wo;
    if (sq) {
        kr = x.x * x.x - x.y * x.y;
        ki = 2.f * (x.x * x.y);
        qr = y.x * y.x - y.y * y.y;
        qi = -2.f * (y.x * y.y);
    } else {
        kr = x.x;
        ki = x.y;
        qr = y.x;
        qi = -y.y;
    }
}

// Knock-out measurement builds (make EXTRA=-DAFX_KO=<mask>; results are WRONG, timing only): bit s drops the LDS traffic of
// site class s -- 0 exchange writes, 1 exchange / image reads, 2 table reads (window, twiddles), 3 band-stage reads, 4 power-row
// writes -- and leaves the arithmetic on whatever the registers hold; bit 5 drops the second radix-16 layer's arithmetic,
// bit 6 the band-stage multiply-adds.  What the step time does NOT lose says what does not bind it (profiles/r05_ab_headline.txt (c)).
// Classes 0, 1, 2, 4, 5 are sites of afx_melfused2.hip; 3 and 6 are the band stage below.
#ifdef AFX_KO
#define KO_ON(s) (((AFX_KO) >> (s)) & 1)
#define RD128_S(s, dst, addr, off) do { if (KO_ON(s)) asm volatile("" : "=v"(dst)); else RD128(dst, addr, off); } while (0)
#define RD64_S(s, dst, addr, off) do { if (KO_ON(s)) asm volatile("" : "=v"(dst)); else RD64(dst, addr, off); } while (0)
#define WR2_64_S(s, addr, d0, d1, o0, o1) do { if (KO_ON(s)) asm volatile("" ::"v"(d0), "v"(d1)); else WR2_64(addr, d0, d1, o0, o1); } while (0)
#define WR2ST_32_S(s, addr, d0, d1, o0, o1) do { if (KO_ON(s)) asm volatile("" ::"v"(d0), "v"(d1)); else WR2ST_32(addr, d0, d1, o0, o1); } while (0)
#else
#define KO_ON(s) 0
#define RD128_S(s, dst, addr, off) RD128(dst, addr, off)
#define RD64_S(s, dst, addr, off) RD64(dst, addr, off)
#define WR2_64_S(s, addr, d0, d1, o0, o1) WR2_64(addr, d0, d1, o0, o1)
#define WR2ST_32_S(s, addr, d0, d1, o0, o1) WR2ST_32(addr, d0, d1, o0, o1)
#endif

// The banded filter bank of one lane: its A row (TA taps) and B row (TB taps) against the power row in LDS.  awr: the lane's
// weights, [TA + TB (+ 4)] floats read by ds_read_b128; apa / apb: the power row at the rows' first bins, read by
// immediate-offset ds_read_b64 (conflict-free by the plan's bank-aware lane assignment) -- three loop-invariant LDS byte
// addresses.  Quads of taps go in blocks of BLK; the NEXT block is requested before this block's values are waited for.
// PINSUMS: this block's sums are pinned before the next block's requests: left free, the scheduler sinks every multiply-add
// behind the last request and keeps all the operands alive (212-532 bytes of scratch per lane at n_fft 512 / 1024; the
// complex instantiations of n_fft 2048: 240-256 registers + 264 bytes of scratch -> 182).  Where it is off the free
// schedule is the measured one.  sA / sB: the rows' sums in even / odd taps.
template <int TA, int TB, int BLK, bool PINSUMS>
__device__ __forceinline__ void band_stage(unsigned awr, unsigned apa, unsigned apb, v2 &sA, v2 &sB) {
    constexpr int QA = TA / 4, QB = TB / 4, QT = QA + QB, NB = (QT + BLK - 1) / BLK;
    static_assert(BLK <= 4, "the wait ladder counts up to four quads in flight");
    sA = v2{0.f, 0.f};
    sB = v2{0.f, 0.f};
    v4f w[2][BLK];
    v2 p0[2][BLK], p1[2][BLK];
    auto request = [&](int blk, v4f (&wq)[BLK], v2 (&q0v)[BLK], v2 (&q1v)[BLK]) {
#pragma unroll
        for (int i = 0; i < BLK; ++i) {
            const int q = blk * BLK + i;
            if (q >= QT) continue;
            RD128_S(3, wq[i], awr, 16 * q);
            if (q < QA) {
                RD64_S(3, q0v[i], apa, 16 * q);
                RD64_S(3, q1v[i], apa, 16 * q + 8);
            } else {
                RD64_S(3, q0v[i], apb, 16 * (q - QA));
                RD64_S(3, q1v[i], apb, 16 * (q - QA) + 8);
            }
        }
    };
    request(0, w[0], p0[0], p1[0]);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        const int cur = blk & 1;
        const int nextQuads = (blk + 1 < NB) ? ((QT - (blk + 1) * BLK) < BLK ? (QT - (blk + 1) * BLK) : BLK) : 0;
        if (blk + 1 < NB) request(blk + 1, w[cur ^ 1], p0[cur ^ 1], p1[cur ^ 1]);
        if (nextQuads == 4) LDS_WAIT_N(12);
        else if (nextQuads == 3) LDS_WAIT_N(9);
        else if (nextQuads == 2) LDS_WAIT_N(6);
        else if (nextQuads == 1) LDS_WAIT_N(3);
        else LDS_WAIT_N(0);
#pragma unroll
        for (int i = 0; i < BLK; ++i) {
            const int q = blk * BLK + i;
            if (q >= QT) continue;
            PIN(w[cur][i]);
            PIN(p0[cur][i]);
            PIN(p1[cur][i]);
            if (KO_ON(6)) {
                asm volatile("" ::"v"(w[cur][i]), "v"(p0[cur][i]), "v"(p1[cur][i]));
            } else if (q < QA) {
                sA += lo2(w[cur][i]) * p0[cur][i];
                sA += hi2(w[cur][i]) * p1[cur][i];
            } else {
                sB += lo2(w[cur][i]) * p0[cur][i];
                sB += hi2(w[cur][i]) * p1[cur][i];
            }
        }
        if constexpr (PINSUMS) {
            PIN(sA);
            PIN(sB);
        }
    }
}

// The packed form (AfxBandPack, afx_bandpack.h): ONE stream of PA | PB | PC taps per lane, weights [PA + PB + PC (+ 4)] floats at
// awr, three power-row addresses ap0 / ap1 / ap2.  A partition starts its sum from the one before (cont1 / cont2: it continues
// that row; loop-invariant lane masks) or from zero; s0 / s1 / s2 are the sums at the END of each partition, so a row's
// multiply-adds are those of band_stage, in the same order, whichever partitions it lies in: leading zero weights give
// fma(0, p, +0) = +0, trailing ones s + 0 p = s (finite p).  Requests, waits and pins as in band_stage.
template <int PA, int PB, int PC, int BLK, bool PINSUMS>
__device__ __forceinline__ void band_stage3(unsigned awr, unsigned ap0, unsigned ap1, unsigned ap2, bool cont1, bool cont2, v2 &s0, v2 &s1,
                                            v2 &s2) {
    constexpr int Q0 = PA / 4, Q1 = Q0 + PB / 4, QT = Q1 + PC / 4, NB = (QT + BLK - 1) / BLK;
    static_assert(BLK <= 4, "the wait ladder counts up to four quads in flight");
    static_assert(PA % 4 == 0 && PB % 4 == 0 && PC % 4 == 0 && PA > 0 && PB > 0 && PC > 0, "partitions are whole quads");
    s0 = v2{0.f, 0.f};
    s1 = v2{0.f, 0.f};
    s2 = v2{0.f, 0.f};
    v4f w[2][BLK];
    v2 p0[2][BLK], p1[2][BLK];
    auto request = [&](int blk, v4f (&wq)[BLK], v2 (&q0v)[BLK], v2 (&q1v)[BLK]) {
#pragma unroll
        for (int i = 0; i < BLK; ++i) {
            const int q = blk * BLK + i;
            if (q >= QT) continue;
            RD128_S(3, wq[i], awr, 16 * q);
            if (q < Q0) {
                RD64_S(3, q0v[i], ap0, 16 * q);
                RD64_S(3, q1v[i], ap0, 16 * q + 8);
            } else if (q < Q1) {
                RD64_S(3, q0v[i], ap1, 16 * (q - Q0));
                RD64_S(3, q1v[i], ap1, 16 * (q - Q0) + 8);
            } else {
                RD64_S(3, q0v[i], ap2, 16 * (q - Q1));
                RD64_S(3, q1v[i], ap2, 16 * (q - Q1) + 8);
            }
        }
    };
    request(0, w[0], p0[0], p1[0]);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        const int cur = blk & 1;
        const int nextQuads = (blk + 1 < NB) ? ((QT - (blk + 1) * BLK) < BLK ? (QT - (blk + 1) * BLK) : BLK) : 0;
        if (blk + 1 < NB) request(blk + 1, w[cur ^ 1], p0[cur ^ 1], p1[cur ^ 1]);
        if (nextQuads == 4) LDS_WAIT_N(12);
        else if (nextQuads == 3) LDS_WAIT_N(9);
        else if (nextQuads == 2) LDS_WAIT_N(6);
        else if (nextQuads == 1) LDS_WAIT_N(3);
        else LDS_WAIT_N(0);
#pragma unroll
        for (int i = 0; i < BLK; ++i) {
            const int q = blk * BLK + i;
            if (q >= QT) continue;
            PIN(w[cur][i]);
            PIN(p0[cur][i]);
            PIN(p1[cur][i]);
            if (q == Q0) s1 = cont1 ? s0 : v2{0.f, 0.f};
            if (q == Q1) s2 = cont2 ? s1 : v2{0.f, 0.f};
            if (KO_ON(6)) {
                asm volatile("" ::"v"(w[cur][i]), "v"(p0[cur][i]), "v"(p1[cur][i]));
            } else if (q < Q0) {
                s0 += lo2(w[cur][i]) * p0[cur][i];
                s0 += hi2(w[cur][i]) * p1[cur][i];
            } else if (q < Q1) {
                s1 += lo2(w[cur][i]) * p0[cur][i];
                s1 += hi2(w[cur][i]) * p1[cur][i];
            } else {
                s2 += lo2(w[cur][i]) * p0[cur][i];
                s2 += hi2(w[cur][i]) * p1[cur][i];
            }
        }
        if constexpr (PINSUMS) {
            PIN(s0);
            PIN(s1);
            PIN(s2);
        }
    }
}

#endif /* AFX_MELPARTS_H */
