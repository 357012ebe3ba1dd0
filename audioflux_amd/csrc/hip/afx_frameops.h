// afx_frameops.h -- hand-issued gfx950 sequences of the fused STFT -> filter-bank frame loops (round 8: the loops' vector
// instructions gone through one by one, profiles/r08_ab_headline.txt): what the compiler spent on 64-bit per-lane addresses
// and on a sixth instruction per conjugate pair, written so that every result keeps its bits.  Each helper has its plain-C
// twin below, behind the macro the lane emulator's hip_runtime.h defines (tests/emu): the emulated builds take the twins and
// compile unchanged.  Same rules as afx_asm.h: the op_sel RULE for packed-f32 instructions, one asm statement per
// dependent sequence, loads issued here are waited for by hand (s_waitcnt vmcnt + PIN before the first use).
#ifndef AFX_FRAMEOPS_H
#define AFX_FRAMEOPS_H

#include <afx_asm.h>

typedef float fo_v4 __attribute__((ext_vector_type(4)));

#ifdef AFX_EMU_HIP_RUNTIME_H
// ---- the lane emulator's versions: the same operations in C ------------------------------------------------------------
__device__ __forceinline__ v2 pair_power(v2 e2, v2 wo) {
#pragma clang fp contract(off)  // the products and the sums round separately, as the five instructions do
    const v2 u = {__builtin_fmaf(e2.x, 0.5f, wo.x), __builtin_fmaf(e2.x, 0.5f, -wo.x)};  // (x.x, y.x)
    const v2 v = {__builtin_fmaf(e2.y, 0.5f, wo.y), __builtin_fmaf(e2.y, 0.5f, -wo.y)};  // (x.y, y.y)
    const v2 uu = {u.x * u.x, u.y * u.y}, vv = {v.x * v.x, v.y * v.y};
    return v2{uu.x + vv.x, uu.y + vv.y};
}
template <int S, bool NT>
__device__ __forceinline__ void rows_fetch_new_s(v2 (&r)[16], unsigned voff, const float *sbase) {
    for (int i = 0; i < S; ++i) __builtin_memcpy(&r[16 - S + i], reinterpret_cast<const char *>(sbase) + voff + 512 * i, 8);
}
__device__ __forceinline__ fo_v4 max4_floor(fo_v4 x) {
    return fo_v4{__builtin_fmaxf(x.x, 1e-8f), __builtin_fmaxf(x.y, 1e-8f), __builtin_fmaxf(x.z, 1e-8f), __builtin_fmaxf(x.w, 1e-8f)};
}
__device__ __forceinline__ float max_floor(float x) { return __builtin_fmaxf(x, 1e-8f); }
#define VM_WAIT_ALL_AT(z) ((void)(z))
#define GLD128X4_L2_S(d0, d1, d2, d3, voff, sbase, o0, o1, o2, o3)                                   \
    (__builtin_memcpy(&(d0), reinterpret_cast<const char *>(sbase) + (voff) + (o0), 16),             \
     __builtin_memcpy(&(d1), reinterpret_cast<const char *>(sbase) + (voff) + (o1), 16),             \
     __builtin_memcpy(&(d2), reinterpret_cast<const char *>(sbase) + (voff) + (o2), 16),             \
     __builtin_memcpy(&(d3), reinterpret_cast<const char *>(sbase) + (voff) + (o3), 16))
#else
// ---- |X|^2 of a conjugate pair from e2 = 2 E and wo = W O (split_pair, afx_melparts.h): x = e2 / 2 + wo = X[k],
// y = e2 / 2 - wo = conj(X[M - k]); returns (|x|^2, |y|^2).  The halves are formed directly, U = (x.x, y.x) and
// V = (x.y, y.y), by the two fmas that formed x and y (broadcast selects: src0 and src2 both low or both high, the constant
// low -- none is the select the RULE forbids), then P = U U + V V: every result lane runs fl(fl(x.x^2) + fl(x.y^2)) with the
// roundings of the six-instruction form (2 fma, 2 mul of (x.x, x.y) / (y.x, y.y), 2 scalar adds) -- five instructions.
__device__ __forceinline__ v2 pair_power(v2 e2, v2 wo) {
    v2 u, v;
    asm("v_pk_fma_f32 %0, %2, 0.5, %3 op_sel:[0,0,0] op_sel_hi:[0,0,0] neg_hi:[0,0,1]\n\t"  // (e2x/2 + wox, e2x/2 - wox)
        "v_pk_fma_f32 %1, %2, 0.5, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1] neg_hi:[0,0,1]\n\t"  // (e2y/2 + woy, e2y/2 - woy)
        "v_pk_mul_f32 %0, %0, %0\n\t"
        "v_pk_mul_f32 %1, %1, %1\n\t"
        "v_pk_add_f32 %0, %0, %1"
        : "=&v"(u), "=&v"(v) : "v"(e2), "v"(wo));
    return u;
}

// ---- the register image of overlapping frames whose rows are 512 bytes apart in memory (n_fft 2048: raw[n1] = the float2 at
// 8 (64 n1 + lane) bytes of the frame), refilled behind shift_rows_inplace<S> (afx_asm.h): the S new rows come from the
// wave-uniform address `sbase` (row 16 - S of the next frame, a scalar register pair) + the loop-invariant lane offset
// voff = 8 lane + immediates 512 k -- no per-lane 64-bit pointer is formed.  The new rows are in-out operands, so their old
// values die here and the loads land in place.  NT: the streaming policy of the AFX_V2_NTIN measurement build.  The loads
// are waited for by hand.  (Moves and loads in ONE statement, as rows_shift_fetch has them for n_fft 4096, made hipcc keep
// two images here: the unaligned path needs the moves without the loads, and two statements that each own the sixteen
// pairs, one per arm, were not coalesced -- 16 to 48 copies per frame.)  `sbase` must come from the scalar unit, as the frame
// loop's next-frame address does (s_mul / s_add: no wait states); a base that came through v_readfirstlane right in front
// would need the s_nop 4 that GST32_S carries.
#define AFX_FO_L(d, k, nt) "global_load_dwordx2 %" #d ", %8, %9 offset:" #k nt
template <int S, bool NT>
__device__ __forceinline__ void rows_fetch_new_s(v2 (&r)[16], unsigned voff, const float *sbase) {
    static_assert(S == 2 || S == 4 || S == 8, "hop = N/8, N/4, N/2");
#define AFX_FO_NEW8 "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15])
    if constexpr (S == 2) {
        if constexpr (NT) asm volatile(AFX_FO_L(6, 0, " nt") "\n\t" AFX_FO_L(7, 512, " nt") : AFX_FO_NEW8 : "v"(voff), "s"(sbase));
        else asm volatile(AFX_FO_L(6, 0, "") "\n\t" AFX_FO_L(7, 512, "") : AFX_FO_NEW8 : "v"(voff), "s"(sbase));
    } else if constexpr (S == 4) {
        if constexpr (NT) asm volatile(AFX_FO_L(4, 0, " nt") "\n\t" AFX_FO_L(5, 512, " nt") "\n\t" AFX_FO_L(6, 1024, " nt") "\n\t" AFX_FO_L(7, 1536, " nt") : AFX_FO_NEW8 : "v"(voff), "s"(sbase));
        else asm volatile(AFX_FO_L(4, 0, "") "\n\t" AFX_FO_L(5, 512, "") "\n\t" AFX_FO_L(6, 1024, "") "\n\t" AFX_FO_L(7, 1536, "") : AFX_FO_NEW8 : "v"(voff), "s"(sbase));
    } else {
        if constexpr (NT) asm volatile(AFX_FO_L(0, 0, " nt") "\n\t" AFX_FO_L(1, 512, " nt") "\n\t" AFX_FO_L(2, 1024, " nt") "\n\t" AFX_FO_L(3, 1536, " nt") "\n\t" AFX_FO_L(4, 2048, " nt") "\n\t" AFX_FO_L(5, 2560, " nt") "\n\t" AFX_FO_L(6, 3072, " nt") "\n\t" AFX_FO_L(7, 3584, " nt") : AFX_FO_NEW8 : "v"(voff), "s"(sbase));
        else asm volatile(AFX_FO_L(0, 0, "") "\n\t" AFX_FO_L(1, 512, "") "\n\t" AFX_FO_L(2, 1024, "") "\n\t" AFX_FO_L(3, 1536, "") "\n\t" AFX_FO_L(4, 2048, "") "\n\t" AFX_FO_L(5, 2560, "") "\n\t" AFX_FO_L(6, 3072, "") "\n\t" AFX_FO_L(7, 3584, "") : AFX_FO_NEW8 : "v"(voff), "s"(sbase));
    }
#undef AFX_FO_NEW8
}
#undef AFX_FO_L

// ---- max(x, 1e-8) in front of the cepstrum blocks' log10 as ONE v_max_f32 per value.  fmaxf compiles to two: v_max_f32 x, x
// (canonicalise: a signalling NaN becomes quiet) and the maximum itself.  Row values are results of this library's own
// arithmetic (band sums, powf), and the hardware never produces a signalling NaN: a NaN row value is quiet, and of a quiet
// NaN and a number v_max_f32 returns the number in IEEE mode -- 1e-8 with the canonicalising instruction in front and
// without it.  Every other value is unchanged by the canonicalisation (denormals are kept in f32 mode), so the results are
// the same bits for every value a row can hold.  0x322bcc77 = 1e-8f.
__device__ __forceinline__ fo_v4 max4_floor(fo_v4 x) {
    fo_v4 r;
    asm("v_max_f32 %0, 0x322bcc77, %4\n\tv_max_f32 %1, 0x322bcc77, %5\n\tv_max_f32 %2, 0x322bcc77, %6\n\tv_max_f32 %3, 0x322bcc77, %7"
        : "=&v"(r.x), "=&v"(r.y), "=&v"(r.z), "=&v"(r.w) : "v"(x.x), "v"(x.y), "v"(x.z), "v"(x.w));
    return r;
}
__device__ __forceinline__ float max_floor(float x) {
    float r;
    asm("v_max_f32 %0, 0x322bcc77, %1" : "=v"(r) : "v"(x));
    return r;
}

// ---- s_waitcnt vmcnt(0) that the wave-uniform integer z (a zero) passes through: every address that has z added to it is
// formed behind the wait (plain address arithmetic is otherwise free to move above an asm statement, "memory" or not).  An
// integer, not the pointer: a pointer that comes out of an asm statement has lost its address space, and its loads become
// flat_load, which counts on lgkmcnt as well -- under the hand-counted LDS waits of the frame loops
#define VM_WAIT_ALL_AT(z) asm volatile("s_waitcnt vmcnt(0)" : "+s"(z) : : "memory")

// ---- four 16-byte loads from ONE wave-uniform base (scalar register pair) + per-lane byte offset + immediates, served by the
// L2 like LOAD_SC1_B128 (rows another lane of the wave stored a moment ago); waited for by hand.  The s_nop covers "VALU
// writes SGPR -> VMEM reads that SGPR" (a base that came through v_readfirstlane), as in GST32_S.
#ifdef AFX_CC_PLAINLOAD  // (measurement, profiles/r06_ab_headline.txt (b))
#define AFX_FO_SC1 ""
#else
#define AFX_FO_SC1 " sc1"
#endif
#define GLD128X4_L2_S(d0, d1, d2, d3, voff, sbase, o0, o1, o2, o3)                                                          \
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %4, %5 offset:%6" AFX_FO_SC1 "\n\tglobal_load_dwordx4 %1, %4, %5 offset:%7" AFX_FO_SC1 \
                 "\n\tglobal_load_dwordx4 %2, %4, %5 offset:%8" AFX_FO_SC1 "\n\tglobal_load_dwordx4 %3, %4, %5 offset:%9" AFX_FO_SC1        \
                 : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)                                                              \
                 : "v"(voff), "s"(sbase), "n"(o0), "n"(o1), "n"(o2), "n"(o3)                                               \
                 : "memory")
#endif  // AFX_EMU_HIP_RUNTIME_H

#endif /* AFX_FRAMEOPS_H */
