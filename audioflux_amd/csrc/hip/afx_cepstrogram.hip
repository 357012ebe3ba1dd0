// afx_cepstrogram.hip -- cepstrogram kernel ("K8" of SURVEY.md 2b): per frame
//   S = FFT_N(x w) ;  L = ln(max(|S|^2, 1e-16)) over ALL N bins
//   c = Re(IFFT_N(L))                               -> out1 = c[0..N/2]
//   envelope = Re(FFT_N(low-quefrency lifter of c)) -> out2
//   detail   = Re(FFT_N(high-quefrency part of c))  -> out3
// following __cepstrogramObj_spectrogram, src/cepstrogram_algorithm.c:127-298
// (log :219-229, iFFT :232-234, envelope :249-266, details :275-288).
//
// One workgroup per frame; the whole chain lives in LDS (two N-point complex
// buffers), so HBM sees 4*hop bytes in and 3*4*(N/2+1) bytes out per frame instead
// of the reference's ten [T,N] scratch matrices.  Three FFTs instead of four: the
// two real lifter inputs ride one complex transform as l + i d and are separated
// with the conjugate-symmetry identities (exact, no evenness assumption).
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_wavefft2048.h"
#include "afx_wavefft_small.h"

namespace {

// the in-place DIF transform in LDS (afx_ldsfft.h) leaves X[k] at bitrev_r(k)
__device__ __forceinline__ int brev(int k, int r) { return (int)(__brev((unsigned)k) >> (32 - r)); }

__global__ void k_cepstrogram(AfxCepstrogramArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int r = a.radix2Exp, N = 1 << r, F = N / 2 + 1;
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    float2 *t = s + afx_lds_padded_size(N);  // both buffers use skewed addressing (afx_ldsfft.h)
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);
    const int tid = threadIdx.x, nth = blockDim.x;
    const long long frame = blockIdx.x;

    // 1. spectrum of the windowed frame (or the cached spectrum: cepstrogram2)
    if (a.x) {
        const float *x = a.framesPerClip > 0
                             ? a.x + (frame / a.framesPerClip) * a.clipStride +
                                   (frame % a.framesPerClip) * (long long)a.hop
                             : a.x + frame * (long long)a.hop;
        for (int i = tid; i < N; i += nth) s[afx_lds_pad(i)] = make_float2(x[i] * a.window[i], 0.f);
        __syncthreads();
        afx_lds_fft_dif_t<true>(s, r, tw, 1, tid, nth);
        for (int k = tid; k < N; k += nth) {
            const float2 c = s[afx_lds_pad(brev(k, r))];
            if (a.specRe) {
                a.specRe[frame * N + k] = c.x;
                a.specIm[frame * N + k] = c.y;
            }
            float p = c.x * c.x + c.y * c.y;
            if (p < 1e-16f) p = 1e-16f;
            t[afx_lds_pad(k)] = make_float2(logf(p), 0.f);
        }
    } else {
        for (int k = tid; k < N; k += nth) {
            const float re = a.specRe[frame * N + k], im = a.specIm[frame * N + k];
            float p = re * re + im * im;
            if (p < 1e-16f) p = 1e-16f;
            t[afx_lds_pad(k)] = make_float2(logf(p), 0.f);
        }
    }
    __syncthreads();

    // 2. real cepstrum: IFFT(L) = conj(FFT(conj L))/N; L is real, only the real part is kept
    afx_lds_fft_dif_t<true>(t, r, tw, 1, tid, nth);
    const float invN = 1.f / (float)N;
    const int q = a.cepNum;
    for (int n = tid; n < N; n += nth) {
        const float y = t[afx_lds_pad(brev(n, r))].x * invN;
        if (a.out1 && n < F) a.out1[frame * F + n] = y;
        // lifters (cepstrogram_algorithm.c:258-263, :282-283)
        float l = 0.f, d = 0.f;
        if (n <= q) l = y;
        if (n >= q + 1 && n <= N - q) d = y;
        s[afx_lds_pad(n)] = make_float2(l, d);
    }
    __syncthreads();
    // mirrored low-quefrency part: l[N-1-j] = l[j+1], j < cepNum
    for (int j = tid; j < q && j + 1 < N; j += nth) {
        const int dst = N - 1 - j;
        if (dst > q) s[afx_lds_pad(dst)].x = s[afx_lds_pad(j + 1)].x;
    }
    __syncthreads();
    if (!a.out2 && !a.out3) return;

    // 3. one complex FFT carries both real sequences: F = FFT(l) + i FFT(d)
    afx_lds_fft_dif_t<true>(s, r, tw, 1, tid, nth);
    for (int k = tid; k < F; k += nth) {
        const float2 A = s[afx_lds_pad(brev(k, r))];
        const float2 B = s[afx_lds_pad(brev((N - k) & (N - 1), r))];
        if (a.out2) a.out2[frame * F + k] = 0.5f * (A.x + B.x);  // Re FFT(l)[k]
        if (a.out3) a.out3[frame * F + k] = 0.5f * (A.y + B.y);  // Re FFT(d)[k]
    }
}

// ---- N = 512 .. 4096: one wave per frame, wave-level real transforms ------------------------
// Every sequence of the chain is real, so each transform is built from the complex wave transform of
// afx_wavefft2048.h / afx_wavefft_small.h (registers + LDS exchanges, no workgroup barrier) instead of
// an N-point complex radix-2 transform in LDS with a barrier per stage pair:
//   S = rfft(x w)                    -> L[k] = ln max(|S[k]|^2, 1e-16), k <= N/2
//   L is real and even (L[N - k] = L[k]), so IFFT(L) = FFT(L) / N is real and even:
//   c = Re rfft(L_even) / N          -> out1 = c[0..N/2]
//   l, d = the two lifter sequences of c (cepstrogram_algorithm.c:258-263, :282-283; c[m] for
//          m > N/2 is c[N - m]: the reference's own value there differs by rounding only)
//   out2 = Re rfft(l), out3 = Re rfft(d)
// For cepNum <= DIRECT_Q (the wrapper's default is 4) the lifter transforms are evaluated in
// closed form instead: l = c on {0..q} and mirrored onto {N-q..N-1}, d = c on {q+1..N-q}, so
//   out2[k] = c[0] + 2 sum_{m=1..q} c[m] cos(2 pi k m / N)
//   out3[k] = L[k] - out2[k] + c[q] cos(2 pi k q / N)      (index N-q is in both sequences;
//                                                            q = 0: out3 = L - c[0])
// with cos(m theta_k) by rotating W_N^k (an error of ~m ulp; q <= 16) -- two transforms per frame.
// Only n_fft 2048 has the lifter transforms as well; elsewhere a larger cepNum takes the size-generic kernel.
// Between the transforms the spectrum / cepstrum goes through an (N/2 + 1)-float natural-order
// row in the wave's exchange buffer.  HBM per frame: 4 hop in (frames overlap in L2), 12 (N/2 + 1) out.
// N = 4096 splits every transform into the 2048-point real transforms E, O of the even / odd
// samples: X[k] = E[k] + W_4096^k O[k], X[2048 - k] = conj(E[k] - W_4096^k O[k]).
// N = 1024 and 512 (round 6): the size-generic kernel ran these at 0.08-0.09 of the HBM roofline.
// Which bin a register of a transform holds is the business of the slot views beside the transforms (afxw::Bins,
// afxw::Bins4096, afxws::Bins<NJ>); the steps below are written once over a view.
// (waves per workgroup 4 / 8 / 12, lifter batches of 10 / 20 bins and the fast logarithm were measured as
// compile-time variants in round 1: profiles/r01_cepstrogram_wave.txt)
constexpr int CW = 8;     // waves per workgroup, N = 2048 (the tables are shared)
constexpr int CW4 = 8;    // N = 4096
constexpr int CWS = 8;    // N = 1024, 512
constexpr int LNB = 20;   // bins per batch of the closed-form lifters (divides 20)
constexpr int DIRECT_Q = 16;       // largest cepNum of the closed-form lifters

struct CepWArgs {
    const float *x;
    long long clipStride, totalFrames;
    int framesPerClip, hop, framesPerWave, aligned, cepNum;
    const float *win;    // [N]
    const float2 *tab;   // the transform's tables (afxw: tw1 | tw2 | tw3 ( | W_4096^k, k <= 1024, for N = 4096))
    float *out1, *out2, *out3;
};

__device__ __forceinline__ float log_power(v2 z) {
    float p = z.x * z.x + z.y * z.y;
    if (p < 1e-16f) p = 1e-16f;  // cepstrogram_algorithm.c:219-229
    return logf(p);
}

// closed-form lifter outputs of NB bins: w[i] = W_N^k of the bin, Lk[i] its log power;
// c = the cepstrum row in LDS (c[0..q] are read, the same address in every lane)
template <int NB>
__device__ __forceinline__ void lifters_direct(const float *c, int q, const v2 (&w)[NB], const float (&Lk)[NB],
                                               float (&env)[NB], float (&det)[NB]) {
    v2 z[NB];
    float acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        z[i] = v2{1.f, 0.f};
        acc[i] = 0.f;
    }
    for (int m = 1; m <= q; ++m) {
        const float cm = c[m];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            z[i] = cmul(z[i], w[i]);  // W_N^(k m): real part cos(2 pi k m / N)
            acc[i] = fmaf(cm, z[i].x, acc[i]);
        }
    }
    const float c0 = c[0], cq = q >= 1 ? c[q] : 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        env[i] = c0 + 2.f * acc[i];
        det[i] = Lk[i] - env[i] + cq * z[i].x;
    }
}

// LDS of a workgroup of W waves: the window (N floats) | TAB_F2 float2 of twiddle tables (TAB_LOAD of them loaded) | W exchange
// images of EX_F2 float2, the head of each doubling as the wave's natural-order row between transforms (N/2 + 1 floats)
template <int N, int W, int TAB_F2, int EX_F2, int TAB_LOAD = TAB_F2>
struct CepWave {
    v2 *tabWin, *tabTw, *ex;
    float *row;
    int lane;
    long long f, fEnd;  // this wave's frames

    // tables into the LDS (all waves); false: no frame left for this wave
    __device__ __forceinline__ bool begin(unsigned char *smem, const CepWArgs &a) {
        tabWin = reinterpret_cast<v2 *>(smem);
        tabTw = tabWin + N / 2;
        lane = threadIdx.x & 63;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: frame counters and row pointers stay scalar)
        ex = tabTw + TAB_F2 + wave * EX_F2;
        row = reinterpret_cast<float *>(ex);
        const float2 *win2 = reinterpret_cast<const float2 *>(a.win);
        for (int i = threadIdx.x; i < N / 2; i += W * 64) tabWin[i] = v2{win2[i].x, win2[i].y};
        for (int i = threadIdx.x; i < TAB_LOAD; i += W * 64) tabTw[i] = v2{a.tab[i].x, a.tab[i].y};
        __syncthreads();
        const long long gw = (long long)blockIdx.x * W + wave;
        f = gw * a.framesPerWave, fEnd = f + a.framesPerWave;
        if (fEnd > a.totalFrames) fEnd = a.totalFrames;
        return f < fEnd;
    }
};

__device__ __forceinline__ const float *frame_ptr(const CepWArgs &a, long long fr) {
    return a.framesPerClip > 0 ? a.x + (fr / a.framesPerClip) * a.clipStride + (fr % a.framesPerClip) * (long long)a.hop
                               : a.x + fr * (long long)a.hop;
}

// a frame into registers, V (float2 / float4) per lane and load: raw[r] = samples VW (64 r + lane) ..; vector loads where every
// frame start is aligned to them
template <typename V, int NR>
__device__ __forceinline__ void fetch(V (&raw)[NR], const float *px, int aligned, int lane) {
    constexpr int VW = sizeof(V) / sizeof(float);
    if (aligned) {
        const V *p = reinterpret_cast<const V *>(px);
#pragma unroll
        for (int r = 0; r < NR; ++r) raw[r] = p[64 * r + lane];
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int c = 0; c < VW; ++c) raw[r][c] = px[VW * (64 * r + lane) + c];
    }
}

// One value per bin slot of layout V -> a natural-order row (in the LDS, or of an output).  Every copy a lane holds is stored, in
// slot order: of the bins lane 0 holds twice (afxw::Bins: equal up to rounding) the later store wins, as it always has.
template <class V>
__device__ __forceinline__ void scatter(float *dst, int lane, const float (&val)[V::SLOTS]) {
#pragma unroll
    for (int slot = 0; slot < V::SLOTS; ++slot)
        if (V::held(slot, lane)) dst[V::bin(slot, lane)] = val[slot];
}

// 3'. closed-form lifter outputs of every bin of layout V, at most LNB slots at a time (register pressure); twiddle(slot) = W_N^bin.
// DROP: one slot lane 0 does not store -- see cepstrogram_wave.
template <class V, int DROP = -1, typename Tw>
__device__ __forceinline__ void lifter_outputs(const float *row, int q, int lane, const float (&Lk)[V::SLOTS], float *o2, float *o3, Tw twiddle) {
    constexpr int NB = V::SLOTS < LNB ? V::SLOTS : LNB;
    static_assert(V::SLOTS % NB == 0, "whole batches");
#pragma unroll
    for (int b0 = 0; b0 < V::SLOTS; b0 += NB) {
        v2 w[NB];
        float lk[NB], env[NB], det[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            w[i] = twiddle(b0 + i);
            lk[i] = Lk[b0 + i];
        }
        lifters_direct<NB>(row, q, w, lk, env, det);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int slot = b0 + i;
            if (V::held(slot, lane) && !(slot == DROP && lane == 0)) {
                if (o2) o2[V::bin(slot, lane)] = env[i];
                if (o3) o3[V::bin(slot, lane)] = det[i];
            }
        }
    }
}

// the 2048-point transform in the shape of afxws::Fft1k / Fft512
struct Fft2k {
    static constexpr int N = 2048, M = 1024, NR = 16, TAB_F2 = afxw::TAB_F2, EX_F2 = afxw::EX_F2;
    typedef afxw::Bins B;
    static __device__ __forceinline__ const v2 *tw3_of(const v2 *tab) { return tab + afxw::TAB_TW1_F2 + afxw::TAB_TW2_F2; }
    static __device__ __forceinline__ void rfft(v2 (&v)[16], v2 *ex, const v2 *tab, int lane, B &o) {
        const afxw::Tables tb = {tab, tab + afxw::TAB_TW1_F2, tw3_of(tab)};
        afxw::rfft2048(v, ex, tb, lane, o);
    }
};

// ---- N = 2048, 1024, 512: one transform per step.  X: Fft2k, afxws::Fft1k, afxws::Fft512.
// DROP: at 2048 the closed-form lifter outputs were stored all x[s][..], then all y[s][..], which left bin 768 of lane 0 to
// y[0][1]; pair by pair x[0][3] (slot 6) would come later, so lane 0 leaves it out there.  (Rows and transform outputs were stored
// pair by pair from the start and take every copy.)  The two copies agree to rounding; the choice only keeps the output bits.
template <class X, int W, int DROP>
__device__ __forceinline__ void cepstrogram_wave(unsigned char *smem, const CepWArgs &a) {
    typedef typename X::B V;
    constexpr int N = X::N, M = X::M, F = M + 1, NR = X::NR, NB = V::SLOTS;
    CepWave<N, W, X::TAB_F2, X::EX_F2> cw;
    if (!cw.begin(smem, a)) return;
    const int lane = cw.lane;
    v2 *ex = cw.ex;
    const v2 *tabWin = cw.tabWin, *tabTw = cw.tabTw;
    float *row = cw.row;
    const v2 *tw3 = X::tw3_of(tabTw);  // 0.5 W_N^k, k <= N/4 at least
    const int q = a.cepNum;
    const float invN = 1.f / (float)N;
    const long long fEnd = cw.fEnd;
    v2 raw[NR];
    fetch(raw, frame_ptr(a, cw.f), a.aligned, lane);
    for (long long f = cw.f; f < fEnd; ++f) {
        v2 v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = raw[r] * tabWin[64 * r + lane];
        if (f + 1 < fEnd) fetch(raw, frame_ptr(a, f + 1), a.aligned, lane);  // in flight under the transforms
        V b;
        // 1. spectrum -> log power (kept in registers for the closed-form details) -> row
        X::rfft(v, ex, tabTw, lane, b);
        float Lk[NB];
        b.for_each([&](int slot, v2 S) { Lk[slot] = log_power(S); });
        scatter<V>(row, lane, Lk);
        wave_lds_order();
        // 2. real cepstrum: rfft of the even extension L[m] = L[N - m]
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int m = 2 * (64 * r + lane);
            v[r] = v2{row[m <= M ? m : N - m], row[m + 1 <= M ? m + 1 : N - m - 1]};
        }
        wave_lds_order();
        X::rfft(v, ex, tabTw, lane, b);
        float ck[NB];
        b.for_each([&](int slot, v2 C) { ck[slot] = C.x * invN; });
        if (a.out1) scatter<V>(a.out1 + f * F, lane, ck);
        if (!a.out2 && !a.out3) continue;
        scatter<V>(row, lane, ck);
        wave_lds_order();
        if (N != 2048 || q <= DIRECT_Q) {
            // 3'. W_N^k = 2 tw3[k], W_N^(M - k) = -conj(W_N^k)
            lifter_outputs<V, DROP>(row, q, lane, Lk, a.out2 ? a.out2 + f * F : nullptr, a.out3 ? a.out3 + f * F : nullptr, [&](int slot) {
                const v2 t = tw3[V::position(slot, lane)] * 2.f;
                return V::mirrored(slot) ? v2{-t.x, t.y} : t;
            });
            wave_lds_order();  // the row is read; the next frame's transform may overwrite it
            continue;
        }
        if constexpr (N == 2048) {
            // 3. lifters: l keeps c[0..q] and its mirror l[N-1-j] = c[j+1], j < q (:258-263);
            //    d keeps c[q+1 .. N-q] (:282-283)
            v2 vd[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int m = 2 * (64 * r + lane);
                const float c0 = row[m <= M ? m : N - m], c1 = row[m + 1 <= M ? m + 1 : N - m - 1];
                const bool l0 = m <= q || m >= N - q, l1 = m + 1 <= q || m + 1 >= N - q;
                const bool d0 = m >= q + 1 && m <= N - q, d1 = m + 1 >= q + 1 && m + 1 <= N - q;
                v[r] = v2{l0 ? c0 : 0.f, l1 ? c1 : 0.f};
                vd[r] = v2{d0 ? c0 : 0.f, d1 ? c1 : 0.f};
            }
            wave_lds_order();
            if (a.out2) {
                X::rfft(v, ex, tabTw, lane, b);
                b.for_each([&](int slot, v2 C) { ck[slot] = C.x; });
                scatter<V>(a.out2 + f * F, lane, ck);
            }
            if (a.out3) {
                X::rfft(vd, ex, tabTw, lane, b);
                b.for_each([&](int slot, v2 C) { ck[slot] = C.x; });
                scatter<V>(a.out3 + f * F, lane, ck);
            }
        }
    }
}

__global__ __launch_bounds__(CW * 64) void k_cepstrogram_w2048(CepWArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cepstrogram_wave<Fft2k, CW, 6>(smem_raw, a);
}

template <class X>
__global__ __launch_bounds__(CWS * 64) void k_cepstrogram_wsmall(CepWArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cepstrogram_wave<X, CWS, -1>(smem_raw, a);
}

// ---- N = 4096: two transforms per step, combined (afxw::combine4096); closed-form lifters only
__global__ __launch_bounds__(CW4 * 64) void k_cepstrogram_w4096(CepWArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int N = 4096, F = 2049;
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef afxw::Bins4096 V;
    CepWave<N, CW4, afxw::TAB_F2 + afxw::W4_PAD_F2, afxw::EX_F2, afxw::TAB_F2 + afxw::W4_F2> cw;
    if (!cw.begin(smem_raw, a)) return;
    const int lane = cw.lane;
    v2 *ex = cw.ex;
    float *row = cw.row;
    const v4 *tabWin = reinterpret_cast<const v4 *>(cw.tabWin);  // [1024] window quads
    const v2 *tabTw = cw.tabTw, *tabW4 = tabTw + afxw::TAB_F2;    // W_4096^k, k <= 1024
    const afxw::Tables tb = {tabTw, tabTw + afxw::TAB_TW1_F2, tabTw + afxw::TAB_TW1_F2 + afxw::TAB_TW2_F2};
    const int q = a.cepNum;
    const long long fEnd = cw.fEnd;
    for (long long f = cw.f; f < fEnd; ++f) {
        v2 ve[16], vo[16];
        {
            // even / odd samples of the windowed frame: lane holds x[4n .. 4n+3], n = 64 n1 + lane
            v4 raw[16];
            fetch(raw, frame_ptr(a, f), a.aligned, lane);
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                const v4 xv = raw[n1], wv = tabWin[64 * n1 + lane];
                ve[n1] = v2{xv.x * wv.x, xv.z * wv.z};
                vo[n1] = v2{xv.y * wv.y, xv.w * wv.w};
            }
        }
        afxw::Bins be, bo;
        // 1. spectrum -> log power (kept in registers for the closed-form details) -> row
        afxw::rfft2048(ve, ex, tb, lane, be);
        afxw::rfft2048(vo, ex, tb, lane, bo);
        float Lk[V::SLOTS];
        V::for_each(be, bo, tabW4, lane, [&](int slot, v2 S) { Lk[slot] = log_power(S); });
        scatter<V>(row, lane, Lk);
        wave_lds_order();
        // 2. real cepstrum: transform of the even extension L[m] = L[4096 - m]
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            const int m = 4 * (64 * n1 + lane);
            auto ext = [&](int i) { return row[i <= 2048 ? i : N - i]; };
            ve[n1] = v2{ext(m), ext(m + 2)};
            vo[n1] = v2{ext(m + 1), ext(m + 3)};
        }
        wave_lds_order();
        afxw::rfft2048(ve, ex, tb, lane, be);
        afxw::rfft2048(vo, ex, tb, lane, bo);
        const float invN = 1.f / (float)N;
        float ck[V::SLOTS];
        V::for_each(be, bo, tabW4, lane, [&](int slot, v2 C) { ck[slot] = C.x * invN; });
        // only c[0 .. q] is read back (by every lane): bins 0 .. 16 live in lanes 0 .. 16, slot 0
        if (lane <= DIRECT_Q) row[lane] = ck[0];
        if (a.out1) scatter<V>(a.out1 + f * F, lane, ck);
        wave_lds_order();
        if (!a.out2 && !a.out3) continue;
        // 3'. W_4096^k per slot: k', 2048 - k' -> -conj, 1024 -+ k' from the table
        lifter_outputs<V>(row, q, lane, Lk, a.out2 ? a.out2 + f * F : nullptr, a.out3 ? a.out3 + f * F : nullptr, [&](int slot) {
            const int kp = V::position(slot, lane), r = slot & 3;
            const v2 wk = tabW4[kp], wp = tabW4[1024 - kp];
            // W^(2048 - k') = -conj(W^k'),  W^(1024 + k') = -conj(W^(1024 - k'))
            return r == 0 ? wk : r == 1 ? v2{-wk.x, wk.y} : r == 2 ? wp : v2{-wp.x, wp.y};
        });
        wave_lds_order();  // the row is read; the next frame's transform may overwrite it
    }
}

}  // namespace

// host: twiddle tables of the wave kernels, tab[AFX_CEPSTROGRAM_FASTTAB_FLOATS]; N = 4096 appends
// W_4096^k, k <= 1024 (in double, rounded once)
extern "C" void afxk_cepstrogram_fast_tables(float *tab, int fftLength) {
    if (fftLength == 1024) {
        afxws::Fft1k::fill_tables(tab);
        return;
    }
    if (fftLength == 512) {
        afxws::Fft512::fill_tables(tab);
        return;
    }
    afxw::fill_tables(tab);
    if (fftLength == 4096) {
        const double PI = 3.14159265358979323846;
        float *w4 = tab + 2 * afxw::TAB_F2;
        for (int k = 0; k < afxw::W4_F2; ++k) {
            w4[2 * k] = (float)cos(-2.0 * PI * (double)k / 4096.0);
            w4[2 * k + 1] = (float)sin(-2.0 * PI * (double)k / 4096.0);
        }
    }
}

namespace {

struct CepSize {  // one row per wave kernel: LDS = CepWave's layout
    void (*kernel)(CepWArgs);
    const char *name;
    int N, waves, tabF2, exF2;
    int loadMask;  // a lane's vector load is loadMask + 1 floats
};
const CepSize CEP_512 = {k_cepstrogram_wsmall<afxws::Fft512>, "k_cepstrogram_wsmall", 512, CWS, afxws::Fft512::TAB_F2, afxws::Fft512::EX_F2, 1};
const CepSize CEP_1024 = {k_cepstrogram_wsmall<afxws::Fft1k>, "k_cepstrogram_wsmall", 1024, CWS, afxws::Fft1k::TAB_F2, afxws::Fft1k::EX_F2, 1};
const CepSize CEP_2048 = {k_cepstrogram_w2048, "k_cepstrogram_w2048", 2048, CW, afxw::TAB_F2, afxw::EX_F2, 1};
const CepSize CEP_4096 = {k_cepstrogram_w4096, "k_cepstrogram_w4096", 4096, CW4, afxw::TAB_F2 + afxw::W4_PAD_F2, afxw::EX_F2, 3};

int launch_cepstrogram_wave(const CepSize &z, const AfxCepstrogramArgs *a, void *stream) {
    CepWArgs w;
    w.x = a->x;
    w.clipStride = a->clipStride;
    w.totalFrames = a->timeLength;
    w.framesPerClip = a->framesPerClip;
    w.hop = a->hop;
    // vector loads (float2 / float4 per lane) need every frame start aligned to them
    const int am = z.loadMask;
    w.aligned = ((reinterpret_cast<size_t>(a->x) & (size_t)(4 * am + 3)) == 0 && (a->hop & am) == 0 &&
                 (a->framesPerClip <= 0 || (a->clipStride & am) == 0))
                    ? 1
                    : 0;
    w.cepNum = a->cepNum;
    w.win = a->window;
    w.tab = reinterpret_cast<const float2 *>(a->fastTab);
    w.out1 = a->out1;
    w.out2 = a->out2;
    w.out3 = a->out3;
    // enough waves for ~4 workgroups per CU, at most 16 frames per wave
    long long fpw = w.totalFrames / (256LL * z.waves * 4);
    w.framesPerWave = fpw < 1 ? 1 : (fpw > 16 ? 16 : (int)fpw);
    const long long waves = (w.totalFrames + w.framesPerWave - 1) / w.framesPerWave;
    const long long blocks = (waves + z.waves - 1) / z.waves;
    const size_t lds = sizeof(float) * z.N + sizeof(float2) * (size_t)(z.tabF2 + z.waves * z.exF2);
    AFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(z.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(z.kernel, dim3((unsigned)blocks), dim3(z.waves * 64), lds, (hipStream_t)stream, w);
    AFX_LAUNCH_CHECK(z.name);
    return AFX_OK;
}

}  // namespace

extern "C" int afxk_cepstrogram(const AfxCepstrogramArgs *a, void *stream) {
    if (a->radix2Exp < 1 || a->radix2Exp > 13) {
        afxdev_set_error("cepstrogram: fftLength 2^%d is outside the supported 2..8192", a->radix2Exp);
        return AFX_ERR_UNSUPPORTED;
    }
    if (a->timeLength <= 0) return AFX_OK;
    const int N = 1 << a->radix2Exp;
    const bool wave2k = N == 2048 && 2 * a->cepNum + 2 < N, wave4k = N == 4096 && a->cepNum <= DIRECT_Q;
    const bool waveS = (N == 1024 || N == 512) && a->cepNum <= DIRECT_Q;
    if ((wave2k || wave4k || waveS) && a->x && !a->specRe && a->fastTab && !afxdev_no_fused())
        return launch_cepstrogram_wave(N == 512 ? CEP_512 : N == 1024 ? CEP_1024 : wave2k ? CEP_2048 : CEP_4096, a, stream);
    int threads = N / 2;
    if (threads < 64) threads = 64;
    if (threads > 512) threads = 512;
    const size_t lds = (size_t)2 * afx_lds_padded_size(N) * sizeof(float2);
    if (lds > 48 * 1024) {
        AFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cepstrogram),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    // one workgroup per frame; HIP rejects 2^32 or more threads in one dimension: beyond that, several launches of
    // whole clips (or, for one long clip, of whole frames)
    const long long maxFrames = ((1LL << 32) - 1) / threads;
    if (a->timeLength > maxFrames) {
        const long long F = N / 2 + 1;
        long long per = maxFrames;
        if (a->framesPerClip > 0) {
            if (a->framesPerClip > maxFrames) {
                afxdev_set_error("cepstrogram: %d frames per clip in one launch", a->framesPerClip);
                return AFX_ERR_UNSUPPORTED;
            }
            per = maxFrames / a->framesPerClip * a->framesPerClip;
        }
        for (long long f0 = 0; f0 < a->timeLength; f0 += per) {
            AfxCepstrogramArgs s = *a;
            s.timeLength = (int)(a->timeLength - f0 < per ? a->timeLength - f0 : per);
            if (a->x) s.x = a->x + (a->framesPerClip > 0 ? f0 / a->framesPerClip * a->clipStride : f0 * a->hop);
            if (a->specRe) s.specRe = a->specRe + f0 * N;
            if (a->specIm) s.specIm = a->specIm + f0 * N;
            if (a->out1) s.out1 = a->out1 + f0 * F;
            if (a->out2) s.out2 = a->out2 + f0 * F;
            if (a->out3) s.out3 = a->out3 + f0 * F;
            hipLaunchKernelGGL(k_cepstrogram, dim3((unsigned)s.timeLength), dim3(threads), lds, (hipStream_t)stream, s);
            AFX_LAUNCH_CHECK("k_cepstrogram");
        }
        return AFX_OK;
    }
    hipLaunchKernelGGL(k_cepstrogram, dim3((unsigned)a->timeLength), dim3(threads), lds,
                       (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_cepstrogram");
    return AFX_OK;
}
