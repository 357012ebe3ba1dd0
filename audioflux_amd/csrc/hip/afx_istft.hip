// afx_istft.hip -- inverse short-time Fourier transform, the device side of stftObj_istft
// (reference: src/stft_algorithm.c:304-409).
//
//   k_istft_frames  one workgroup per frame: the fftLength complex bins of the frame (split
//                   re / im planes, as stftObj_stft stores them) are read once, transformed by the
//                   shared in-LDS FFT (inverse = conj . forward . conj, /N), and the real part
//                   times the synthesis window w^e goes to a [frames, N] scratch.
//   k_istft_ola     one thread per output sample: the <= ceil(N/hop) frames that cover the sample
//                   are GATHERED in ascending frame order -- the order the reference's
//                   scatter loop adds them in (:378-386), so the float32 sums round the same way
//                   and no atomics are needed -- together with the window-power normaliser
//                   sum w^(e+1), clamped (< 1e-6 -> 1) and divided out (:389-396).
//
// Both are HBM streaming kernels: per frame 8 N bytes in, 4 N out, then 4 N in and 4 hop out.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_wavefft2048.h"
#include "afx_wavefft_small.h"

namespace {

__global__ void k_istft_frames(AfxIstftArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *s = reinterpret_cast<float2 *>(smem_raw);
    const int r = a.radix2Exp, N = 1 << r;
    const long long frame = blockIdx.x;
    const int tid = threadIdx.x, nth = blockDim.x;
    const float *re = a.re + frame * N, *im = a.im + frame * N;
    for (int i = tid; i < N; i += nth) s[afx_lds_pad(i)] = make_float2(re[i], -im[i]);
    __syncthreads();
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);
    afx_lds_fft_dif_t<true>(s, r, tw, 1, tid, nth);
    const float invN = 1.f / (float)N;
    float *dst = a.frames + frame * N;
    for (int n = tid; n < N; n += nth) {
        const int src = (int)(__brev((unsigned)n) >> (32 - r));
        dst[n] = (s[afx_lds_pad(src)].x * invN) * a.win1[n];
    }
}

__global__ void k_istft_ola(AfxIstftArgs a) {
    const int N = 1 << a.radix2Exp, H = a.hop, T = a.timeLength;
    const long long outLen = (long long)(T - 1) * H + N;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= outLen) return;
    const int b = blockIdx.y;
    const float *frames = a.frames + (long long)b * T * N;
    float *out = a.out + (long long)b * a.outStride;
    long long iLo = j >= N ? (j - N) / H + 1 : 0;
    long long iHi = j / H;
    if (iHi > T - 1) iHi = T - 1;
    float acc = out[j], nrm = 0.f;
    for (long long i = iLo; i <= iHi; ++i) {
        const int k = (int)(j - i * H);
        acc += frames[i * N + k];
        nrm += a.win2[k];
    }
    if (nrm < 1e-6f) nrm = 1.f;
    out[j] = acc / nrm;
}

}  // namespace

// ---- n_fft 2048: one wave per frame, overlap-add in the LDS, no frame scratch (round 6) -----------------------------------
//
// The inverse transform of a frame is ONE forward real transform (afx_wavefft2048.h, the function the forward kernels run): with
// Xs = the Hermitian part of the given bins (what the real part of the reference's complex inverse keeps, stft_algorithm.c:304-409),
//     u[k] = Re Xs[k] + Im Xs[k] = (re[k] + re[N-k] + im[k] - im[N-k]) / 2      (a real sequence),   U = FFT(u):
//     x[n] = (Re U[n] + Im U[n]) / N,   x[N-n] = (Re U[n] - Im U[n]) / N,   0 <= n <= N/2
// (the cosine sums of the even part and the sine sums of the odd part, each once).  A lane holds u[2n], u[2n+1], n = 64 n1 + lane;
// the mirrored bins N - 2n - 1 are element .y of register 15 - n1 in lane 63 - lane, N - 2n element .x of register 15 - n1 in lane
// 64 - lane (lane 0: its own register 16 - n1): two cross-lane reads per plane instead of reversed loads.
// Overlap-add: a wave walks a run of consecutive frames of one clip (the ceil(N / hop) - 1 frames before its run first: their tails
// reach into it) with a ring of N floats in the LDS: a sample enters the ring with the caller's value of out[] (the reference adds
// to what is there), takes the frames in ascending order -- the order of the reference's scatter loop (:378-386) and of k_istft_ola,
// so the float32 sums round the same way -- and leaves it, divided by the window-power sum (:389-396), when frame i has been
// added to [i hop, (i + 1) hop).  Per frame 8 N bytes in and 4 hop out (+ 4 hop of out[] read): the [frames, N] scratch round trip
// (8 N bytes) and the second launch are gone.
//
// What the sizes share -- the LDS layout and its prologue, the run of frames a wave walks, the ring with its entering samples, the
// batched add, the window-power sums and the drain -- is OlaRing below.  A kernel keeps what is its own: how the frame's bins
// become u, which transform runs, and the walk over the transform's bin slots (the views of afx_wavefft2048.h / afx_wavefft_small.h
// say which bin a slot is and whether this lane owns it).
namespace {

#ifndef AFX_ISTFT_WAVES
#define AFX_ISTFT_WAVES 7
#endif
constexpr int IW = AFX_ISTFT_WAVES;  // waves per workgroup: 25 KB of tables (window w^e, twiddles) + <= 8 KB of window-power sums + 7 x 16.5 KB (exchange image + ring)
constexpr int IW4 = 4;   // n_fft 4096: 16 KB window + 25 KB twiddles + <= 16 KB window-power sums + 4 x 24.5 KB (exchange image + ring)
constexpr int ISW = 12;  // n_fft 1024 / 512 / 256 (1024: 12 x 9 KB of exchange image + ring, 11 KB of tables)

// contributions to the ring that are added together.  Every output index occurs once per frame, so the slots of a batch are
// distinct: its reads, then its writes -- written one by one the compiler must order each read behind the previous write.  The
// batch size sets how many LDS reads are in flight and how long at / val / ok live.
template <int CNT>
struct OlaBatch {
    int at[CNT];
    float val[CNT];
    bool ok[CNT];
};

// LDS of a workgroup of W waves: win1[N] | TAB_F2 float2 of twiddle tables (TAB_LOAD of them loaded) | W exchange images of EX_F2
// float2 | W rings of N floats | nrmTab[hop]
template <int N, int W, int TAB_F2, int EX_F2, int TAB_LOAD = TAB_F2>
struct OlaRing {
    float *win1;                       // [N] synthesis window w^e
    const float *__restrict__ win2;    // w^(e+1), global: read at the clip's ends only
    v2 *tabTw, *ex;                    // the transform's tables; this wave's exchange image
    float *ring, *nrmTab, *out;
    int lane, b, T, H, f0, f1, fs;     // clip, frames, hop; the run [f0, f1) and the first frame whose tail reaches into it
    long long ownLo, ownHi;            // the samples this wave stores
    int i;                             // the frame being added (at_frame)
    long long j0;                      // its first sample

    // Tables and window-power sums into the LDS (all waves), then this wave's run; false: no run left for it.  On return the ring
    // holds the samples that enter with frame fs.
    __device__ __forceinline__ bool begin(unsigned char *smem, const AfxIstftArgs &a, const float2 *__restrict__ tab, int framesPerRun, int runsPerClip) {
        win1 = reinterpret_cast<float *>(smem);
        win2 = a.win2;
        tabTw = reinterpret_cast<v2 *>(win1 + N);
        lane = threadIdx.x & 63;
        const int wave = threadIdx.x >> 6;
        ex = tabTw + TAB_F2 + wave * EX_F2;
        ring = reinterpret_cast<float *>(tabTw + TAB_F2 + W * EX_F2) + wave * N;
        // window-power sum of a sample every covering frame of which exists (N <= j, j / hop <= T - 1): a function of j mod hop, added
        // in the order of k_istft_ola's loop (ascending frames = descending window positions)
        nrmTab = ring + (W - wave) * N;  // [hop], behind the last wave's ring
        for (int k = threadIdx.x; k < N; k += W * 64) win1[k] = a.win1[k];
        for (int k = threadIdx.x; k < TAB_LOAD; k += W * 64) tabTw[k] = v2{tab[k].x, tab[k].y};
        for (int t = threadIdx.x; t < a.hop; t += W * 64) {
            float sum = 0.f;
            for (int k = t + ((N - 1 - t) / a.hop) * a.hop; k >= 0; k -= a.hop) sum += win2[k];
            nrmTab[t] = sum;
        }
        __syncthreads();

        const long long run = (long long)blockIdx.x * W + wave;
        if (run >= (long long)a.batch * runsPerClip) return false;
        b = (int)(run / runsPerClip), T = a.timeLength, H = a.hop;
        f0 = (int)(run - (long long)b * runsPerClip) * framesPerRun;
        f1 = f0 + framesPerRun < T ? f0 + framesPerRun : T;
        const int halo = (N - 1) / H;
        fs = f0 > halo ? f0 - halo : 0;
        const long long outLen = (long long)(T - 1) * H + N;
        ownLo = (long long)f0 * H, ownHi = f1 == T ? outLen : (long long)f1 * H;
        out = a.out + (long long)b * a.outStride;
        for (int t = lane; t < N; t += 64) ring[((long long)fs * H + t) & (N - 1)] = entering((long long)fs * H + t);
        return true;
    }

    // samples that enter the ring with a frame: the caller's values where this wave will store, zeros elsewhere
    __device__ __forceinline__ float entering(long long j) const { return (j >= ownLo && j < ownHi) ? out[j] : 0.f; }

    // the window-power sum of sample j (k_istft_ola's loop; interior samples: the table)
    __device__ __forceinline__ float power(long long j) const {
        if (j >= N && j / H <= T - 1) return nrmTab[(int)(j % H)];
        long long iLo = j >= N ? (j - N) / H + 1 : 0, iHi = j / H;
        if (iHi > T - 1) iHi = T - 1;
        float nrm = 0.f;
        for (long long q = iLo; q <= iHi; ++q) nrm += win2[(int)(j - q * H)];
        return nrm;
    }

    __device__ __forceinline__ void at_frame(int frame) {
        i = frame;
        j0 = (long long)frame * H;
    }

    // sample n of the frame, x / (2 N) of it windowed, as entry e of a batch.  (The 0.5 of the Hermitian part rides in the scale.)
    template <int CNT>
    __device__ __forceinline__ void put(OlaBatch<CNT> &bt, int e, bool valid, int n, float x) const {
        const float scale = 0.5f / (float)N;
        bt.ok[e] = valid;
        bt.at[e] = (int)((j0 + n) & (N - 1));
        bt.val[e] = valid ? (x * scale) * win1[n] : 0.f;
    }
    template <int CNT, int USED = CNT>
    __device__ __forceinline__ void flush(const OlaBatch<CNT> &bt) const {
        float cur[USED];
#pragma unroll
        for (int e = 0; e < USED; ++e) cur[e] = bt.ok[e] ? ring[bt.at[e]] : 0.f;
#pragma unroll
        for (int e = 0; e < USED; ++e)
            if (bt.ok[e]) ring[bt.at[e]] = cur[e] + bt.val[e];
    }
    // One bin U[bin] of the transform of u gives x[bin] = (Re U + Im U) / N and, where the bin is not its own mirror image,
    // x[N - bin] = (Re U - Im U) / N; Z is U[bin], or its conjugate as the layouts' y registers hold it.  SPF slots fill a batch,
    // which is then added.
    // Two spellings of one rule.  The compiler contracts cur + val into one fma where it can prove an entry valid and leaves
    // multiply and add where a select stays; what it proves depends on how and where the mirror's validity is written, and the last
    // bit of the output with it.  Each size keeps the spelling it was written with: decided by the caller in the layout's terms
    // (k' > 0: 2048, 1024, 512), or from the bin between the two entries (4096).
    template <int SPF>
    __device__ __forceinline__ void add_bin(OlaBatch<2 * SPF> &bt, int slot, bool owned, bool mirror, int bin, bool conjugate, v2 Z) const {
        const int e = 2 * (slot % SPF);
        put(bt, e, owned, bin, conjugate ? Z.x - Z.y : Z.x + Z.y);
        put(bt, e + 1, mirror, (N - bin) & (N - 1), conjugate ? Z.x + Z.y : Z.x - Z.y);
        if (slot % SPF == SPF - 1) flush(bt);
    }
    template <int SPF>
    __device__ __forceinline__ void add_bin(OlaBatch<2 * SPF> &bt, int slot, bool owned, int bin, v2 U) const {
        const int e = 2 * (slot % SPF);
        put(bt, e, owned, bin, U.x + U.y);
        put(bt, e + 1, owned && bin > 0 && bin < N / 2, (N - bin) & (N - 1), U.x - U.y);
        if (slot % SPF == SPF - 1) flush(bt);
    }

    // samples no later frame reaches leave the ring: [i hop, (i + 1) hop), everything to the clip's end behind its last frame.
    // SPP samples per lane at a time: their reads first, then the stores.
    template <int SPP>
    __device__ __forceinline__ void drain() const {
        wave_lds_order();
        if (i >= f0) {
            const int cnt = i == T - 1 ? N : H;
            for (int t0 = 0; t0 < cnt && t0 < N; t0 += 64 * SPP) {  // (t0 < N: one pass where a pass covers the frame)
                float acc[SPP], nrm[SPP];
#pragma unroll
                for (int u = 0; u < SPP; ++u) {
                    const int t = t0 + lane + 64 * u;
                    acc[u] = t < cnt ? ring[(j0 + t) & (N - 1)] : 0.f;
                    nrm[u] = t < cnt ? power(j0 + t) : 1.f;
                }
#pragma unroll
                for (int u = 0; u < SPP; ++u) {
                    const int t = t0 + lane + 64 * u;
                    if (t < cnt) out[j0 + t] = acc[u] / (nrm[u] < 1e-6f ? 1.f : nrm[u]);
                }
            }
        }
        wave_lds_order();
    }

    // the next frame's new samples take the slots just stored
    __device__ __forceinline__ void enter_next() const {
        if (i + 1 < f1)
            for (int t = lane; t < H; t += 64) ring[(j0 + N + t) & (N - 1)] = entering(j0 + N + t);
    }
    // ... requested a frame ahead (request_next before the transform, enter_next(nxt) behind the drain) where they fit eight
    // registers per lane: hop <= 512
    __device__ __forceinline__ void request_next(float (&nxt)[8]) const {
        if (H <= 512 && i + 1 < f1) {
#pragma unroll
            for (int t = 0; t < 8; ++t) nxt[t] = lane + 64 * t < H ? entering(j0 + N + lane + 64 * t) : 0.f;
        }
    }
    __device__ __forceinline__ void enter_next(const float (&nxt)[8]) const {
        if (H > 512) return enter_next();
        if (i + 1 < f1) {
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (lane + 64 * t < H) ring[(j0 + N + lane + 64 * t) & (N - 1)] = nxt[t];
        }
    }
};

// ---- n_fft 2048 ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IW * 64) void k_istft_w2048(AfxIstftArgs a, const float2 *__restrict__ tab, int framesPerRun, int runsPerClip) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int N = 2048;
    OlaRing<N, IW, afxw::TAB_F2, afxw::EX_F2> ola;
    if (!ola.begin(smem_raw, a, tab, framesPerRun, runsPerClip)) return;
    const afxw::Tables tb = {ola.tabTw, ola.tabTw + afxw::TAB_TW1_F2, ola.tabTw + afxw::TAB_TW1_F2 + afxw::TAB_TW2_F2};
    const int lane = ola.lane;
    const bool lane0 = lane == 0;
    // the bins of the frame about to be transformed; the next frame's are requested behind the transform, under the overlap-add
    v2 r[16], m[16];
    auto fetch = [&](int i) {
        const v2 *re2 = reinterpret_cast<const v2 *>(a.re + ((long long)ola.b * ola.T + i) * N);
        const v2 *im2 = reinterpret_cast<const v2 *>(a.im + ((long long)ola.b * ola.T + i) * N);
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            r[n1] = re2[64 * n1 + lane];
            m[n1] = im2[64 * n1 + lane];
        }
    };
    fetch(ola.fs);

    for (int i = ola.fs; i < ola.f1; ++i) {
        ola.at_frame(i);
        float nxt[8];
        ola.request_next(nxt);
        // the frame's bins -> u
        v2 v[16];
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            // mirrors: .y from lane 63 - lane, .x from lane 64 - lane (lane 0: own register 16 - n1, bin N = bin 0 for n1 = 0)
            const float ry = __shfl(r[15 - n1].y, 63 - lane, 64), my = __shfl(m[15 - n1].y, 63 - lane, 64);
            float rx = __shfl(r[15 - n1].x, (64 - lane) & 63, 64), mx = __shfl(m[15 - n1].x, (64 - lane) & 63, 64);
            if (lane0) {
                rx = r[n1 == 0 ? 0 : 16 - n1].x;
                mx = m[n1 == 0 ? 0 : 16 - n1].x;
            }
            v[n1] = v2{(r[n1].x + rx) + (m[n1].x - mx), (r[n1].y + ry) + (m[n1].y - my)};
        }
        afxw::Bins bn;
        afxw::rfft2048(v, ola.ex, tb, lane, bn);
        if (i + 1 < ola.f1) fetch(i + 1);  // (behind the transform: in flight across it the 64 registers spill)
        // batches of 16, 16 and 8 contributions: the slots of s = 0, of s = 1, the base-128 extras
        OlaBatch<16> bt;
        typedef afxw::Bins V;
        bn.for_each([&](int slot, v2 Z) {
            const bool owned = V::owned(slot, lane);
            ola.add_bin<8>(bt, slot, owned, owned && V::paired(slot, lane), V::bin(slot, lane), V::mirrored(slot), Z);
        });
        ola.flush<16, 8>(bt);
        ola.drain<8>();
        ola.enter_next(nxt);
    }
}

// ---- n_fft 4096 (the reference wrapper's default): the same scheme; U = the real transform of the 4096 values u[k] from the wave
// transforms of its even and odd samples (afxw::combine4096, as the forward kernels do).  A lane holds u[4n .. 4n + 3], n = 64 n1 + lane:
// the mirrors 4096 - 4n - c are element 0 of quad 1024 - n (lane 64 - lane; lane 0: its own register 16 - n1) for c = 0 and
// elements 3, 2, 1 of quad 1023 - n (lane 63 - lane, register 15 - n1) for c = 1, 2, 3.
__global__ __launch_bounds__(IW4 * 64) void k_istft_w4096(AfxIstftArgs a, const float2 *__restrict__ tab, int framesPerRun, int runsPerClip) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef afxw::Bins4096 V;
    constexpr int N = 4096;
    OlaRing<N, IW4, afxw::TAB_F2 + afxw::W4_PAD_F2, afxw::EX_F2, afxw::TAB_F2 + afxw::W4_F2> ola;
    if (!ola.begin(smem_raw, a, tab, framesPerRun, runsPerClip)) return;
    const afxw::Tables tb = {ola.tabTw, ola.tabTw + afxw::TAB_TW1_F2, ola.tabTw + afxw::TAB_TW1_F2 + afxw::TAB_TW2_F2};
    const v2 *tabW4 = ola.tabTw + afxw::TAB_F2;
    const int lane = ola.lane;
    const bool lane0 = lane == 0;

    for (int i = ola.fs; i < ola.f1; ++i) {
        ola.at_frame(i);
        afxw::Bins be, bo;
        {
            // the frame's bins -> u: even samples (u[4n], u[4n + 2]) and odd samples (u[4n + 1], u[4n + 3]) of every quad
            const v4 *re4 = reinterpret_cast<const v4 *>(a.re + ((long long)ola.b * ola.T + i) * N);
            const v4 *im4 = reinterpret_cast<const v4 *>(a.im + ((long long)ola.b * ola.T + i) * N);
            v4 r[16], m[16];
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                r[n1] = re4[64 * n1 + lane];
                m[n1] = im4[64 * n1 + lane];
            }
            v2 ve[16], vo[16];
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                const v4 rq = r[15 - n1], mq = m[15 - n1];
                float r0 = __shfl(rq.x, (64 - lane) & 63, 64), m0 = __shfl(mq.x, (64 - lane) & 63, 64);
                if (lane0) {
                    r0 = r[n1 == 0 ? 0 : 16 - n1].x;
                    m0 = m[n1 == 0 ? 0 : 16 - n1].x;
                }
                const float r1 = __shfl(rq.w, 63 - lane, 64), m1 = __shfl(mq.w, 63 - lane, 64);
                const float r2 = __shfl(rq.z, 63 - lane, 64), m2 = __shfl(mq.z, 63 - lane, 64);
                const float r3 = __shfl(rq.y, 63 - lane, 64), m3 = __shfl(mq.y, 63 - lane, 64);
                ve[n1] = v2{(r[n1].x + r0) + (m[n1].x - m0), (r[n1].z + r2) + (m[n1].z - m2)};
                vo[n1] = v2{(r[n1].y + r1) + (m[n1].y - m1), (r[n1].w + r3) + (m[n1].w - m3)};
            }
            afxw::rfft2048(ve, ola.ex, tb, lane, be);
            afxw::rfft2048(vo, ola.ex, tb, lane, bo);
        }
        // 16 contributions every 8 slots, from inside the combination
        OlaBatch<16> bt;
        V::for_each(be, bo, tabW4, lane, [&](int slot, v2 U) { ola.add_bin<8>(bt, slot, V::owned(slot, lane), V::bin(slot, lane), U); });
        ola.drain<8>();
        ola.enter_next();
    }
}

// ---- n_fft 1024 / 512: the same scheme on the wave transforms of afx_wavefft_small.h (8 x 8 x 8 in eight registers, 4 x 4 x 4 x 4
// in four).  Their bins come out once each: k = lane + 64 j < N / 4 with its partner N / 2 - k, N / 4 in every lane.
template <class F>
__global__ __launch_bounds__(ISW * 64) void k_istft_wsmall(AfxIstftArgs a, const float2 *__restrict__ tab, int framesPerRun, int runsPerClip) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    typedef typename F::B V;
    constexpr int N = F::N, NR = F::NR;
    OlaRing<N, ISW, F::TAB_F2, F::EX_F2> ola;
    if (!ola.begin(smem_raw, a, tab, framesPerRun, runsPerClip)) return;
    const int lane = ola.lane;
    const bool lane0 = lane == 0;
    v2 r[NR], m[NR];
    auto fetch = [&](int i) {
        const v2 *re2 = reinterpret_cast<const v2 *>(a.re + ((long long)ola.b * ola.T + i) * N);
        const v2 *im2 = reinterpret_cast<const v2 *>(a.im + ((long long)ola.b * ola.T + i) * N);
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            r[q] = re2[64 * q + lane];
            m[q] = im2[64 * q + lane];
        }
    };
    fetch(ola.fs);
    for (int i = ola.fs; i < ola.f1; ++i) {
        ola.at_frame(i);
        v2 v[NR];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const float ry = __shfl(r[NR - 1 - q].y, 63 - lane, 64), my = __shfl(m[NR - 1 - q].y, 63 - lane, 64);
            float rx = __shfl(r[NR - 1 - q].x, (64 - lane) & 63, 64), mx = __shfl(m[NR - 1 - q].x, (64 - lane) & 63, 64);
            if (lane0) {
                rx = r[q == 0 ? 0 : NR - q].x;
                mx = m[q == 0 ? 0 : NR - q].x;
            }
            v[q] = v2{(r[q].x + rx) + (m[q].x - mx), (r[q].y + ry) + (m[q].y - my)};
        }
        if (i + 1 < ola.f1) fetch(i + 1);
        V bn;
        F::rfft(v, ola.ex, ola.tabTw, lane, bn);
        OlaBatch<2 * V::SLOTS> bt;  // one batch per frame
        bn.for_each([&](int slot, v2 Z) {
            const bool owned = V::owned(slot, lane);
            ola.template add_bin<V::SLOTS>(bt, slot, owned, owned && V::paired(slot, lane), V::bin(slot, lane), V::mirrored(slot), Z);
        });
        ola.template drain<4>();
        ola.enter_next();
    }
}

// ---- n_fft 256: TWO frames per 256-point complex wave transform (the inverse of afx_stft256.hip's trick).  With As, Bs the Hermitian
// parts of the bins of two consecutive frames a, b:  x_a + i x_b = IFFT(As + i Bs) = conj(FFT(conj(As + i Bs))) / N, and
// conj(As + i Bs)[k] = (Re As - Im Bs, -Im As - Re Bs).  The transform's natural-order output gives sample n = lane + 64 q of both frames
// in one lane: frame a is added to the ring, then frame b one hop further -- ascending frames, as everywhere.
__global__ __launch_bounds__(ISW * 64) void k_istft_w256(AfxIstftArgs a, const float2 *__restrict__ tab, int framesPerRun, int runsPerClip) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    typedef afxws::Fft512 F;
    constexpr int N = 256;
    OlaRing<N, ISW, F::TAB_F2, F::EX_F2> ola;
    if (!ola.begin(smem_raw, a, tab, framesPerRun, runsPerClip)) return;
    const int lane = ola.lane, b = ola.b, T = ola.T;
    const bool lane0 = lane == 0;
    // one frame's samples (x[q] = sample lane + 64 q) into the ring, its finished samples out, the next frame's new samples in
    auto overlap_add = [&](int i, const float (&x)[4]) {
        ola.at_frame(i);
        OlaBatch<4> bt;
#pragma unroll
        for (int q = 0; q < 4; ++q) ola.put(bt, q, true, lane + 64 * q, x[q]);
        ola.flush(bt);
        ola.drain<4>();
        ola.enter_next();
        wave_lds_order();
    };

    for (int i = ola.fs; i < ola.f1; i += 2) {
        const int ib = i + 1 < ola.f1 ? i + 1 : i;  // an odd run: the last frame rides twice, added once
        const float *ra = a.re + ((long long)b * T + i) * N, *ia = a.im + ((long long)b * T + i) * N;
        const float *rb = a.re + ((long long)b * T + ib) * N, *ib_ = a.im + ((long long)b * T + ib) * N;
        float are[4], aim[4], bre[4], bim[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            are[r] = ra[64 * r + lane];
            aim[r] = ia[64 * r + lane];
            bre[r] = rb[64 * r + lane];
            bim[r] = ib_[64 * r + lane];
        }
        v2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // bin N - k, k = 64 r + lane: register 3 - r of lane 64 - lane (lane 0: its own register 4 - r; r = 0: bin 0 itself)
            const int src = (64 - lane) & 63;
            float mar = __shfl(are[3 - r], src, 64), mai = __shfl(aim[3 - r], src, 64);
            float mbr = __shfl(bre[3 - r], src, 64), mbi = __shfl(bim[3 - r], src, 64);
            if (lane0) {
                mar = are[r == 0 ? 0 : 4 - r];
                mai = aim[r == 0 ? 0 : 4 - r];
                mbr = bre[r == 0 ? 0 : 4 - r];
                mbi = bim[r == 0 ? 0 : 4 - r];
            }
            const float asr = are[r] + mar, asi = aim[r] - mai, bsr = bre[r] + mbr, bsi = bim[r] - mbi;  // 2 x the Hermitian parts
            v[r] = v2{asr - bsi, -asi - bsr};
        }
        F::cfft(v, ola.ex, ola.tabTw, lane);
        __builtin_amdgcn_s_setprio(0);
        wave_lds_order();  // (the natural-order image in `ex` is not needed: the lanes' registers hold their samples)
        float xa[4], xb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xa[q] = v[q].x;
            xb[q] = -v[q].y;
        }
        overlap_add(i, xa);
        if (ib != i) overlap_add(ib, xb);
    }
}

// Frames per run.  A wave walks one run (+ `halo` frames before it) and every wave slot of the device takes one run per round, so a launch
// costs rounds x (frames per run + halo) frame times: the cheapest (rounds, run length) pair with all runs placed -- 64 clips of 938 frames
// on 1792 slots as 1920 runs of 32 is two rounds of 35 frame times, as 1792 runs of 34 one round of 37.  Runs never shorter than `least`.
int frames_per_run(int batch, int T, long long slots, int halo, int least) {
    long long best = T, bestCost = -1;
    for (int rounds = 1; rounds <= 8; ++rounds) {
        const long long perClip = slots * rounds / batch;  // runs a clip may take
        if (perClip < 1) continue;
        long long fpr = (T + perClip - 1) / perClip;
        if (fpr < least) fpr = least;
        if (fpr > T) fpr = T;
        const long long runs = (long long)batch * ((T + fpr - 1) / fpr);
        const long long cost = ((runs + slots - 1) / slots) * (fpr + halo);
        if (bestCost < 0 || cost < bestCost) {
            bestCost = cost;
            best = fpr;
        }
    }
    return (int)best;
}

// workgroups of `waves` waves and `lds` bytes a CU holds at a time (160 KB of LDS, 32 waves)
int resident_groups(size_t lds, int waves) {
    long long g = lds ? (long long)(163840 / lds) : 1;
    if (g > 32 / waves) g = 32 / waves;
    return g < 1 ? 1 : (int)g;
}

}  // namespace

extern "C" const void *afxk_wave_tables(void);  // afx_stft.hip: the afxw tables + the W_4096^k tail

namespace {

// twiddle tables of the small wave transforms, one device copy per device and size (never freed)
template <class F>
const float2 *small_tables() {
    return reinterpret_cast<const float2 *>(afx_device_table<F::fill_tables>(sizeof(float) * 2 * F::TAB_F2));
}
const float2 *wave_tables() { return static_cast<const float2 *>(afxk_wave_tables()); }

// One row per n_fft of the one-launch inverse.  The sizes were written one by one (round 6) and differ in more than their
// geometry; every difference is kept as it was and stands here as a field, to be read side by side.
struct IstftSize {
    void (*kernel)(AfxIstftArgs, const float2 *, int, int);
    const char *name;
    int N, waves;            // frame length; waves per workgroup
    int tabF2, exF2;         // float2 of twiddle tables in the LDS; of one wave's exchange image
    const float2 *(*tables)();
    unsigned align;          // bytes the re / im planes must be aligned to (the lanes' vector loads)
    bool residentGroups;     // the wave slots that place the runs count the workgroups a CU holds at a time (else one per CU)
    int least;               // shortest run of frames
    bool ldsLimit;           // the hop's window-power sums can push the LDS past 160 KB: then not this kernel's case
    bool dynLdsAttribute;    // raise the kernel's dynamic-LDS limit before the launch
};
const IstftSize ISTFT_256 = {k_istft_w256, "k_istft_w256", 256, ISW, afxws::Fft512::TAB_F2, afxws::Fft512::EX_F2, small_tables<afxws::Fft512>,
                             8, true, 32, false, false};
const IstftSize ISTFT_512 = {k_istft_wsmall<afxws::Fft512>, "k_istft_wsmall", 512, ISW, afxws::Fft512::TAB_F2, afxws::Fft512::EX_F2,
                             small_tables<afxws::Fft512>, 8, true, 16, false, true};
const IstftSize ISTFT_1024 = {k_istft_wsmall<afxws::Fft1k>, "k_istft_wsmall", 1024, ISW, afxws::Fft1k::TAB_F2, afxws::Fft1k::EX_F2,
                              small_tables<afxws::Fft1k>, 8, true, 16, false, true};
const IstftSize ISTFT_2048 = {k_istft_w2048, "k_istft_w2048", 2048, IW, afxw::TAB_F2, afxw::EX_F2, wave_tables, 8, false, 16, false, true};
const IstftSize ISTFT_4096 = {k_istft_w4096, "k_istft_w4096", 4096, IW4, afxw::TAB_F2 + afxw::W4_PAD_F2, afxw::EX_F2, wave_tables,
                              16, false, 16, true, true};  // (hops beyond ~3000 miss the LDS limit: the size-generic launches)

// CU count -> LDS bytes (OlaRing's layout) -> frames per run -> grid -> attribute -> launch
int launch_istft(const IstftSize &z, const AfxIstftArgs *a, void *stream) {
    if ((reinterpret_cast<uintptr_t>(a->re) | reinterpret_cast<uintptr_t>(a->im)) & (z.align - 1)) return AFX_ERR_UNSUPPORTED;
    const float2 *tab = z.tables();
    if (!tab) return AFX_ERR_UNSUPPORTED;
    const size_t lds = sizeof(float) * z.N + sizeof(float2) * (size_t)(z.tabF2 + z.waves * z.exF2) + sizeof(float) * z.N * z.waves +
                       sizeof(float) * (size_t)a->hop;
    if (z.ldsLimit && lds > 160 * 1024) return AFX_ERR_UNSUPPORTED;
    const long long slots = (long long)afx_cu_count() * z.waves * (z.residentGroups ? resident_groups(lds, z.waves) : 1);
    const long long fpr = frames_per_run(a->batch, a->timeLength, slots, (z.N - 1) / a->hop, z.least);
    const long long runsPerClip = (a->timeLength + fpr - 1) / fpr, runs = runsPerClip * a->batch;
    const long long blocks = (runs + z.waves - 1) / z.waves;
    if (blocks > 0x7fffffffLL) return AFX_ERR_UNSUPPORTED;
    if (z.dynLdsAttribute)
        AFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(z.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(z.kernel, dim3((unsigned)blocks), dim3(z.waves * 64), lds, (hipStream_t)stream, *a, tab, (int)fpr, (int)runsPerClip);
    AFX_LAUNCH_CHECK(z.name);
    return AFX_OK;
}

}  // namespace

// AFX_ERR_UNSUPPORTED: not this kernel's case (afxk_istft then runs the two size-generic launches, which need a->frames)
extern "C" int afxk_istft_fused(const AfxIstftArgs *a, void *stream) {
    if (a->hop < 1 || a->hop > (1 << a->radix2Exp) || a->timeLength < 1) return AFX_ERR_UNSUPPORTED;
    switch (a->radix2Exp) {
        case 8: return launch_istft(ISTFT_256, a, stream);
        case 9: return launch_istft(ISTFT_512, a, stream);
        case 10: return launch_istft(ISTFT_1024, a, stream);
        case 11: return launch_istft(ISTFT_2048, a, stream);
        case 12: return launch_istft(ISTFT_4096, a, stream);
        default: return AFX_ERR_UNSUPPORTED;
    }
}

extern "C" int afxk_istft(const AfxIstftArgs *a, void *stream) {
    if (!a->frames) {
        afxdev_set_error("istft: the size-generic kernels need the frame scratch");
        return AFX_ERR_ARG;
    }
    if (a->radix2Exp < 1 || a->radix2Exp > 14) {
        afxdev_set_error("istft: fftLength 2^%d is outside the supported 2..16384", a->radix2Exp);
        return AFX_ERR_UNSUPPORTED;
    }
    const long long frames = (long long)a->batch * a->timeLength;
    if (frames <= 0) return AFX_OK;
    // k_istft_frames: one workgroup of <= 256 threads per frame (HIP rejects 2^32 or more threads in one dimension);
    // k_istft_ola: one grid row per clip (65 535).  Larger batches go out as several launches of whole clips.
    const long long maxFrames = ((1LL << 32) - 1) / 256;
    if ((frames > maxFrames || a->batch > 65535) && a->batch > 1 && a->timeLength <= maxFrames) {
        long long clipsPer = maxFrames / a->timeLength;
        if (clipsPer > 65535) clipsPer = 65535;
        const long long rowFloats = 1LL << a->radix2Exp;
        for (long long b0 = 0; b0 < a->batch; b0 += clipsPer) {
            AfxIstftArgs s = *a;
            const long long row0 = b0 * a->timeLength;
            s.batch = (int)(a->batch - b0 < clipsPer ? a->batch - b0 : clipsPer);
            s.re = a->re + row0 * rowFloats;
            s.im = a->im + row0 * rowFloats;
            s.frames = a->frames + row0 * rowFloats;
            s.out = a->out + b0 * a->outStride;
            const int st = afxk_istft(&s, stream);
            if (st != AFX_OK) return st;
        }
        return AFX_OK;
    }
    if (frames > 0x7fffffffLL || a->batch > 65535) {
        afxdev_set_error("istft: %lld frames / %d clips in one launch", frames, a->batch);
        return AFX_ERR_UNSUPPORTED;
    }
    const int N = 1 << a->radix2Exp;
    int threads = N / 4;
    if (threads < 64) threads = 64;
    if (threads > 256) threads = 256;
    const size_t lds = (size_t)afx_lds_padded_size(N) * sizeof(float2);
    if (lds > 48 * 1024) {
        AFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_istft_frames),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL(k_istft_frames, dim3((unsigned)frames), dim3(threads), lds, (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_istft_frames");
    const long long outLen = (long long)(a->timeLength - 1) * a->hop + N;
    const long long blocks = (outLen + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        afxdev_set_error("istft: %lld output samples per clip", outLen);
        return AFX_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(k_istft_ola, dim3((unsigned)blocks, (unsigned)a->batch), dim3(256), 0,
                       (hipStream_t)stream, *a);
    AFX_LAUNCH_CHECK("k_istft_ola");
    return AFX_OK;
}
