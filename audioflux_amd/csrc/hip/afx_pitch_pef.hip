// afx_pitch_pef.hip -- pitch-estimation-filter tracking (include/mir/_pitch_pef.h), one launch from samples to
// (fre, value[, curve]).
//
// Workgroups stride over the (clip, frame) rows; frames carry no state from one to the next (_pitch_pef.c:308-327,
// :376-381, :419-425).  With N = fftLength, one transform buffer of 2N complex points in LDS (afx_ldsfft.h) serves all of:
//   1. z[n] = xw[2n] + i xw[2n + 1], n < N / 2, zeros up to N: the windowed frame zero-padded to 2N real points, packed;
//      one N-point complex transform; the real split X[k] = Ze + W_2N^k Zo gives pw[k] = |X[k]|^2, k = 0 ... N, into LDS;
//   2. the log spectrum B[P + m] = y[m] bw[m], m < 2N, zeros elsewhere up to 4N, y[m] the reference's interpolation
//      expression on operands the host precomputed (AfxPitchPefTap), written PACKED (B[2q] + i B[2q + 1]) over the buffer;
//   3. one 2N-point complex transform and, in one pass over the pairs (k, 2N - k), k = 0 ... N: the real split to the
//      4N-point spectrum of B, the product with filterSpec = conj(spectrum of h) / 2N, and the packing of the result for
//      the inverse.  The pass reads bit-reversed and writes in natural order, so the values wait in registers across one
//      barrier;
//   4. the inverse as a FORWARD transform read at the mirrored index: r[n] = F[(2N - n) mod 2N], r[n] = R[2n] + i R[2n + 1].
//      Lags k <= maxIndex < 2N and taps n < N reach B[n + k], n + k < 3N: nothing wraps at 4N points;
//   5. first argmax of R over minIndex ... maxIndex (afx_pitchparts.h): a row of zeros comes out as minIndex;
//   6. fre = lg[index].
#include <hip/hip_runtime.h>

#include <afx_asm.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_pitchparts.h"

namespace {

template <int R>
struct PefCfg {
    static constexpr int N = 1 << R;
    // threads: one radix-4 butterfly each per pass of the 2N-point transform, at most 1024.  One workgroup holds up to 84 KB
    // of LDS (72 KB with the default band at N = 4096), so at the large sizes a CU runs one or two of them: the waves that hide LDS and barrier latency have to come
    // from inside the workgroup (the HPS finding, profiles/pitch_hs_mi355x.txt)
    static constexpr int NT = N / 2 < 64 ? 64 : (N / 2 > 1024 ? 1024 : N / 2);
    static constexpr int PAIRS = N / NT + 1;  // pairs (k, 2N - k), k = 0 ... N, per thread
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <int R>
__global__ void __launch_bounds__(PefCfg<R>::NT) k_pitch_pef(AfxPitchPefArgs a, long long rows) {
    using C = PefCfg<R>;
    constexpr int N = C::N, NT = C::NT, PAIRS = C::PAIRS, N2 = 2 * N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *red = reinterpret_cast<float *>(smem_raw);        // [32]: cross-wave exchange of the reduction
    float2 *s = reinterpret_cast<float2 *>(smem_raw + 128);  // transform buffer of 2N points, afx_lds_pad addressing
    float *pw = reinterpret_cast<float *>(s + afx_lds_padded_size(N2));  // [pwLength]: the bins the log grid reads
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);  // W_4N^m, m < 2N
    const float2 *G = reinterpret_cast<const float2 *>(a.filterSpec);
    const int minIndex = a.minIndex, maxIndex = a.maxIndex, P = a.filterPadNum, pwLength = a.pwLength;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        // the thread index is opaque per row: otherwise every LDS address and twiddle address of the 17 ... 20 unrolled
        // transform passes below is hoisted out of this loop as an invariant -- 128 VGPRs and spills at N = 2048 / 4096
        // against 49 / 58 with the addresses recomputed per pass
        int tid = threadIdx.x;
        PIN(tid);
        int b, t;
        const float *x = afx_pitch_row(a.x, row, a.timeLength, a.clipStride, a.hop, b, t);

        // 1. the windowed frame, packed and zero-padded (neighbouring frames overlap: re-read through L2)
        for (int q = tid; q < N; q += NT) {
            float2 v = make_float2(0.f, 0.f);
            if (q < N / 2) v = make_float2(x[2 * q] * a.window[2 * q], x[2 * q + 1] * a.window[2 * q + 1]);
            s[afx_lds_pad(q)] = v;
        }
        __syncthreads();
        afx_lds_fft_dif_t<true>(s, R, tw, 4, tid, NT);  // Z[k] at s[bitrev_R(k)]
        for (int k = tid; k <= N / 2; k += NT) {
            const int kp = (N - k) & (N - 1);
            const float2 zk = s[afx_lds_pad((int)(__brev((unsigned)k) >> (32 - R)))];
            const float2 zp = s[afx_lds_pad((int)(__brev((unsigned)kp) >> (32 - R)))];
            const float2 ze = make_float2(0.5f * (zk.x + zp.x), 0.5f * (zk.y - zp.y));
            const float2 zo = make_float2(0.5f * (zk.y + zp.y), -0.5f * (zk.x - zp.x));
            const float2 tt = cmul(tw[2 * k], zo);  // W_2N^k
            const float2 xa = make_float2(ze.x + tt.x, ze.y + tt.y), xb = make_float2(ze.x - tt.x, ze.y - tt.y);
            if (k < pwLength) pw[k] = xa.x * xa.x + xa.y * xa.y;
            if (N - k < pwLength) pw[N - k] = xb.x * xb.x + xb.y * xb.y;
        }
        __syncthreads();

        // 2. the weighted log spectrum behind P zeros, packed over the whole buffer
        for (int q = tid; q < N2; q += NT) {
            float v[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int m = 2 * q + c - P;
                v[c] = 0.f;
                if (m >= 0 && m < N2) {
                    const float4 tap = reinterpret_cast<const float4 *>(a.taps)[m];  // (index, dx, dl, bw): one 16-byte load
                    const int j = __float_as_int(tap.x);
                    float y;
                    if (j < 0) {
                        y = pw[N];  // (pwLength is N + 1 then)
                    } else {
                        const float y1 = pw[j], y2 = pw[j + 1];
                        y = y1 + tap.y * (y2 - y1) / tap.z;
                    }
                    v[c] = y * tap.w;
                }
            }
            s[afx_lds_pad(q)] = make_float2(v[0], v[1]);
        }
        __syncthreads();
        afx_lds_fft_dif_t<true>(s, R + 1, tw, 2, tid, NT);  // Z[k] at s[bitrev_{R+1}(k)]

        // 3. split, product with the filter's spectrum, packing: pairs (k, 2N - k)
        float2 ya[PAIRS], yb[PAIRS];
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int k = tid + NT * i;
            if (k <= N) {
                const int kp = (N2 - k) & (N2 - 1);
                const float2 zk = s[afx_lds_pad((int)(__brev((unsigned)k) >> (31 - R)))];
                const float2 zp = s[afx_lds_pad((int)(__brev((unsigned)kp) >> (31 - R)))];
                const float2 w = tw[k];  // W_4N^k
                const float2 ze = make_float2(0.5f * (zk.x + zp.x), 0.5f * (zk.y - zp.y));
                const float2 zo = make_float2(0.5f * (zk.y + zp.y), -0.5f * (zk.x - zp.x));
                const float2 tt = cmul(w, zo);
                const float2 xk = make_float2(ze.x + tt.x, ze.y + tt.y);     // X[k]
                const float2 xp = make_float2(ze.x - tt.x, -(ze.y - tt.y));  // X[2N - k]
                const float2 yk = cmul(xk, G[k]), yp = cmul(xp, G[N2 - k]);
                const float2 ye = make_float2(0.5f * (yk.x + yp.x), 0.5f * (yk.y - yp.y));
                const float2 d2 = make_float2(0.5f * (yk.x - yp.x), 0.5f * (yk.y + yp.y));
                const float2 yo = cmul(d2, make_float2(w.x, -w.y));
                ya[i] = make_float2(ye.x - yo.y, ye.y + yo.x);   // Ye + i Yo
                yb[i] = make_float2(ye.x + yo.y, yo.x - ye.y);   // conj(Ye) + i conj(Yo)
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int k = tid + NT * i;
            if (k <= N) {
                const int kp = (N2 - k) & (N2 - 1);
                s[afx_lds_pad(k)] = ya[i];
                if (kp != k) s[afx_lds_pad(kp)] = yb[i];
            }
        }
        __syncthreads();
        afx_lds_fft_dif_t<true>(s, R + 1, tw, 2, tid, NT);

        // 4. the lags 0 ... maxIndex, the thread's first maximum from minIndex on
        float bv = -__builtin_huge_valf();
        int bi = AFX_PITCH_NONE;
        for (int k = tid; k <= maxIndex; k += NT) {
            const int n = (N2 - (k >> 1)) & (N2 - 1);
            const float2 r = s[afx_lds_pad((int)(__brev((unsigned)n) >> (31 - R)))];
            const float c = (k & 1) ? r.y : r.x;
            if (a.curve) a.curve[row * (maxIndex + 1) + k] = c;
            AFX_PITCH_CANDIDATE(bv, bi, c, k, minIndex)
        }

        // 5. over the workgroup: the larger value, the smaller index among equal ones
        AFX_PITCH_ARGMAX(NT, bv, bi, red, tid, lane, wave)
        if (tid == 0) {
            if (bi == AFX_PITCH_NONE) bi = minIndex;  // every candidate a NaN
            const long long at = (long long)b * a.outStride + t;
            if (a.fre) a.fre[at] = a.lg[bi];
            if (a.value) a.value[at] = bv;
        }
        __syncthreads();  // red, pw and the buffer are free for the next frame
    }
}

template <int R>
int launch(const AfxPitchPefArgs &a, long long rows, void *stream) {
    using C = PefCfg<R>;
    const long long lds = afx_pitch_pef_lds_bytes(R, a.pwLength);
    // (the limit is raised once per instantiation and device: to the largest plan of the size)
    if (const int st = afx_dyn_lds<k_pitch_pef<R>>((int)afx_pitch_pef_lds_bytes(R, C::N + 1))) return st;
    // enough workgroups to fill every CU several times over at the small sizes; they stride over the rows
    const long long cap = 256LL * 8;
    const unsigned grid = (unsigned)(rows < cap ? rows : cap);
    hipLaunchKernelGGL((k_pitch_pef<R>), dim3(grid), dim3(C::NT), (size_t)lds, (hipStream_t)stream, a, rows);
    AFX_LAUNCH_CHECK("k_pitch_pef");
    return AFX_OK;
}

}  // namespace

extern "C" int afxk_pitch_pef(const AfxPitchPefArgs *a, void *stream) {
    if (!a || !a->x || !a->window || !a->twiddle || !a->taps || !a->filterSpec || !a->lg || a->batch <= 0 || a->timeLength <= 0 ||
        a->hop <= 0)
        return AFX_ERR_ARG;
    if (a->radix2Exp < AFX_PITCH_PEF_MIN_EXP || a->radix2Exp > AFX_PITCH_PEF_MAX_EXP) return AFX_ERR_UNSUPPORTED;
    const int N = 1 << a->radix2Exp;
    // the limits the kernel's indexing rests on
    if (a->minIndex < 0 || a->maxIndex < a->minIndex || a->maxIndex >= 2 * N || a->filterPadNum < 0 || a->filterPadNum > N ||
        a->pwLength < 2 || a->pwLength > N + 1)
        return AFX_ERR_ARG;
    if (((size_t)a->taps & 15) != 0) return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    if (a->clipStride < a->dataLength && a->batch > 1) return AFX_ERR_ARG;
    if ((a->fre || a->value) && a->outStride < a->timeLength) return AFX_ERR_ARG;
    if (!a->fre && !a->value && !a->curve) return AFX_OK;
    const long long rows = (long long)a->batch * a->timeLength;
    if (rows > 0x7fffffffLL) {
        afxdev_set_error("pitch: %lld frames in one launch", rows);
        return AFX_ERR_UNSUPPORTED;
    }
    switch (a->radix2Exp) {
        case 6: return launch<6>(*a, rows, stream);
        case 7: return launch<7>(*a, rows, stream);
        case 8: return launch<8>(*a, rows, stream);
        case 9: return launch<9>(*a, rows, stream);
        case 10: return launch<10>(*a, rows, stream);
        case 11: return launch<11>(*a, rows, stream);
        default: return launch<12>(*a, rows, stream);
    }
}
