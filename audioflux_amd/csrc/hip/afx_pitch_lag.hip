// afx_pitch_lag.hip -- the lag-domain pitch trackers (include/mir/_pitch_ncf.h, include/mir/_pitch_cep.h), one launch from
// samples to (fre, value[, curve]).  NCF and the cepstrum are the same computation apart from one function of the spectrum.
//
// One workgroup per frame; frames carry no state from one to the next (_pitch_ncf.c:437-466, _pitch_cep.c:430-446).  With
// N = fftLength and L = 2N = 2^R, one transform buffer of L complex points in LDS (afx_ldsfft.h) serves all of:
//   1. z[n] = x[n] w[n], n < N, zeros up to L (written, not loaded); one L-point transform, X[k] at s[bitrev(k)];
//   2. the mid-stage in place: P[k] = |X[k]|^2 (NCF) or logf(|X[k]|^2) (CEP), and with it the move back to natural order --
//      the positions (i, bitrev(i)) swap, each pair owned by one thread, so no second buffer and no barrier in between;
//   3. P is real and even, so its inverse transform is the forward one over L: r[n] = Re F[n] / L, F[n] at s[bitrev(n)];
//   4. the curve, k = 0 ... maxIndex:
//        NCF  r'[n] = r[n] / sqrt(L), c[k] = r'[k + 1] / sqrt(r'[0]) for minIndex - 1 <= k <= maxIndex - 1, 0 elsewhere
//             (the float32 operation order of _pitch_ncf.c:454-465; r'[0] comes out of the transform itself);
//        CEP  c[k] = r[k];
//   5. first argmax of c over minIndex ... maxIndex (afx_pitchparts.h), fre = samplate / (index + 1).
// A frame without a usable curve -- NCF: r'[0] is not positive (silence); CEP: one of the L power bins is exactly 0, found
// with one OR over the workgroup -- has NaN in every computed entry and the index minIndex, as __vmax gives for a row that
// starts with a NaN (flux_vector.c:1536).
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_pitchparts.h"

namespace {

template <int R>
using LagCfg = AfxPitchLagCfg<R>;  // afx_pitchparts.h: shared with afx_harmonic_ratio.hip

template <int R, int MODE>
__global__ void __launch_bounds__(LagCfg<R>::NT) k_pitch_lag(AfxPitchLagArgs a) {
    using C = LagCfg<R>;
    constexpr int L = C::L, N = L / 2, NT = C::NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *red = reinterpret_cast<float *>(smem_raw);            // [32]: cross-wave exchange of the reduction
    int *flag = reinterpret_cast<int *>(smem_raw + 128);         // CEP: a power bin of exactly 0
    float2 *s = reinterpret_cast<float2 *>(smem_raw + 256);      // transform buffer of L points, afx_lds_pad addressing
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);  // W_L^m, m < L / 2
    const int minIndex = a.minIndex, maxIndex = a.maxIndex;
    const long long row = blockIdx.x;
    int b, t;
    const float *x = afx_pitch_row(a.x, row, a.timeLength, a.clipStride, a.hop, b, t);

    // 1. the windowed frame and its zero padding (neighbouring frames overlap: re-read through L2)
    for (int j = tid; j < N; j += NT) {
        float v = x[j];
        if (a.window) v *= a.window[j];
        s[afx_lds_pad(j)] = make_float2(v, 0.f);
        s[afx_lds_pad(j + N)] = make_float2(0.f, 0.f);
    }
    if (MODE == AFX_PITCH_LAG_CEP && tid == 0) *flag = 0;
    __syncthreads();
    afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);  // X[k] at s[bitrev(k)]

    // 2. |X|^2 or its log, back in natural order: the pair (i, bitrev(i)) belongs to the thread that holds the smaller one
    bool zero = false;
    for (int i = tid; i < L; i += NT) {
        const int j = (int)(__brev((unsigned)i) >> (32 - R));
        if (i <= j) {
            const float2 u = s[afx_lds_pad(i)], v = s[afx_lds_pad(j)];  // X[j], X[i]
            float pu = u.x * u.x + u.y * u.y, pv = v.x * v.x + v.y * v.y;
            if (MODE == AFX_PITCH_LAG_CEP) {
                zero = zero || pu == 0.f || pv == 0.f;
                pu = logf(pu);
                pv = logf(pv);
            }
            s[afx_lds_pad(i)] = make_float2(pv, 0.f);
            s[afx_lds_pad(j)] = make_float2(pu, 0.f);
        }
    }
    if (MODE == AFX_PITCH_LAG_CEP && zero) *flag = 1;  // (every writer stores the same value)
    __syncthreads();
    bool bad = MODE == AFX_PITCH_LAG_CEP && *flag != 0;

    // 3. the inverse of the real, even sequence as a forward transform: L r[n] = Re s[bitrev(n)]
    afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);

    // 4. the curve 0 ... maxIndex, the thread's first maximum from minIndex on
    const float invL = 1.f / (float)L;
    float inv = 1.f, invSqrtL = 1.f;
    if (MODE == AFX_PITCH_LAG_NCF) {
        invSqrtL = (float)(1.0 / sqrtf((float)L));
        const float r0 = s[afx_lds_pad(0)].x * invL * invSqrtL;
        inv = (float)(1.0 / sqrtf(r0));
        bad = !(r0 > 0.f);
    }
    const float nan = __builtin_nanf("");
    float bv = -__builtin_huge_valf();
    int bi = AFX_PITCH_NONE;
    for (int k = tid; k <= maxIndex; k += NT) {
        float c;
        if (MODE == AFX_PITCH_LAG_NCF) {
            c = 0.f;
            if (k >= minIndex - 1 && k < maxIndex)  // k + 1 <= maxIndex <= N - 1
                c = bad ? nan : s[afx_lds_pad((int)(__brev((unsigned)(k + 1)) >> (32 - R)))].x * invL * invSqrtL * inv;
        } else {
            c = bad ? nan : s[afx_lds_pad((int)(__brev((unsigned)k) >> (32 - R)))].x * invL;  // k <= maxIndex <= L - 1
        }
        if (a.curve) a.curve[row * (maxIndex + 1) + k] = c;
        AFX_PITCH_CANDIDATE(bv, bi, c, k, minIndex)
    }

    // 5. over the workgroup: the larger value, the smaller index among equal ones
    AFX_PITCH_ARGMAX(NT, bv, bi, red, tid, lane, wave)
    if (tid == 0) {
        if (bad || bi == AFX_PITCH_NONE) {  // the row starts with a NaN: it wins
            bi = minIndex;
            bv = nan;
        }
        const long long at = (long long)b * a.outStride + t;
        if (a.fre) a.fre[at] = (float)((double)a.samplate / (double)(bi + 1));  // 1.0 * samplate / (index + 1)
        if (a.value) a.value[at] = bv;
    }
}

template <int R, int MODE>
int launch(const AfxPitchLagArgs &a, long long rows, void *stream) {
    using C = LagCfg<R>;
    AFX_LAUNCH_DYN_LDS((k_pitch_lag<R, MODE>), dim3((unsigned)rows), dim3(C::NT), (size_t)afx_pitch_lag_lds_bytes(R - 1), stream, a);
    AFX_LAUNCH_CHECK("k_pitch_lag");
    return AFX_OK;
}

template <int MODE>
int dispatch(const AfxPitchLagArgs &a, long long rows, void *stream) {
    switch (a.radix2Exp) {
        case 6: return launch<7, MODE>(a, rows, stream);
        case 7: return launch<8, MODE>(a, rows, stream);
        case 8: return launch<9, MODE>(a, rows, stream);
        case 9: return launch<10, MODE>(a, rows, stream);
        case 10: return launch<11, MODE>(a, rows, stream);
        case 11: return launch<12, MODE>(a, rows, stream);
        default: return launch<13, MODE>(a, rows, stream);
    }
}

}  // namespace

extern "C" int afxk_pitch_lag(const AfxPitchLagArgs *a, void *stream) {
    if (!a || !a->x || !a->twiddle || a->batch <= 0 || a->timeLength <= 0 || a->hop <= 0) return AFX_ERR_ARG;
    if (a->mode != AFX_PITCH_LAG_NCF && a->mode != AFX_PITCH_LAG_CEP) return AFX_ERR_ARG;
    if (a->radix2Exp < AFX_PITCH_LAG_MIN_EXP || a->radix2Exp > AFX_PITCH_LAG_MAX_EXP) return AFX_ERR_UNSUPPORTED;
    const int N = 1 << a->radix2Exp;
    // the limits the kernel's indexing rests on
    const int ncf = a->mode == AFX_PITCH_LAG_NCF;
    if (a->minIndex < (ncf ? 1 : 0) || a->maxIndex < a->minIndex || a->maxIndex > (ncf ? N - 1 : 2 * N - 1)) return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    if (a->clipStride < a->dataLength && a->batch > 1) return AFX_ERR_ARG;
    if ((a->fre || a->value) && a->outStride < a->timeLength) return AFX_ERR_ARG;
    if (!a->fre && !a->value && !a->curve) return AFX_OK;
    const long long rows = (long long)a->batch * a->timeLength;
    if (rows > 0x7fffffffLL) {
        afxdev_set_error("pitch: %lld frames in one launch", rows);
        return AFX_ERR_UNSUPPORTED;
    }
    return a->mode == AFX_PITCH_LAG_NCF ? dispatch<AFX_PITCH_LAG_NCF>(*a, rows, stream) : dispatch<AFX_PITCH_LAG_CEP>(*a, rows, stream);
}
