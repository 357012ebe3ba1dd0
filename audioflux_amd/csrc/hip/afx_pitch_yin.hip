// afx_pitch_yin.hip -- YIN pitch tracking (include/mir/_pitch_yin.h), one launch from samples to (fre, trough, min).
//
// One workgroup per frame; frames carry no state from one to the next (_pitch_yin.c:352-427).  Per frame, in LDS and registers:
//   1. z[n] = x[n] + i 2^g y[n], y[n] = x[autoLength - n] for n <= autoLength, else 0: ONE complex transform gives the spectra
//      of the frame and of its reversed prefix, X = (Z[k] + conj Z[N-k]) / 2, Y = (Z[k] - conj Z[N-k]) / 2i; both are real, and
//      2^g (from the two energies, undone exactly at the end) brings them to the same scale;
//   2. P = X Y is Hermitian, so the inverse is real: c = Re FFT(conj P) / N, and c[autoLength + j] is the correlation term
//      r[j] = sum_{m <= autoLength} x[m] x[m + j] -- autoLength + 1 products (_pitch_yin.c:358-360);
//   3. energy term e[j] = E[autoLength + j] - E[j] from the inclusive prefix sum E of x^2 (autoLength squares starting one
//      sample later, :383-405); both terms snapped to 0 below 1e-6; d[j] = e[0] + e[j] - 2 r[j];
//   4. yin[k] = d[L] / ((d[1] + ... + d[L]) / L + 1e-16), L = minIndex + k (:414-448);
//   5. first trough below thresh (a min over lags of the lanes' first hits), its parabolic offset (:462-503), min of the
//      curve, optionally all qualifying troughs in lag order and the curve itself.
// The two prefix sums are scans (lane-local runs, a wave scan, one pass over the waves) accumulated in double; the reference
// adds serially in float32, so the low-order bits differ -- tests/pitch_check.py states what is accepted.
// Thread t owns the 2^r / threads consecutive samples / lags from t * PER on (scans, epilogue) and strides over the
// transform; the blocked views of LDS are skewed by one float per 16 so that the lanes of a wave hit different banks.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_hipcheck.h"
#include "afx_ldsfft.h"
#include "afx_pitchparts.h"

namespace {

template <int R>
struct YinCfg {
    static constexpr int N = 1 << R;
    static constexpr int NT = N / 16 < 64 ? 64 : (N / 16 > 512 ? 512 : N / 16);  // threads: 16 points each from 1024 on
    static constexpr int PER = N / NT;                                            // 1 ... 16
    static constexpr int NP = (N / 2 + NT - 1) / NT;                              // spectrum pairs (k, N - k) per thread
    static constexpr int XE = N + (N >> 4) + 1;                                   // floats of the skewed sample / curve array
    static constexpr size_t LDS = sizeof(double) * 16 + sizeof(float2) * afx_lds_padded_size(N) + sizeof(float) * XE;
};

__device__ __forceinline__ int yin_skew(int j) { return j + (j >> 4); }

__device__ __forceinline__ double yin_shfl_up(double v, int d) {
    int w[2];
    __builtin_memcpy(w, &v, 8);
    w[0] = __shfl_up(w[0], d);
    w[1] = __shfl_up(w[1], d);
    __builtin_memcpy(&v, w, 8);
    return v;
}

// exclusive prefix of v over the workgroup's threads in thread order; every thread calls it.  red: 8 doubles of LDS, free
// again on return
template <int NT>
__device__ __forceinline__ double yin_scan(double v, double *red, int lane, int wave, double *total) {
    double inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double u = yin_shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    double off = 0.0, all = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const double r = red[w];
        if (w < wave) off += r;
        all += r;
    }
    __syncthreads();
    if (total) *total = all;
    return off + inc - v;
}

// min over the workgroup, to every thread.  red: 8 dwords of LDS, free again on return
template <int NT, class T>
__device__ __forceinline__ T yin_min(T v, T *red, int lane, int wave) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const T u = __shfl_xor(v, m);
        v = u < v ? u : v;
    }
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T r = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = red[w] < r ? red[w] : r;
    __syncthreads();
    return r;
}

__device__ __forceinline__ float yin_snap(float v) { return fabs((double)v) >= 1e-6 ? v : 0.f; }

// offset of the parabola through (k - 1, k, k + 1), 0 at the borders and beyond one lag (_pitch_yin.c:462-503)
__device__ __forceinline__ float yin_offset(const float *y, int k, int yinLength) {
    if (k < 1 || k > yinLength - 2) return 0.f;
    const float v1 = y[yin_skew(k - 1)], v2 = y[yin_skew(k)], v3 = y[yin_skew(k + 1)];
    const float num = (v3 - v1) / 2.f;
    const float den = (v1 + v3 - 2.f * v2) / 2.f;
    const float off = (float)(-(double)num / ((double)(2.f * den) + 1e-16));
    return fabsf(off) <= 1.f ? off : 0.f;
}

template <int R>
__global__ void __launch_bounds__(YinCfg<R>::NT) k_pitch_yin(AfxPitchYinArgs a) {
    using C = YinCfg<R>;
    constexpr int N = C::N, NT = C::NT, PER = C::PER, NP = C::NP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *red = reinterpret_cast<double *>(smem_raw);              // [16]: cross-wave exchange of scans and reductions
    float2 *s = reinterpret_cast<float2 *>(red + 16);                // transform buffer, afx_lds_pad addressing
    float *xe = reinterpret_cast<float *>(s + afx_lds_padded_size(N));  // samples -> energy prefix -> the curve, yin_skew addressing

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x;
    int b, t;
    const float *x = afx_pitch_row(a.x, row, a.timeLength, a.clipStride, a.hop, b, t);
    const int A = a.autoLength, minIndex = a.minIndex, maxIndex = a.maxIndex, Y = maxIndex - minIndex + 1;

    // 1. the frame (neighbouring frames overlap: re-read through L2)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = tid + NT * i;
        const float v = x[j];
        xe[yin_skew(j)] = v;
        s[afx_lds_pad(j)] = make_float2(v, 0.f);
    }
    __syncthreads();

    // 2. E[j] = x[0]^2 + ... + x[j]^2, accumulated in double, kept as float over the samples
    double eAll;
    {
        double e[PER], run = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const float v = xe[yin_skew(tid * PER + i)];
            run += (double)v * (double)v;
            e[i] = run;
        }
        const double base = yin_scan<NT>(run, red, lane, wave, &eAll);
#pragma unroll
        for (int i = 0; i < PER; ++i) xe[yin_skew(tid * PER + i)] = (float)(base + e[i]);
    }
    __syncthreads();

    // 2b. the reversed prefix y[n] = x[A - n], n <= A, as the imaginary part -- times 2^g, so that both halves of the packed
    //     transform have the same scale: Y comes out of Z with an error relative to |Z|, and a quiet prefix inside a loud
    //     frame (an onset) would otherwise put noise above the 1e-6 snap where the reference has exact zeros
    int g = 30;
    {
        const float eY = xe[yin_skew(A)];
        if (eY > 0.f) {
            const int h = ilogb(eAll / (double)eY) / 2;  // eAll >= eY: h >= 0
            g = h < 30 ? h : 30;
        }
        const float up = ldexpf(1.f, g);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = tid + NT * i;
            if (j <= A) s[afx_lds_pad(j)].y = x[A - j] * up;
        }
    }
    __syncthreads();

    // 3. Z = FFT(x + i y), Z[k] at s[bitrev(k)]
    const float2 *tw = reinterpret_cast<const float2 *>(a.twiddle);
    afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);

    // 4. Q = conj(X Y) in natural order for the second transform; the factors 1/2 of X and Y are applied with 1/N at the end
    {
        float2 q0[NP], q1[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int k = tid + NT * i;
            q0[i] = q1[i] = make_float2(0.f, 0.f);
            if (k == 0) {  // bins 0 and N/2 pair with themselves: X = 2 Re Z, Y = 2 Im Z
                const float2 z0 = s[afx_lds_pad(0)], zh = s[afx_lds_pad(1)];
                q0[i] = make_float2(4.f * z0.x * z0.y, 0.f);
                q1[i] = make_float2(4.f * zh.x * zh.y, 0.f);
            } else if (k < N / 2) {
                const float2 zk = s[afx_lds_pad((int)(__brev((unsigned)k) >> (32 - R)))];
                const float2 zn = s[afx_lds_pad((int)(__brev((unsigned)(N - k)) >> (32 - R)))];
                const float xr = zk.x + zn.x, xi = zk.y - zn.y;  // 2 X = Z[k] + conj Z[N-k]
                const float yr = zk.y + zn.y, yi = zn.x - zk.x;  // 2 Y = (Z[k] - conj Z[N-k]) / i
                const float pr = xr * yr - xi * yi, pi = xr * yi + xi * yr;
                q0[i] = make_float2(pr, -pi);  // Q[k] = conj P[k]
                q1[i] = make_float2(pr, pi);   // Q[N-k] = conj P[N-k] = P[k]
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int k = tid + NT * i;
            if (k < N / 2) {
                s[afx_lds_pad(k)] = q0[i];
                s[afx_lds_pad(k == 0 ? N / 2 : N - k)] = q1[i];
            }
        }
        __syncthreads();
    }
    afx_lds_fft_dif_t<true>(s, R, tw, 1, tid, NT);  // 4 N c[n] = Re s[bitrev(n)]

    // 5. d[j] for the thread's lags, the running sum from lag 1 on, the curve
    float yv[PER];
    {
        const float scale = ldexpf(0.25f / (float)N, -g);
        const float e0 = yin_snap(xe[yin_skew(A)] - xe[yin_skew(0)]);
        float d[PER];
        double cum[PER], run = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = tid * PER + i;
            float v = 0.f;
            if (j <= maxIndex) {  // maxIndex <= N - A - 1: A + j stays inside the frame
                const float r = yin_snap(s[afx_lds_pad((int)(__brev((unsigned)(A + j)) >> (32 - R)))].x * scale);
                const float e = yin_snap(xe[yin_skew(A + j)] - xe[yin_skew(j)]);
                v = e0 + e - 2.f * r;
                if (j >= 1) run += (double)v;
            }
            d[i] = v;
            cum[i] = run;
        }
        const double base = yin_scan<NT>(run, red, lane, wave, nullptr);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = tid * PER + i;
            const float mean = (float)(base + cum[i]) / (float)j;
            yv[i] = (float)((double)d[i] / ((double)mean + 1e-16));
        }
    }
    __syncthreads();  // every thread has read E and the correlation: the curve takes the place of E
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = tid * PER + i;
        if (j >= minIndex && j <= maxIndex) xe[yin_skew(j - minIndex)] = yv[i];
    }
    __syncthreads();

    // 6. the decision: thread-local over its PER lags of the curve, then over the workgroup
    float mn = __builtin_huge_valf();
    int first = 0x7fffffff, count = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = tid * PER + i;
        if (k < Y) {
            const float y = xe[yin_skew(k)];
            mn = y < mn ? y : mn;
            if (k <= Y - 2) {
                const float yr = xe[yin_skew(k + 1)];
                bool hit = y < a.thresh;
                if (k == 0) hit = hit && y < yr;
                else hit = hit && y <= yr && y < xe[yin_skew(k - 1)];
                if (hit) {
                    first = first < k ? first : k;
                    ++count;
                }
            }
        }
    }
    mn = yin_min<NT>(mn, reinterpret_cast<float *>(red), lane, wave);
    const int kf = yin_min<NT>(first, reinterpret_cast<int *>(red), lane, wave);
    if (tid == 0) {
        const long long at = (long long)b * a.outStride + t;
        float fre = 0.f, val = 0.f;
        if (kf != 0x7fffffff) {
            fre = (float)a.samplate / ((float)(minIndex + kf) + yin_offset(xe, kf, Y));
            val = xe[yin_skew(kf)];
        }
        if (a.fre) a.fre[at] = fre;
        if (a.trough) a.trough[at] = val;
        if (a.minv) a.minv[at] = mn;
    }
    if (a.candLen) {  // all qualifying troughs in lag order, the first candPitch stored
        double total;
        const int base = (int)yin_scan<NT>((double)count, red, lane, wave, &total);
        int at = base;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = tid * PER + i;
            if (k <= Y - 2 && at < a.candPitch) {
                const float y = xe[yin_skew(k)], yr = xe[yin_skew(k + 1)];
                bool hit = y < a.thresh;
                if (k == 0) hit = hit && y < yr;
                else hit = hit && y <= yr && y < xe[yin_skew(k - 1)];
                if (hit) {
                    if (a.candFre) {
                        a.candFre[row * a.candPitch + at] = (float)a.samplate / ((float)(minIndex + k) + yin_offset(xe, k, Y));
                        a.candVal[row * a.candPitch + at] = y;
                    }
                    ++at;
                }
            }
        }
        if (tid == 0) a.candLen[row] = (int)total;
    }
    if (a.curve)
        for (int k = tid; k < Y; k += NT) a.curve[row * Y + k] = xe[yin_skew(k)];
}

template <int R>
int launch(const AfxPitchYinArgs &a, long long rows, void *stream) {
    using C = YinCfg<R>;
    AFX_LAUNCH_DYN_LDS(k_pitch_yin<R>, dim3((unsigned)rows), dim3(C::NT), C::LDS, stream, a);
    AFX_LAUNCH_CHECK("k_pitch_yin");
    return AFX_OK;
}

}  // namespace

extern "C" int afxk_pitch_yin(const AfxPitchYinArgs *a, void *stream) {
    if (!a || !a->x || !a->twiddle || a->batch <= 0 || a->timeLength <= 0 || a->hop <= 0) return AFX_ERR_ARG;
    if (a->radix2Exp < 6 || a->radix2Exp > 13) return AFX_ERR_UNSUPPORTED;
    const int N = 1 << a->radix2Exp;
    // the limits the kernel's indexing rests on
    if (a->autoLength < 0 || a->autoLength >= N || a->minIndex < 1 || a->maxIndex < a->minIndex + 2 ||
        a->maxIndex > N - a->autoLength - 1)
        return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    if ((a->candFre != NULL) != (a->candVal != NULL) || ((a->candFre || a->candLen) && a->candPitch < 0)) return AFX_ERR_ARG;
    if (a->candFre && !a->candLen) return AFX_ERR_ARG;
    if (!a->fre && !a->trough && !a->minv && !a->candLen && !a->curve) return AFX_OK;
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
        case 12: return launch<12>(*a, rows, stream);
        default: return launch<13>(*a, rows, stream);
    }
}
