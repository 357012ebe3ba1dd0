// the DEVICE code of audioflux_amd/csrc/hip/afx_st.hip (k_st_rows) compiled for the host against tests/emu/hip/hip_runtime.h;
// exports afxk_st_rows.  afxk_nsgt_spectrum is a STAND-IN here: a float64 FFT that writes the documented transposed layout
// rounded to float32 -- the forward pass itself (afx_cwt.hip) is not exercised by this build, only the row kernel is.
// Everything else of the device layer is the generated stand-in.
#include "hip/hip_runtime.h"

#include <complex>
#include <vector>

namespace {
alignas(16) unsigned char smem_raw[160 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_st.hip"

extern "C" int afxk_nsgt_spectrum(const AfxCwtPlanDims *d, const float *tw, const float *x, long long xStride, int chunks,
                                  float *scratchA, float *Xt, void *stream) {
    (void)tw; (void)scratchA; (void)stream;
    if (!d || !x || !Xt || d->pad != 0 || d->dataLength != 1 << (d->r1 + d->r2)) return AFX_ERR_ARG;
    const int r = d->r1 + d->r2, N = 1 << r, L1 = 1 << d->r1, L2 = 1 << d->r2;
    const double pi = 3.14159265358979323846;
    std::vector<std::complex<double>> a(N);
    for (int c = 0; c < chunks; ++c) {
        for (int n = 0; n < N; ++n) {  // bit-reversed load, then radix-2 decimation in time
            unsigned rev = 0;
            for (int b = 0; b < r; ++b) rev |= ((unsigned)(n >> b) & 1u) << (r - 1 - b);
            a[rev] = std::complex<double>(x[(long long)c * xStride + n], 0.0);
        }
        for (int len = 2; len <= N; len <<= 1)
            for (int s = 0; s < N; s += len)
                for (int j = 0; j < len / 2; ++j) {
                    const std::complex<double> w = std::polar(1.0, -2.0 * pi * j / len), u = a[s + j], v = a[s + j + len / 2] * w;
                    a[s + j] = u + v;
                    a[s + j + len / 2] = u - v;
                }
        float *out = Xt + 2ll * c * N;
        for (int k = 0; k < N; ++k) {  // frequency k1 + 2^r1 k2 at [k1][k2]
            const int k1 = k & (L1 - 1), k2 = k >> d->r1;
            out[2 * (k1 * L2 + k2)] = (float)a[k].real();
            out[2 * (k1 * L2 + k2) + 1] = (float)a[k].imag();
        }
    }
    return AFX_OK;
}
