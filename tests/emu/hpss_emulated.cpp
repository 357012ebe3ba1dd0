// the DEVICE code of audioflux_amd/csrc/hip/afx_hpss.hip (k_hpss_tile in its separation and its two median forms, k_median_rank)
// compiled for the host against tests/emu/hip/hip_runtime.h; exports afxk_hpss_mask / afxk_median_filter.  The forward transform
// the host object asks for (afxk_stft: complex bins of in-clip frames) is supplied here as a float64 loop that does what
// afx_device.h says the kernel does; the inverse is the emulated device code of tests/emu/istft_emulated.cpp.
#include "hip/hip_runtime.h"

#include <complex>
#include <vector>
namespace {
alignas(16) unsigned char smem_raw[160 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_hpss.hip"

extern "C" int afxk_stft(const AfxStftArgs *a, void *) {
    if (a->mode != AFX_SPEC_COMPLEX || a->padLeft || a->padMode || a->bandStart || a->fullSpectrum) return AFX_ERR_UNSUPPORTED;
    const int N = 1 << a->radix2Exp;
    const long long pitch = a->outPitch ? a->outPitch : a->binCount;
    const double PI = 3.14159265358979323846;
    std::vector<std::complex<double>> v(N), tw(N / 2);
    for (int k = 0; k < N / 2; ++k) tw[k] = std::polar(1.0, -2.0 * PI * k / N);
    for (int b = 0; b < a->batch; ++b)
        for (int t = 0; t < a->timeLength; ++t) {
            const float *x = a->x + (long long)b * a->clipStride + (long long)t * a->hop;
            for (int i = 0; i < N; ++i) {  // bit-reversed load, then radix-2 decimation in time
                int rev = 0;
                for (int s = 0; s < a->radix2Exp; ++s) rev |= ((i >> s) & 1) << (a->radix2Exp - 1 - s);
                v[rev] = (double)x[i] * (double)a->window[i];
            }
            for (int len = 2; len <= N; len <<= 1)
                for (int i = 0; i < N; i += len)
                    for (int k = 0; k < len / 2; ++k) {
                        const std::complex<double> u = v[i + k], w = v[i + k + len / 2] * tw[(size_t)k * (N / len)];
                        v[i + k] = u + w;
                        v[i + k + len / 2] = u - w;
                    }
            const long long row = (long long)b * a->timeLength + t;
            for (int j = 0; j < a->binCount; ++j) {
                a->outRe[row * pitch + j] = (float)v[a->binLo + j].real();
                a->outIm[row * pitch + j] = (float)v[a->binLo + j].imag();
            }
        }
    return AFX_OK;
}
