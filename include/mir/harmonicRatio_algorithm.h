/* harmonicRatio_algorithm.h -- C ABI of the harmonic ratio: per frame of windowLength = N = 2^radix2Exp samples the
 * autocorrelation r of the Hamming-windowed frame (through the power spectrum of the frame zero-padded to fftLength = 2N),
 * normalised lag by lag with the energy of the part of the frame the lag still overlaps,
 *     g[j] = r[j] / sqrtf(r[0] * c[j] + 1e-16),   c[j] = sum of f[n]^2 over n <= N - 2 - j,
 * and the first maximum of g between the first zero crossing of r and maxLength = floorf(samplate / lowFre), refined by a
 * three-point parabola.
 *
 * Replaces the reference functions of the same names (src/mir/harmonicRatio_algorithm.h, harmonicRatio_algorithm.c:52-308) as
 * bound by python/audioflux/mir/harmonic_ratio.py.  Everything between the samples and the value per frame runs on the device
 * (csrc/hip/afx_harmonic_ratio.hip) and stays in LDS: the two 2N-point transforms of mir/_pitch_ncf.h in one buffer.
 *
 * What the reference computes and this library reproduces (none of it is "fixed"):
 *  - windowType is read by nobody: the window is always the periodic Hamming window of N points.
 *  - radix2Exp = r gives N = 2^r and transforms of 2N points; with a NULL pointer the TRANSFORM exponent is 12, so N = 2048.
 *  - minIndex, the lag below the first j in 2 ... maxLength with r[j - 1] and r[j] of opposite sign (or zero), is set to 0
 *    once per CALL, not per frame: a frame without such a j inherits the value the nearest earlier frame of the same call
 *    left (0 when there is none).  Splitting a signal over two calls therefore changes such frames.
 *  - an empty range (minIndex = maxLength - 1) gives 0; a maximum at either end of the range is returned as it is; a silent
 *    frame gives 0.
 *  - a frame that starts in silence has c[j] near 0 for a run of lags: g there is r[j] / sqrt(1e-16)-like and the value is
 *    ill-conditioned for any float32 evaluation (tests/harmonic_ratio_check.py prices it).
 *
 * Deviations from the reference:
 *  - radix2Exp outside 6 ... 12 returns -100 and leaves *harmonicRatioObj NULL (the reference accepts radix2Exp + 1 in
 *    1 ... 30 and falls back to N = 2048 for the rest).  13 would need a 16384-point buffer: 128 KB of LDS, one workgroup per CU.
 *  - the running sum c is a workgroup scan, the reference's a serial float32 sum; the spectra come from float32 transforms of
 *    another factorisation: low-order bits differ, a decision differs only where two candidates were within rounding
 *    (tests/harmonic_ratio_check.py states what is accepted).
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef HARMONICRATIO_ALGORITHM_H
#define HARMONICRATIO_ALGORITHM_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>
#include "../flux_base.h"

typedef struct OpaqueHarmonicRatio *HarmonicRatioObj;

/* harmonicRatio_algorithm.c:52-155.  NULL arguments take the defaults: samplate 32000 (accepted 1 ... 196000), lowFre 25
 * (accepted when > 0 and < samplate / 2, samplate / 2 by integer division), radix2Exp: N = 2048 (see above), windowType
 * ignored, slideLength N / 4 (any positive value, also > N).  maxLength = floorf(samplate / lowFre) in float32, at most
 * N - 1.  Returns 0, -100 (see above) or a device status (afx_last_error()). */
int harmonicRatioObj_new(HarmonicRatioObj *harmonicRatioObj,
						int *samplate,float *lowFre,
						int *radix2Exp,WindowType *windowType,int *slideLength);

/* :157-170: 0 for dataLength < N, else (dataLength - N) / slideLength + 1 */
int harmonicRatioObj_calTimeLength(HarmonicRatioObj harmonicRatioObj,int dataLength);
/* :172-287: valueArr[i] of frame i at i * slideLength, as described above; nothing is written when dataLength < N.  A
 * failure is recorded on the calling thread (afx_error_count()). */
void harmonicRatioObj_harmonicRatio(HarmonicRatioObj harmonicRatioObj,float *dataArr,int dataLength,float *valueArr);

void harmonicRatioObj_free(HarmonicRatioObj harmonicRatioObj);

/* ---- additive: clips that already live in HBM ---------------------------------------------------------------------------
 * `batch` clips of dataLength samples, clip b at dData + b * clipStride (clipStride >= dataLength), frames =
 * (dataLength - N) / slideLength + 1 each.  Each clip is ONE reference call: minIndex starts at 0 in every clip and an
 * inherited value never crosses a clip boundary.  dValue / dLag / dFirst [b * outStride + t], outStride >= frames: the value,
 * the lag j of the chosen maximum (-1 for an empty range) and the minIndex the frame used, inherited ones included (dLag and
 * dFirst are int and may be NULL); every frame is written, nothing else.  Three launches, asynchronous on hipStream, no host
 * round trip: every frame with its own crossing, the inherited values per clip, and the frames whose inherited value is not
 * 0 once more -- no input costs more than twice the transforms of one without such frames.  The object keeps 2 ints per
 * frame of scratch (grow-only).  Returns 0; -6 for NULL / non-positive / short-stride arguments; 0 without writing anything
 * when dataLength < N. */
int harmonicRatioObj_harmonicRatioBatchDevice(HarmonicRatioObj harmonicRatioObj, const float *dData, int batch, int dataLength,
                                              long long clipStride, float *dValue, int *dLag, int *dFirst, long long outStride,
                                              void *hipStream);
/* g by lag: dCurve[(b * frames + t) * maxLength + j], j = 0 ... maxLength - 1; entries at j <= minIndex are exact zeros */
int harmonicRatioObj_curveBatchDevice(HarmonicRatioObj harmonicRatioObj, const float *dData, int batch, int dataLength,
                                      long long clipStride, float *dCurve, void *hipStream);
int harmonicRatioObj_maxLength(HarmonicRatioObj harmonicRatioObj);
int harmonicRatioObj_windowLength(HarmonicRatioObj harmonicRatioObj);

/* what harmonicRatioObj_new decides, without a device */
typedef struct {
    int samplate, radix2Exp, windowLength, fftLength, slideLength;
    float lowFre;
    int maxLength;
    long long ldsBytes;  /* LDS one workgroup declares */
    float *window;       /* [windowLength]: winDataArr, the plan's own copy, bit for bit the reference's; NULL after -100 */
} AfxHarmonicRatioPlan;
/* Fills *plan and returns the constructor's status: 0 or -100.  afx_harmonic_ratio_plan_free releases the window of any plan
 * this call filled. */
int afx_harmonic_ratio_plan_host(int *samplate, float *lowFre, int *radix2Exp, WindowType *windowType, int *slideLength,
                                 AfxHarmonicRatioPlan *plan);
void afx_harmonic_ratio_plan_free(AfxHarmonicRatioPlan *plan);

#ifdef __cplusplus
}
#endif

#endif
