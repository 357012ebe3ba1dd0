/* hpss_algorithm.h -- C ABI of the harmonic / percussive source separation object: an STFT (hop fftLength/4, no
 * padding), two median filters over the magnitude plane (order hOrder along time per bin, order pOrder along
 * frequency per frame, zeros outside the plane), a soft mask H = h^2 / (h^2 + p^2) mag, P = p^2 / (h^2 + p^2) mag with
 * the phase re-applied, and one weighted-overlap-add inverse STFT per output.
 *
 * Replaces the reference functions of the same names (src/mir/hpss_algorithm.h:16-31, src/mir/hpss_algorithm.c:40-358)
 * as bound by python/audioflux/mir/hpss.py.  The transforms are the STFT object's kernels (csrc/hip/afx_stft.hip,
 * afx_istft.hip); magnitude, both medians and the mask run in k_hpss_tile (csrc/hip/afx_hpss.hip) without the magnitude
 * or median planes ever existing in memory.  Batched device-pointer calls: afx_batch.h.
 *
 * Deviations from the reference, all on inputs where it crashes or reads stale memory:
 *  - radix2Exp outside 2 ... 14 returns -100 (< 2: the hop fftLength/4 would be 0; > 14: this backend's FFT limit) and
 *    leaves *hpssObj NULL.  The reference ignores stftObj_new's status and crashes in the first call.
 *  - an order of 1 is the identity filter.  The reference skips the filter (flux_vector.c:3009) and masks with whatever
 *    its buffer held: zeros on the first call, the previous call's values afterwards.
 *  - odd orders above 63 return -4 (not implemented) from hpssObj_new instead of failing in a compute call;
 *    afx_medianFilterDevice (afx_batch.h) covers odd orders up to 255.
 *  - fewer samples than fftLength (no frame): nothing is written.
 *  - NaN / Inf samples: unspecified values, no fault (a selection by comparisons and a sort order NaNs differently).
 */
#ifndef HPSS_ALGORITHM_H
#define HPSS_ALGORITHM_H

#include "../flux_base.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueHPSS *HPSSObj;

/* windowType NULL -> Hamm (not Rect as in stftObj_new); hOrder / pOrder NULL, <= 0 or even -> 21 / 31.
 * slideLength is accepted and IGNORED: the hop is always fftLength/4, as in the reference (hpss_algorithm.c:81).
 * returns 0, -100 bad radix2Exp, -4 an order above 63, <= -2 backend failure.  replaces hpss_algorithm.c:40-97 */
int hpssObj_new(HPSSObj *hpssObj, int radix2Exp, WindowType *windowType, int *slideLength, int *hOrder, int *pOrder);

/* samples of the outputs for dataLength input samples: (T - 1) * fftLength/4 + fftLength with
 * T = (dataLength - fftLength) / (fftLength/4) + 1 frames, T = 0 below fftLength samples (the result is then
 * 3 * fftLength/4 by the reference's arithmetic, and nothing is written).  replaces hpss_algorithm.c:99-115 */
int hpssObj_calDataLength(HPSSObj hpssObj, int dataLength);

/* dataArr[dataLength] -> hArr / pArr [hpssObj_calDataLength(dataLength)], ACCUMULATED onto what the arrays hold (like
 * stftObj_istft: pass zeros for the plain result).  Either may be NULL: that output and its inverse transform are skipped;
 * both NULL: returns.  Host pointers; a failure is counted by afx_error_count().  replaces hpss_algorithm.c:117-327 */
void hpssObj_hpss(HPSSObj hpssObj, float *dataArr, int dataLength, float *hArr, float *pArr);

/* replaces hpss_algorithm.c:329-349 */
void hpssObj_free(HPSSObj hpssObj);
/* prints the parameters (the reference's is empty, hpss_algorithm.c:351-353) */
void hpssObj_debug(HPSSObj hpssObj);

#ifdef __cplusplus
}
#endif
#endif /* HPSS_ALGORITHM_H */
