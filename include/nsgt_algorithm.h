/* nsgt_algorithm.h -- C ABI of the non-stationary Gabor transform object: one FFT of the whole 2^radix2Exp chunk, then
 * per band a window on a slice of the spectrum, an inverse DFT of the band's own length ("cells"), and a
 * sample-and-hold of every band's cells onto the time grid of the longest band (the [num, maxLength] matrix).
 *
 * Replaces the reference functions of the same names (src/nsgt_algorithm.h, src/nsgt_algorithm.c,
 * src/filterbank/nsgt_filterBank.c) as bound by python/audioflux/nsgt.py.  Execution: the forward pass of the CWT
 * kernels for the spectrum, afx_nsgt.hip for everything per band.  Two deliberate divergences: a plan with a band
 * longer than the chunk is refused (the reference writes past its scratch), and nsgtObj_setMinLength rebuilds the time
 * map with the bank (the reference keeps the stale one and reads past it).
 */
#ifndef NSGT_ALGORITHM_H
#define NSGT_ALGORITHM_H

#include "flux_base.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueNSGT *NSGTObj;

typedef enum {
    NSGTFilterBank_Efficient = 0, /* symmetric windows of 2 max(centre - left, right - centre) + 1 bins */
    NSGTFilterBank_Standard = 1   /* periodic windows of right - left + 1 bins */
} NSGTFilterBankType;

/* num 2..2^radix2Exp/2+1 bands over chunks of 2^radix2Exp samples; optional pointers NULL -> samplate 32000, lowFre 0
 * (octave / log: C1 ... ), highFre samplate/2, binPerOctave 12 (4..48), minLength 3 (the shortest window), bank
 * Efficient, scale Octave, style Hann, normal BandWidth.  Gammatone is taken as Hann, Area as BandWidth.
 * returns 0, -100 bad radix2Exp, 1 bad scale type, -1 bad num / range, -4 where this backend does not run the plan
 * (a band longer than 2^radix2Exp; radix2Exp outside 4..20; more than 2^28 cells or matrix elements per chunk),
 * <= -2 backend failure.  *nsgtObj is NULL unless 0 is returned. */
int nsgtObj_new(NSGTObj *nsgtObj, int num, int radix2Exp, int *samplate, float *lowFre, float *highFre,
                int *binPerOctave, int *minLength, NSGTFilterBankType *nsgtFilterBankType,
                SpectralFilterBankScaleType *filterScaleType, SpectralFilterBankStyleType *filterStyleType,
                SpectralFilterBankNormalType *filterNormalType);

/* minLength >= 1 and different from the current one: the whole plan is rebuilt -- bank, lengths, cells AND the time
 * map.  A plan that would be refused leaves the object as it was; the failure is counted (afx_error_count). */
void nsgtObj_setMinLength(NSGTObj nsgtObj, int minLength);

/* dataArr[2^radix2Exp] -> mRealArr3 / mImageArr3 [num, maxLength] */
void nsgtObj_nsgt(NSGTObj nsgtObj, float *dataArr, float *mRealArr3, float *mImageArr3);

/* the cells of the last nsgtObj_nsgt, band after band, totalLength values: borrowed, valid until the next call or free */
void nsgtObj_getCellData(NSGTObj nsgtObj, float **realArr3, float **imageArr3);

int nsgtObj_getMaxTimeLength(NSGTObj nsgtObj);
int nsgtObj_getTotalTimeLength(NSGTObj nsgtObj);

/* borrowed, num valid entries, valid until nsgtObj_setMinLength or the free */
int *nsgtObj_getTimeLengthArr(NSGTObj nsgtObj);
float *nsgtObj_getFreBandArr(NSGTObj nsgtObj);
int *nsgtObj_getBinBandArr(NSGTObj nsgtObj);

/* NULL-safe */
void nsgtObj_free(NSGTObj nsgtObj);

/* Additive: chunks that already live in HBM.  Chunk c = 2^radix2Exp samples at x + c * xStride -> outRe / outIm
 * [chunks][num][maxLength]; cellRe / cellIm [chunks][totalLength] (both or neither; NULL: the cells are not stored).  All
 * pointers are device pointers; every element of every output is written; asynchronous on `stream` (a HIP stream, NULL: the
 * default stream).  Spectra go through the object's scratch, large batches in passes.  AFX_ERR_ARG (-6): NULL object / x /
 * outRe / outIm, one cell pointer without the other, chunks <= 0, xStride < 2^radix2Exp, a stream of another device than the
 * object's. */
int nsgtObj_nsgtBatchDevice(NSGTObj nsgtObj, const float *x, int chunks, long long xStride, float *outRe, float *outIm,
                            float *cellRe, float *cellIm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSGT_ALGORITHM_H */
