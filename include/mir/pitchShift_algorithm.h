/* pitchShift_algorithm.h -- C ABI of the pitch-shift object: a time stretch by rate = 2^(-nSemitone / 12), then the
 * band-limited resampler (ResampleQuality_Fast, isScale 1) at ratio `rate`, which brings the signal back to its length.
 *
 * Replaces the reference functions of the same names (src/mir/pitchShift_algorithm.h, src/mir/pitchShift_algorithm.c:28-89) as
 * bound by python/audioflux/mir/pitch_shift.py.  The object owns a time-stretch object (timeStretch_algorithm.h) and a
 * resampler (dsp/resample_algorithm.h); there is no CPU compute path.
 *
 * Deviations from the reference (those of the time-stretch object apply too):
 *  - never more than dataLength1 samples are written.  The reference writes floorf(roundf(n / rate) * rate), which is n + 1
 *    for odd n at nSemitone = -12: one past the array its wrapper allocates.  Where the resampled length is below n (2999 of
 *    3000 at -5 semitones) the remaining samples are left as the caller gave them.
 *  - the destination is overwritten; the reference accumulates onto it and its wrapper passes zeros.
 *  - NULL arguments and dataLength1 < fftLength: recorded (afx_error_count()), nothing is written.
 */
#ifndef PITCHSHIFT_ALGORITHM_H
#define PITCHSHIFT_ALGORITHM_H

#include "../flux_base.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaquePitchShift *PitchShiftObj;

/* the arguments of timeStretchObj_new.  replaces pitchShift_algorithm.c:28-48 */
int pitchShiftObj_new(PitchShiftObj *pitchShiftObj,int *radix2Exp,int *slideLength,WindowType *windowType);

/* dataArr1[dataLength1] -> dataArr2[min(dataLength1, floorf(roundf(dataLength1 / rate) * rate))]; |nSemitone| > 12
 * returns without writing; samplate has no effect on the result.  Host pointers.  replaces pitchShift_algorithm.c:51-79 */
void pitchShiftObj_pitchShift(PitchShiftObj pitchShiftObj,int samplate,int nSemitone,float *dataArr1,int dataLength1,float *dataArr2);

/* (two underscores: the reference's spelling, pitchShift_algorithm.c:81) */
void pitchShiftObj__free(PitchShiftObj pitchShiftObj);

/* ---- additive: clips that already live in HBM (the contract at the top of afx_batch.h) ---------------------------------
 * -> dOut[b * outStride + i], i < the returned length = min(dataLength, resampled length); bit for bit what
 * pitchShiftObj_pitchShift writes.  Asynchronous on hipStream; only a call whose rate differs from the previous call's waits for the
 * resampler table's readers, rescales the table and uploads it.  0 for |nSemitone| > 12; -6 for NULL / non-positive / short-stride arguments
 * or a clip that holds no frame. */
int pitchShiftObj_pitchShiftBatchDevice(PitchShiftObj pitchShiftObj, int nSemitone, const float *dData, int batch, int dataLength,
                                        long long clipStride, float *dOut, long long outStride, void *hipStream);
/* the limit of the owned time-stretch object and of this object's own scratch (stretched and resampled clips), each */
void pitchShiftObj_setScratchLimit(PitchShiftObj pitchShiftObj, long long bytes);

#ifdef __cplusplus
}
#endif
#endif /* PITCHSHIFT_ALGORITHM_H */
