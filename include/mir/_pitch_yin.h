/* _pitch_yin.h -- C ABI of the YIN pitch tracker: per frame of fftLength samples the difference function d[j] (an FFT
 * autocorrelation over the first autoLength + 1 samples plus a running energy), its cumulative-mean normalisation
 * yin[k] over the lags minIndex ... maxIndex, and the first trough below `thresh`, refined by a three-point parabola.
 *
 * Replaces the reference functions of the same names (src/mir/_pitch_yin.h:13-40, src/mir/_pitch_yin.c:87-938) as bound
 * by python/audioflux/mir/pitch_yin.py.  Everything between the samples and the three results per frame runs in ONE
 * kernel launch (csrc/hip/afx_pitch_yin.hip); none of the reference's nine [timeLength, ~fftLength] planes exists.
 * Batched device-pointer calls: afx_batch.h.
 *
 * Deviations from the reference:
 *  - radix2Exp outside 6 ... 13 returns -100 and leaves *pitchYINObj NULL (the reference falls back to 12 for values
 *    outside 1 ... 30 and accepts the rest).
 *  - plans with minIndex = floorf(samplate / highFre) = 0 return -6 and a NULL handle.  They are reachable because the
 *    fallback 2093 Hz / the default 2094 Hz are not re-checked against a low samplate (e.g. 2000); the reference reads
 *    mMeanArr[-1] on them (_pitch_yin.c:437-441).
 *  - plans with yinLength = maxIndex - minIndex + 1 < 3 (autoLength close to fftLength cuts maxIndex) return -6 and a
 *    NULL handle; the reference indexes before its arrays on them.
 *  - the two prefix sums (energy, running mean) are scans accumulated in double where the reference adds serially in
 *    float32: low-order bits of the curve differ; a decision differs only where a comparison was within rounding.
 *  - pitchYINObj_enableDebug prints the parameters only.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef _PITCH_YIN_H
#define _PITCH_YIN_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>

typedef struct OpaquePitchYIN *PitchYINObj;

/* _pitch_yin.c:87-196.  NULL arguments take the defaults: samplate 32000 (accepted 1 ... 196000), lowFre 27 (values below
 * 27 are replaced by 27), highFre 2094 -- a value outside (lowFre, samplate / 2) resets BOTH to 27 / 2093 --, radix2Exp 12,
 * slideLength fftLength / 4 (any positive value, also > fftLength), autoLength fftLength / 2 (accepted 0 ... fftLength - 1),
 * isContinue 0.  minIndex = floorf(samplate / highFre), maxIndex = min(ceilf(samplate / lowFre), fftLength - autoLength - 1),
 * evaluated in float.  Returns 0, -100 / -6 (see above) or a device status (afx_last_error()). */
int pitchYINObj_new(PitchYINObj *pitchYINObj,
				int *samplate,float *lowFre,float *highFre,
				int *radix2Exp,int *slideLength,int *autoLength,
				int *isContinue);

/* _pitch_yin.c:219-228: default 0.1; any thresh > 0 is taken, others are ignored */
void pitchYINObj_setThresh(PitchYINObj pitchYINObj,float thresh);
/* _pitch_yin.c:733-760: frames of a call with dataLength samples; with isContinue the kept tail counts */
int pitchYINObj_calTimeLength(PitchYINObj pitchYINObj,int dataLength);

/* _pitch_yin.c:230-246, :352-560.  Per frame i: the first lag index j <= yinLength - 2 with yin[j] < thresh that is a trough
 * (j = 0: below its right neighbour; else <= right and < left) gives freArr[i] = samplate / (minIndex + j + offset[j]) and
 * valueArr1[i] = yin[j]; WITHOUT such a lag freArr[i] and valueArr1[i] keep what the caller put there.  valueArr2[i] =
 * min(yin).  valueArr1 / valueArr2 may be NULL.  With isContinue the samples a call leaves unused (or, with a hop above
 * fftLength, the number still to skip) carry over to the next call (:791-938).  A failure is recorded on the calling
 * thread (afx_error_count()). */
void pitchYINObj_pitch(PitchYINObj pitchYINObj,float *dataArr,int dataLength,
					float *freArr,float *valueArr1,float *valueArr2);

/* _pitch_yin.c:246-264, :562-603: every trough below thresh of every frame of the last pitch call, in lag order:
 * mFreArr / mTroughArr [timeLength, mLen], lenArr [timeLength]; returns mLen = yinLength / 2 + 1.  The arrays belong to the
 * object and stay valid until its next pitch call or its release. */
int pitchYINObj_getTroughData(PitchYINObj pitchYINObj,float **mFreArr,float **mTroughArr,int **lenArr);

void pitchYINObj_enableDebug(PitchYINObj pitchYINObj,int isDebug);
void pitchYINObj_free(PitchYINObj pitchYINObj);

#ifdef __cplusplus
}
#endif

#endif
