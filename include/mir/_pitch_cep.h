/* _pitch_cep.h -- C ABI of the cepstrum pitch tracker: per frame of fftLength = N samples the log power spectrum
 * ln |X[k]|^2 of the windowed frame zero-padded to 2N points, its inverse transform c (the real cepstrum) and the first
 * maximum of c over the quefrencies minIndex ... maxIndex; freArr = samplate / (index + 1).
 *
 * Replaces the reference functions of the same names (src/mir/_pitch_cep.h, src/mir/_pitch_cep.c:77-502) as bound by
 * python/audioflux/mir/pitch_cep.py.  Everything between the samples and the result per frame runs in ONE kernel launch
 * (csrc/hip/afx_pitch_lag.hip, shared with mir/_pitch_ncf.h) and stays in LDS: two 2N-point transforms in one buffer, the
 * second one the inverse run as a forward transform of the real, even log spectrum.
 *
 * Deviations from the reference:
 *  - radix2Exp outside 6 ... 12 returns -100 and leaves *pitchCEPObj NULL (the reference falls back to 12 for values
 *    outside 1 ... 30 and accepts the rest).  13 would need a 16384-point buffer: 128 KB of LDS, one workgroup per CU.
 *  - plans in which the reference reads out of bounds return -6 and a NULL handle:
 *      maxIndex > 2N - 1: the peak pick (_pitch_cep.c:471) reads past the row of 2N entries.
 *  - a frame in which any of the kernel's own 2N power bins is exactly 0 (a silent frame above all) has NaN in the whole
 *    row and the index minIndex.  The reference's result there depends on how -inf runs through its radix-2 butterflies.
 *  - the spectra come from float32 transforms of another factorisation than the reference's: low-order bits of the curve
 *    differ; the decision differs only where two candidates were within rounding (tests/pitch_lag_check.py states what is
 *    accepted).
 *  - pitchCEPObj_enableDebug prints the parameters only.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef _PITCH_CEP_H
#define _PITCH_CEP_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>

#include "../flux_base.h"

typedef struct OpaquePitchCEP *PitchCEPObj;

/* _pitch_cep.c:77-237.  NULL arguments take the defaults: samplate 32000 (accepted 1 ... 196000), lowFre 32 (values below
 * 27 are ignored), highFre 2000 -- a value outside (lowFre, samplate / 2), samplate / 2 by integer division, resets BOTH to
 * 32 / 2000 --, radix2Exp 12, slideLength fftLength / 4 (any positive value, also > fftLength), windowType Hamm (a value is
 * taken only if it is <= Hamm: Rect, Hann, Hamm), isContinue 0.  minIndex = roundf(samplate / highFre), maxIndex =
 * roundf(samplate / lowFre) in float32.  Returns 0, -100 / -6 (see above) or a device status (afx_last_error()). */
int pitchCEPObj_new(PitchCEPObj *pitchCEPObj,
				int *samplate,float *lowFre,float *highFre,
				int *radix2Exp,int *slideLength,WindowType *windowType,
				int *isContinue);

/* _pitch_cep.c:168-193: frames of a call with dataLength samples; with isContinue the kept tail counts */
int pitchCEPObj_calTimeLength(PitchCEPObj pitchCEPObj,int dataLength);

/* _pitch_cep.c:360-474.  Per frame i at i * slideLength: window (Rect: no multiply), ln |X|^2 over the 2N bins of the
 * zero-padded frame, c = Re ifft(ln |X|^2) / 2N, index = first argmax of c over minIndex ... maxIndex (a strict >; a silent
 * frame gives minIndex), freArr[i] = samplate / (index + 1).  With isContinue the samples a call leaves unused (or, with a
 * hop above fftLength, the number still to skip) carry over to the next call (:239-358).  A failure is recorded on the
 * calling thread (afx_error_count()). */
void pitchCEPObj_pitch(PitchCEPObj pitchCEPObj,float *dataArr,int dataLength,
					float *freArr);

/* _pitch_cep.c:476-479 */
void pitchCEPObj_enableDebug(PitchCEPObj pitchCEPObj,int isDebug);
/* _pitch_cep.c:481-502 */
void pitchCEPObj_free(PitchCEPObj pitchCEPObj);

/* ---- additive: clips that already live in HBM ---------------------------------------------------------------------------
 * `batch` clips of dataLength samples, clip b at dData + b * clipStride (clipStride >= dataLength), frames =
 * (dataLength - fftLength) / slideLength + 1 each.  dFre / dValue [b * outStride + t], outStride >= frames: the frequency
 * and the curve's entry at the chosen index, bit for bit (dValue may be NULL); every frame is written, nothing else.  One
 * launch, asynchronous on hipStream.  Returns 0; -4 for an object created with isContinue (it carries one signal's tail);
 * -6 for NULL / non-positive / short-stride arguments; 0 without writing anything when dataLength < fftLength. */
int pitchCEPObj_pitchBatchDevice(PitchCEPObj pitchCEPObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dFre, float *dValue, long long outStride, void *hipStream);
/* the head of each mCepArr row: dCurve[(b * frames + t) * (maxIndex + 1) + q], q = 0 ... maxIndex */
int pitchCEPObj_curveBatchDevice(PitchCEPObj pitchCEPObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dCurve, void *hipStream);
int pitchCEPObj_minIndex(PitchCEPObj pitchCEPObj);
int pitchCEPObj_maxIndex(PitchCEPObj pitchCEPObj);

/* what pitchNCFObj_new / pitchCEPObj_new decide, without a device */
#ifndef AFX_PITCH_LAG_PLAN
#define AFX_PITCH_LAG_PLAN
typedef struct {
    int samplate, radix2Exp, fftLength, slideLength, isContinue;
    int windowType;
    float lowFre, highFre;
    int minIndex, maxIndex;
    int lagLength;       /* 2N: points of the two transforms */
    long long ldsBytes;  /* LDS one workgroup declares */
    float *window;       /* [N]: winDataArr, the plan's own copy, bit for bit the reference's; NULL after -100 */
} AfxPitchLagPlan;
#endif
/* Fills *plan and returns the constructor's status: 0, -100, -6 (plan then holds what was decided, the window included for
 * -6).  afx_pitch_cep_plan_free releases the window of any plan this call filled. */
int afx_pitch_cep_plan_host(int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength, WindowType *windowType,
                            int *isContinue, AfxPitchLagPlan *plan);
void afx_pitch_cep_plan_free(AfxPitchLagPlan *plan);

#ifdef __cplusplus
}
#endif

#endif
