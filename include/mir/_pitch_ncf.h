/* _pitch_ncf.h -- C ABI of the normalised-autocorrelation pitch tracker: per frame of fftLength = N samples the power
 * spectrum P[k] = |X[k]|^2 of the windowed frame zero-padded to 2N points, its inverse transform r (the autocorrelation),
 * the curve c[i] = (2N)^(-1/4) r[i + 1] / sqrt(r[0]) and the first maximum of c over minIndex ... maxIndex;
 * freArr = samplate / (index + 1).
 *
 * Replaces the reference functions of the same names (src/mir/_pitch_ncf.h, src/mir/_pitch_ncf.c:77-522) as bound by
 * python/audioflux/mir/pitch_ncf.py.  Everything between the samples and the result per frame runs in ONE kernel launch
 * (csrc/hip/afx_pitch_lag.hip, shared with mir/_pitch_cep.h) and stays in LDS: two 2N-point transforms in one buffer, the
 * second one the inverse run as a forward transform of the real, even power spectrum.
 *
 * Deviations from the reference:
 *  - radix2Exp outside 6 ... 12 returns -100 and leaves *pitchNCFObj NULL (the reference falls back to 12 for values
 *    outside 1 ... 30 and accepts the rest).  13 would need a 16384-point buffer: 128 KB of LDS, one workgroup per CU.
 *  - plans in which the reference overruns its own buffers return -6 and a NULL handle:
 *      maxIndex > N - 1: the rearrangement before the normalisation (_pitch_ncf.c:456-457) writes 2 maxIndex + 1 floats
 *        into a 2N buffer (heap corruption, e.g. N = 64 with maxIndex 250);
 *      minIndex < 1 (a samplate below highFre / 2, reachable only with the default highFre): the row's zero fill
 *        (:462) gets a negative length.
 *  - curve[maxIndex] is always 0.  The reference never computes that entry; its peak pick reads it from a row buffer that
 *    is zeroed when it is allocated and reused between calls, so a NaN the peak pick of an EARLIER call left there can
 *    survive.  It matters only when every real lag is negative.
 *  - the spectra come from float32 transforms of another factorisation than the reference's: low-order bits of the curve
 *    differ; the decision differs only where two candidates were within rounding (tests/pitch_lag_check.py states what is
 *    accepted).
 *  - pitchNCFObj_enableDebug prints the parameters only.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef _PITCH_NCF_H
#define _PITCH_NCF_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>

#include "../flux_base.h"

typedef struct OpaquePitchNCF *PitchNCFObj;

/* _pitch_ncf.c:77-235.  NULL arguments take the defaults: samplate 32000 (accepted 1 ... 196000), lowFre 32 (values below
 * 27 are ignored), highFre 2000 -- a value outside (lowFre, samplate / 2), samplate / 2 by integer division, resets BOTH to
 * 32 / 2000 --, radix2Exp 12, slideLength fftLength / 4 (any positive value, also > fftLength), windowType Rect (any type),
 * isContinue 0.  minIndex = roundf(samplate / highFre), maxIndex = roundf(samplate / lowFre) in float32.  Returns 0,
 * -100 / -6 (see above) or a device status (afx_last_error()). */
int pitchNCFObj_new(PitchNCFObj *pitchNCFObj,
				int *samplate,float *lowFre,float *highFre,
				int *radix2Exp,int *slideLength,WindowType *windowType,
				int *isContinue);

/* _pitch_ncf.c:166-191: frames of a call with dataLength samples; with isContinue the kept tail counts */
int pitchNCFObj_calTimeLength(PitchNCFObj pitchNCFObj,int dataLength);

/* _pitch_ncf.c:358-494.  Per frame i at i * slideLength: window (Rect: no multiply), P = |X|^2 over the 2N bins of the
 * zero-padded frame, r = Re ifft(P) / 2N, c[k] as above for k = minIndex - 1 ... maxIndex - 1 and 0 elsewhere, index = first
 * argmax of c over minIndex ... maxIndex (a strict >; a silent frame has r[0] = 0, a row of NaN, and gives minIndex),
 * freArr[i] = samplate / (index + 1).  With isContinue the samples a call leaves unused (or, with a hop above fftLength,
 * the number still to skip) carry over to the next call (:237-356).  A failure is recorded on the calling thread
 * (afx_error_count()). */
void pitchNCFObj_pitch(PitchNCFObj pitchNCFObj,float *dataArr,int dataLength,
					float *freArr);

/* _pitch_ncf.c:496-499 */
void pitchNCFObj_enableDebug(PitchNCFObj pitchNCFObj,int isDebug);
/* _pitch_ncf.c:501-522 */
void pitchNCFObj_free(PitchNCFObj pitchNCFObj);

/* ---- additive: clips that already live in HBM ---------------------------------------------------------------------------
 * `batch` clips of dataLength samples, clip b at dData + b * clipStride (clipStride >= dataLength), frames =
 * (dataLength - fftLength) / slideLength + 1 each.  dFre / dValue [b * outStride + t], outStride >= frames: the frequency
 * and the curve's entry at the chosen index, bit for bit (dValue may be NULL); every frame is written, nothing else.  One
 * launch, asynchronous on hipStream.  Returns 0; -4 for an object created with isContinue (it carries one signal's tail);
 * -6 for NULL / non-positive / short-stride arguments; 0 without writing anything when dataLength < fftLength. */
int pitchNCFObj_pitchBatchDevice(PitchNCFObj pitchNCFObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dFre, float *dValue, long long outStride, void *hipStream);
/* the head of each mCorrArr row: dCurve[(b * frames + t) * (maxIndex + 1) + k], k = 0 ... maxIndex */
int pitchNCFObj_curveBatchDevice(PitchNCFObj pitchNCFObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dCurve, void *hipStream);
int pitchNCFObj_minIndex(PitchNCFObj pitchNCFObj);
int pitchNCFObj_maxIndex(PitchNCFObj pitchNCFObj);

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
 * -6).  afx_pitch_ncf_plan_free releases the window of any plan this call filled. */
int afx_pitch_ncf_plan_host(int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength, WindowType *windowType,
                            int *isContinue, AfxPitchLagPlan *plan);
void afx_pitch_ncf_plan_free(AfxPitchLagPlan *plan);

#ifdef __cplusplus
}
#endif

#endif
