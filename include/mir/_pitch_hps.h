/* _pitch_hps.h -- C ABI of the harmonic-product-spectrum pitch tracker: per frame of fftLength samples the magnitude
 * spectrum of the windowed frame, zero-padded to interpFFTLength M = util_roundPowerTwo(samplate) points (about one bin
 * per hertz), the product curve[j] = |X[j]| |X[2j]| ... |X[harmonicCount j]| over the candidates j = 0 ... maxIndex, and
 * the first maximum of the curve over minIndex ... maxIndex.
 *
 * Replaces the reference functions of the same names (src/mir/_pitch_hps.h, src/mir/_pitch_hps.c:81-546) as bound by
 * python/audioflux/mir/pitch_hps.py.  Everything between the samples and the result per frame runs in ONE kernel launch
 * (csrc/hip/afx_pitch_hs.hip, shared with mir/_pitch_lhs.h); neither the M-point transform nor the reference's
 * [timeLength, M] plane exists: only the bins 0 ... maxIndex * harmonicCount are computed, as M / fftLength modulated
 * fftLength-point transforms held in LDS.
 *
 * Deviations from the reference:
 *  - radix2Exp outside 6 ... 13 returns -100 and leaves *pitchHPSObj NULL (the reference falls back to 12 for values
 *    outside 1 ... 30 and accepts the rest).
 *  - plans with fftLength > M (e.g. samplate 2000, radix2Exp 12) return -6 and a NULL handle: the reference copies
 *    fftLength floats into its M-float frame buffer (_pitch_hps.c:469-472).
 *  - plans with maxIndex * harmonicCount >= M return -6 and a NULL handle: the reference reads past its M-bin spectrum
 *    (_pitch_hps.c:482-486).  Reachable when M < samplate (44100 Hz, highFre 8000, 5 harmonics) and, for THIS object,
 *    whenever harmonicCount exceeds samplate / (maxIndex + 1): the reference computes that clamp (_pitch_hps.c:246-252)
 *    but never stores it, so pitchHPSObj_harmonicCount returns the count as given.  (pitchLHSObj stores it.)
 *  - the spectrum comes from float32 transforms of another factorisation than the reference's radix-2 pass over M points:
 *    low-order bits of the curve differ; the decision differs only where two candidates were within rounding
 *    (tests/pitch_hs_check.py states what is accepted).
 *  - pitchHPSObj_enableDebug prints the parameters only.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef _PITCH_HPS_H
#define _PITCH_HPS_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>

#include "../flux_base.h"

typedef struct OpaquePitchHS *PitchHPSObj;

/* _pitch_hps.c:81-185, :214-269.  NULL arguments take the defaults: samplate 32000 (accepted 1 ... 196000), lowFre 32
 * (values below 27 are replaced by 32), highFre 2000 -- a value outside (lowFre, samplate / 2), samplate / 2 by integer
 * division, resets BOTH to 32 / 2000 --, radix2Exp 12, slideLength fftLength / 4 (any positive value, also > fftLength),
 * windowType Hamm (a type above Window_Hamm falls back to Hamm), harmonicCount 5 (> 0), isContinue 0.
 * minIndex = ceilf(lowFre), maxIndex = floorf(highFre): hertz used as bin indices of the M-point spectrum.
 * Returns 0, -100 / -6 (see above) or a device status (afx_last_error()). */
int pitchHPSObj_new(PitchHPSObj *pitchHPSObj,
				int *samplate,float *lowFre,float *highFre,
				int *radix2Exp,int *slideLength,WindowType *windowType,
				int *harmonicCount,
				int *isContinue);

/* _pitch_hps.c:187-212: frames of a call with dataLength samples; with isContinue the kept tail counts */
int pitchHPSObj_calTimeLength(PitchHPSObj pitchHPSObj,int dataLength);

/* _pitch_hps.c:393-518.  Per frame i at i * slideLength: window (skipped for Window_Rect), |X[m]| = sqrtf(re^2 + im^2) of
 * the M-point transform of the zero-padded frame, curve[j] = prod_{k < harmonicCount} |X[j (k + 1)]| in float32 in that
 * order, index = first argmax over minIndex ... maxIndex (an all-zero frame gives minIndex), freArr[i] =
 * (index + 1) * (1.0 * samplate / M) -- the + 1 is the reference's.  With isContinue the samples a call leaves unused
 * (or, with a hop above fftLength, the number still to skip) carry over to the next call (:271-390).  A failure is
 * recorded on the calling thread (afx_error_count()). */
void pitchHPSObj_pitch(PitchHPSObj pitchHPSObj,float *dataArr,int dataLength,
					float *freArr);

/* _pitch_hps.c:520-523 */
void pitchHPSObj_enableDebug(PitchHPSObj pitchHPSObj,int isDebug);
/* _pitch_hps.c:525-546 */
void pitchHPSObj_free(PitchHPSObj pitchHPSObj);

/* ---- additive: clips that already live in HBM ---------------------------------------------------------------------------
 * `batch` clips of dataLength samples, clip b at dData + b * clipStride (clipStride >= dataLength), frames =
 * (dataLength - fftLength) / slideLength + 1 each.  dFre / dValue [b * outStride + t], outStride >= frames: the frequency
 * and the curve's value at the chosen index (dValue may be NULL); every frame is written, nothing else.  One launch,
 * asynchronous on hipStream.  Returns 0; -4 for an object created with isContinue (it carries one signal's tail); -6 for
 * NULL / non-positive / short-stride arguments; 0 without writing anything when dataLength < fftLength. */
int pitchHPSObj_pitchBatchDevice(PitchHPSObj pitchHPSObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dFre, float *dValue, long long outStride, void *hipStream);
/* the curve the reference keeps in mHpsArr: dCurve[(b * frames + t) * (maxIndex + 1) + j], j = 0 ... maxIndex (the entries
 * below minIndex included) */
int pitchHPSObj_curveBatchDevice(PitchHPSObj pitchHPSObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dCurve, void *hipStream);
int pitchHPSObj_minIndex(PitchHPSObj pitchHPSObj);
int pitchHPSObj_maxIndex(PitchHPSObj pitchHPSObj);
int pitchHPSObj_harmonicCount(PitchHPSObj pitchHPSObj); /* as the object uses it: see the deviations */
int pitchHPSObj_interpLength(PitchHPSObj pitchHPSObj);  /* M */

/* what pitchHPSObj_new / pitchLHSObj_new decide, without a device */
typedef struct {
    int samplate, radix2Exp, fftLength, slideLength, isContinue;
    float lowFre, highFre;
    int windowType;    /* after the fallback */
    int interpLength;  /* M */
    int minIndex, maxIndex;
    int harmonicCount; /* as the object uses it */
    int lastBin;       /* maxIndex * harmonicCount: the highest bin read */
    int transforms;    /* fftLength-point transforms per frame: 1 for M = fftLength, else M / fftLength / 2 + 1 */
    int sliceInLds;    /* 1: the magnitudes of bins 0 ... lastBin stay in LDS; 0: in a per-workgroup slice of device scratch */
    long long sliceFloats;  /* floats of one slice */
    long long ldsBytes;     /* LDS one workgroup declares */
} AfxPitchHsPlan;
/* kind 0: HPS, 1: LHS.  Fills *plan and returns the constructor's status: 0, -100, -6 (plan then holds what was decided up to
 * the refusal). */
int afx_pitch_hs_plan_host(int kind, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,
                           WindowType *windowType, int *harmonicCount, int *isContinue, AfxPitchHsPlan *plan);

#ifdef __cplusplus
}
#endif

#endif
