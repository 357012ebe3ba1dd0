/* _pitch_pef.h -- C ABI of the pitch-estimation-filter tracker: per frame of fftLength = N samples the power spectrum of the
 * windowed frame zero-padded to 2N points, interpolated linearly onto 2N logarithmically spaced frequencies and weighted
 * by their band widths, the cross-correlation R[k] = sum_{n < N} h[n] B[n + k] of that log spectrum (B, behind
 * filterPadNum zeros) with the N-tap comb filter h, and the first maximum of R over minIndex ... maxIndex;
 * freArr = the log frequency at that index.
 *
 * Replaces the reference functions of the same names (src/mir/_pitch_pef.h, src/mir/_pitch_pef.c:106-826) as bound by
 * python/audioflux/mir/pitch_pef.py.  Everything between the samples and the result per frame runs in ONE kernel launch
 * (csrc/hip/afx_pitch_pef.hip) and stays in LDS.  The reference correlates through two transforms of 8N points (4N when
 * filterPadNum is 0) per frame and keeps three [timeLength, 8N] planes; only lags 0 ... maxIndex < 2N are ever read, and
 * for those n + k < 3N: nothing wraps at 4N points, so a 4N-point REAL correlation (two 2N-point complex transforms) gives
 * the same lags, and no plane exists.
 *
 * Deviations from the reference:
 *  - radix2Exp outside 6 ... 12 returns -100 and leaves *pitchPEFObj NULL (the reference falls back to 12 for values
 *    outside 1 ... 30 and accepts the rest).  13 does not fit: its 2N-point complex buffer and a fully read spectrum need 167 KB of LDS.
 *  - plans in which the reference itself reads out of bounds return -6 and a NULL handle:
 *      minIndex < 0: lowFre and highFre fall between the same two log frequencies, the search (_pitch_pef.c:465-489)
 *        leaves minIndex at -1;
 *      maxIndex <= minIndex: highFre at or above the last log frequency (e.g. cutFre == highFre) leaves maxIndex at 0;
 *      min(maxIndex + 1, 2N + filterPadNum - 1) != maxIndex + 1: the rearrangement before the peak pick (:418-423) is
 *        the plain "first maximum over minIndex ... maxIndex" only when the two are equal.
 *  - the spectra come from float32 transforms of another factorisation and length than the reference's: low-order bits of
 *    the curve differ; the decision differs only where two candidates were within rounding (tests/pitch_pef_check.py states
 *    what is accepted).
 *  - pitchPEFObj_setFilterParams keeps the reference's OBSERVABLE behaviour: it validates its arguments and changes
 *    nothing (the reference rebuilds the filter from the stored values and never stores the new ones, :685-694).
 *  - pitchPEFObj_enableDebug prints the parameters only.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef _PITCH_PEF_H
#define _PITCH_PEF_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>

#include "../flux_base.h"

typedef struct OpaquePitchPEF *PitchPEFObj;

/* _pitch_pef.c:106-231, :428-522, :696-785.  NULL arguments take the defaults: samplate 32000 (accepted 1 ... 196000),
 * lowFre 32 (values below 27 are ignored), highFre 2000 -- a value outside (lowFre, samplate / 2), samplate / 2 by integer
 * division, resets BOTH to 32 / 2000 --, cutFre 4000 (a value below highFre becomes highFre), radix2Exp 12, slideLength
 * fftLength / 4 (any positive value, also > fftLength), windowType Hamm (any type), alpha 10 (> 0), beta 0.5 (> 0),
 * gamma 1.8 (> 1), isContinue 0.  Returns 0, -100 / -6 (see above) or a device status (afx_last_error()). */
int pitchPEFObj_new(PitchPEFObj *pitchPEFObj,
				int *samplate,float *lowFre,float *highFre,float *cutFre,
				int *radix2Exp,int *slideLength,WindowType *windowType,
				float *alpha,float *beta,float *gamma,
				int *isContinue);

/* _pitch_pef.c:658-683: frames of a call with dataLength samples; with isContinue the kept tail counts */
int pitchPEFObj_calTimeLength(PitchPEFObj pitchPEFObj,int dataLength);
/* _pitch_pef.c:685-694: arguments that are not (alpha > 0, beta > 0, gamma > 1) are ignored; valid ones are, too -- see the
 * deviations: the filter stays the constructor's */
void pitchPEFObj_setFilterParams(PitchPEFObj pitchPEFObj,float alpha,float beta,float gamma);

/* _pitch_pef.c:233-426.  Per frame i at i * slideLength: window, power spectrum pw[0 ... N] of the frame zero-padded to 2N
 * points, y[m] = pw[j] + (lg[m] - lin[j]) * (pw[j + 1] - pw[j]) / (lin[j + 1] - lin[j]) on the log grid, times the band
 * width, R[k] = sum_n h[n] B[n + k] with B[filterPadNum + m] = y[m], index = first argmax of R over minIndex ... maxIndex
 * (an all-zero frame gives minIndex), freArr[i] = lg[index].  With isContinue the samples a call leaves unused (or, with a
 * hop above fftLength, the number still to skip) carry over to the next call (:524-656).  A failure is recorded on the
 * calling thread (afx_error_count()). */
void pitchPEFObj_pitch(PitchPEFObj pitchPEFObj,float *dataArr,int dataLength,
					float *freArr);

/* _pitch_pef.c:787-790 */
void pitchPEFObj_enableDebug(PitchPEFObj pitchPEFObj,int isDebug);
/* _pitch_pef.c:792-826 */
void pitchPEFObj_free(PitchPEFObj pitchPEFObj);

/* ---- additive: clips that already live in HBM ---------------------------------------------------------------------------
 * `batch` clips of dataLength samples, clip b at dData + b * clipStride (clipStride >= dataLength), frames =
 * (dataLength - fftLength) / slideLength + 1 each.  dFre / dValue [b * outStride + t], outStride >= frames: the frequency
 * and R at the chosen index (dValue may be NULL); every frame is written, nothing else.  One launch, asynchronous on
 * hipStream.  Returns 0; -4 for an object created with isContinue (it carries one signal's tail); -6 for NULL /
 * non-positive / short-stride arguments; 0 without writing anything when dataLength < fftLength. */
int pitchPEFObj_pitchBatchDevice(PitchPEFObj pitchPEFObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dFre, float *dValue, long long outStride, void *hipStream);
/* the lags the reference keeps at the head of each mXcorrArr row: dCurve[(b * frames + t) * (maxIndex + 1) + k],
 * k = 0 ... maxIndex (the entries below minIndex included) */
int pitchPEFObj_curveBatchDevice(PitchPEFObj pitchPEFObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dCurve, void *hipStream);
int pitchPEFObj_minIndex(PitchPEFObj pitchPEFObj);
int pitchPEFObj_maxIndex(PitchPEFObj pitchPEFObj);
int pitchPEFObj_filterPadNum(PitchPEFObj pitchPEFObj);
int pitchPEFObj_logLength(PitchPEFObj pitchPEFObj); /* 2N: entries of the log-frequency grid */

/* what pitchPEFObj_new decides, without a device */
typedef struct {
    int samplate, radix2Exp, fftLength, slideLength, isContinue;
    int windowType;
    float lowFre, highFre, cutFre, alpha, beta, gamma;
    int minIndex, maxIndex;
    int filterPadNum;    /* P = #{q[i] < 1}: zeros in front of the log spectrum */
    int logLength;       /* 2N */
    int refXcorrLength;  /* the reference's transform length: 8N with P > 0, else 4N */
    int corrLength;      /* the real correlation length the kernel uses: 4N */
    int pwLength;        /* bins 0 ... pwLength - 1 of the power spectrum are read by the log grid (<= N + 1) */
    long long ldsBytes;  /* LDS one workgroup declares */
    float *lg;           /* [2N] log frequencies: logFreBandArr    -- the four tables are the plan's own copies, */
    float *bw;           /* [2N] band widths: bandWidthArr            bit for bit the reference's; NULL after -100 */
    float *h;            /* [N] filter: filterArr[0 ... N - 1] */
    float *window;       /* [N]: winDataArr */
} AfxPitchPefPlan;
/* Fills *plan and returns the constructor's status: 0, -100, -6 (plan then holds what was decided, tables included for -6).
 * afx_pitch_pef_plan_free releases the tables of any plan this call filled. */
int afx_pitch_pef_plan_host(int *samplate, float *lowFre, float *highFre, float *cutFre, int *radix2Exp, int *slideLength,
                            WindowType *windowType, float *alpha, float *beta, float *gamma, int *isContinue,
                            AfxPitchPefPlan *plan);
void afx_pitch_pef_plan_free(AfxPitchPefPlan *plan);

#ifdef __cplusplus
}
#endif

#endif
