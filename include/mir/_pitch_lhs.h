/* _pitch_lhs.h -- C ABI of the log-harmonic-sum pitch tracker: mir/_pitch_hps.h with a sum of logarithms in place of the
 * product, curve[j] = log|X[j]| + log|X[2j]| + ... + log|X[harmonicCount j]|.
 *
 * Replaces the reference functions of the same names (src/mir/_pitch_lhs.h, src/mir/_pitch_lhs.c:81-559) as bound by
 * python/audioflux/mir/pitch_lhs.py.  One kernel launch per call (csrc/hip/afx_pitch_hs.hip); the reference's two
 * [timeLength, M] planes (mDbArr, mSumArr) do not exist.
 *
 * Where the reference's LHS constructor differs from its HPS constructor, this object follows LHS:
 *  - windowType is taken as given (_pitch_lhs.c:142-144): every WindowType of flux_base.h builds its window, a value
 *    outside the enumeration gives the rectangular one (window_calFFTWindow's last branch); there is no fallback to Hamm.
 *  - the window multiply is unconditional (:459); for Window_Rect it multiplies by ones.
 *  - harmonicCount IS clamped to samplate / (maxIndex + 1) by integer division, at least 1 (:244-257).
 *
 * Deviations from the reference: those of mir/_pitch_hps.h --
 *  - radix2Exp outside 6 ... 13 returns -100 and a NULL handle;
 *  - fftLength > M returns -6 and a NULL handle (_pitch_lhs.c:455-458 overruns its frame buffer);
 *  - maxIndex * harmonicCount >= M (after the clamp) returns -6 and a NULL handle (:496-500 reads past the spectrum;
 *    reachable when M < samplate: 44100 Hz, highFre 8000, 5 harmonics);
 *  - float32 transforms of another factorisation: near a spectral null the logarithm amplifies the difference, which
 *    tests/pitch_hs_check.py prices per curve entry;
 *  - pitchLHSObj_enableDebug prints the parameters only, and only when isDebug is non-zero (the reference stores 1
 *    whatever it is given);
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef _PITCH_LHS_H
#define _PITCH_LHS_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>

#include "../flux_base.h"
#include "_pitch_hps.h"

typedef struct OpaquePitchHS *PitchLHSObj;

/* _pitch_lhs.c:81-183, :212-266.  Defaults and clamps as pitchHPSObj_new but for the three differences above. */
int pitchLHSObj_new(PitchLHSObj *pitchLHSObj,
				int *samplate,float *lowFre,float *highFre,
				int *radix2Exp,int *slideLength,WindowType *windowType,
				int *harmonicCount,
				int *isContinue);

/* _pitch_lhs.c:185-210 */
int pitchLHSObj_calTimeLength(PitchLHSObj pitchLHSObj,int dataLength);

/* _pitch_lhs.c:391-532.  Per frame: window, logf(sqrtf(re^2 + im^2)) of the M-point transform of the zero-padded frame,
 * curve[j] = sum_{k < harmonicCount} log|X[j (k + 1)]| in float32 in that order, index = first argmax over minIndex ...
 * maxIndex -- an all-zero frame has -inf everywhere and gives minIndex, as __vmax never replaces its first element --,
 * freArr[i] = (index + 1) * (1.0 * samplate / M).  Streaming as pitchHPSObj_pitch (:268-389). */
void pitchLHSObj_pitch(PitchLHSObj pitchLHSObj,float *dataArr,int dataLength,
					float *freArr);

/* _pitch_lhs.c:534-537 */
void pitchLHSObj_enableDebug(PitchLHSObj pitchLHSObj,int isDebug);
/* _pitch_lhs.c:539-559 */
void pitchLHSObj_free(PitchLHSObj pitchLHSObj);

/* ---- additive: see pitchHPSObj_pitchBatchDevice / _curveBatchDevice (the curve is the reference's mSumArr) ---------- */
int pitchLHSObj_pitchBatchDevice(PitchLHSObj pitchLHSObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dFre, float *dValue, long long outStride, void *hipStream);
int pitchLHSObj_curveBatchDevice(PitchLHSObj pitchLHSObj, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dCurve, void *hipStream);
int pitchLHSObj_minIndex(PitchLHSObj pitchLHSObj);
int pitchLHSObj_maxIndex(PitchLHSObj pitchLHSObj);
int pitchLHSObj_harmonicCount(PitchLHSObj pitchLHSObj); /* after the clamp */
int pitchLHSObj_interpLength(PitchLHSObj pitchLHSObj);

#ifdef __cplusplus
}
#endif

#endif
