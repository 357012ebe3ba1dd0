/* resample_algorithm.h -- C ABI of the band-limited resampler: output i of a signal is the sum of the samples around
 * n = floor(i / ratio), ratio = targetRate / sourceRate, weighted by a windowed-sinc table of zeroNum zero crossings with
 * 2^nbit entries each, read every floor(min(1, ratio) 2^nbit) entries and interpolated linearly between neighbours.
 *
 * Replaces the reference functions of the same names (src/dsp/resample_algorithm.h, src/dsp/resample_algorithm.c:59-658)
 * as bound by python/audioflux/dsp/resample.py.  The table is built on the host in the reference's float32 operation
 * order; every output of every clip is computed in ONE kernel launch (csrc/hip/afx_resample.hip) that keeps the table in
 * LDS (Best / Mid / Fast: 128 / 64 / 32 KB) and forms the difference table from neighbouring entries.  There is no CPU
 * compute path.
 *
 * Deviations from the reference:
 *  - the destination is OVERWRITTEN.  The reference accumulates into dataArr2 (:498, :514) and its wrapper always passes
 *    zeros; here dataArr2 needs no initialisation, and only the returned number of values is written.
 *  - a table above 2^24 entries (zeroNum 2^nbit; 64 MB of device memory, a cap chosen for memory) makes the constructor
 *    return -4 and a NULL handle.  Tables up to 160 KB are kept in LDS by the kernel, larger ones are read from global
 *    memory by the same kernel.
 *  - with isContinue and q <= 1 (an integer up-sampling ratio such as 16000 -> 32000, or any ratio given through
 *    resampleObj_setSamplateRatio, which sets p = q = 0) the reference leaves the lengths of the PREVIOUS call in place
 *    (:239-244).  Here resampleObj_calDataLength and resampleObj_resample return 0 and write nothing.
 *  - the remainder of an isContinue call is dropped, as in the reference: it stores the up to q - 1 samples a call does
 *    not consume only when a remainder was already pending (:377: the merged buffer exists only then), and the object is
 *    born without one, so none is ever stored.  Pieces fed to an isContinue object give what the reference gives for the
 *    same pieces, not what one call over the whole signal gives.
 *  - where float32 rounding of dataLength * ratio gives one output more than samples cover, the reference reads past the
 *    end of dataArr1 (n = floor(i / ratio) >= dataLength); here such samples count as 0.
 *  - a ratio below 2^-nbit (no whole table entry per tap; the reference divides by zero) is refused: -6, recorded.
 *  - NULL handle or arrays, dataLength <= 0: resampleObj_resample returns -6 (and records it, afx_error_count()); the
 *    reference dereferences them.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef RESAMPLE_ALGORITHM_H
#define RESAMPLE_ALGORITHM_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdio.h>
#include <stdlib.h>
#include "../flux_base.h"

/* resample_algorithm.h:14-19 (only the band-limited algorithm exists, in the reference too) */
typedef enum{
	ResampleAlg_Polyphase=0, // stand

	ResampleAlg_Bandlimited, // ccrma

} ResampleAlgType;

/* resample_algorithm.h:21-26 */
typedef enum{
	ResampleQuality_Best=0,
	ResampleQuality_Mid,
	ResampleQuality_Fast,

} ResampleQualityType;

typedef struct OpaqueResample *ResampleObj;

/* resample_algorithm.c:59-97.  Kaiser tables: Best zeroNum 64, beta 14.7696565, rollOff 0.9475937; Mid 32, 11.6625806,
 * 0.8987969; Fast 16, 8.5555046, 0.85; nbit 9 for all.  NULL qualType: Best.  Returns 0, -4 / -5 or a device status
 * (afx_last_error()). */
int resampleObj_new(ResampleObj *resampleObj,ResampleQualityType *qualType,int *isScale,int *isContinue);
/* resample_algorithm.c:107-211, table :546-634.  NULL arguments and values outside their range take the defaults: zeroNum
 * 64 (> 0), nbit 9 (1 ... 29), winType Hann (types <= Rect, and values beyond the enum, become Hann), value 0 (>= 0; 0 becomes 5 for Kaiser and 2.5 for
 * Gauss, Tukey takes it as its alpha), rollOff 0.945 (0 < rollOff <= 1).  table[k] = rollOff sinc(rollOff k / 2^nbit) times
 * the right half of the symmetric window of 2 zeroNum 2^nbit + 1 points.  The object is born at 32000 -> 16000 (ratio 0.5, p 1,
 * q 2) with the table multiplied by 0.5. */
int resampleObj_newWithWindow(ResampleObj *resampleObj,
							int *zeroNum,int *nbit,
							WindowType *winType,float *value,
							float *rollOff,
							int *isScale,
							int *isContinue);

/* resample_algorithm.c:219-251.  Without isContinue floorf(dataLength * ratio) in float32; with it, for q > 1,
 * (dataLength - dataLength % q) p / q (q <= 1: 0, see above).  0 for a NULL handle or dataLength <= 0. */
int resampleObj_calDataLength(ResampleObj resampleObj,int dataLength);

/* resample_algorithm.c:253-301.  Equal or non-positive rates are ignored.  ratio = targetRate / (float)sourceRate, p / q its
 * lowest terms.  Where the ratio changes and the old or the new one is below 1 the table is divided by the old ratio (if
 * < 1), then multiplied by the new one (if < 1), entry by entry in float32, and uploaded again. */
void resampleObj_setSamplate(ResampleObj resampleObj,int sourceRate,int targetRate);
/* resample_algorithm.c:303-332: the same with the ratio given; negative values are ignored; p = q = 0 */
void resampleObj_setSamplateRatio(ResampleObj resampleObj,float ratio);
/* resample_algorithm.c:334-341: from the next call on the lengths follow the other rule */
void resampleObj_enableContinue(ResampleObj resampleObj,int flag);

/* resample_algorithm.c:350-521.  dataArr2[i], i < the returned length (resampleObj_calDataLength(dataLength1)), overwritten
 * with the resampled signal, divided by sqrtf(ratio) with isScale.  No filter state is carried from one call to the next, as
 * in the reference: the ends of every call see zeros.  Returns the length, or a negative status that is also recorded on
 * the calling thread (afx_error_count()). */
int resampleObj_resample(ResampleObj resampleObj,float *dataArr1,int dataLength1,float *dataArr2);

/* resample_algorithm.c:636-654 */
void resampleObj_free(ResampleObj resampleObj);
/* resample_algorithm.c:656-658: prints the parameters (the reference prints nothing) */
void resampleObj_debug(ResampleObj resampleObj);

/* ---- additive: clips that already live in HBM ---------------------------------------------------------------------------
 * `batch` clips of dataLength samples, clip b at dData + b * clipStride (clipStride >= dataLength), each resampled on its
 * own into dOut[b * outStride + i], i < the returned length = floorf(dataLength * ratio); outStride >= that length.  Exactly
 * these values are written, bit for bit what resampleObj_resample gives for the clip.  One launch, asynchronous on
 * hipStream.  Returns the length per clip (0: nothing to do, nothing written); -4 for an object with isContinue (it belongs
 * to one signal); -6 for NULL / non-positive / short-stride arguments. */
int resampleObj_resampleBatchDevice(ResampleObj resampleObj, const float *dData, int batch, int dataLength, long long clipStride,
                                    float *dOut, long long outStride, void *hipStream);

/* what the constructors and the rate setters decide, without a device */
typedef struct {
    int zeroNum, nbit, bitLength, interpLength;
    int winType;
    float value, rollOff;
    int isScale, isContinue;
    float ratio;
    int p, q, sourceRate, targetRate;
    int step, taps;           /* floorf(min(1, ratio) bitLength); taps per side at most                               */
    int tableInLds, group;    /* the launch of a batch of 4 or more clips: table in LDS, clips per work item          */
    long long ldsBytes;       /* LDS one workgroup of that launch declares                                            */
    float *table;             /* [interpLength]: interpArr as it stands (times ratio when that is < 1); the plan's own copy */
} AfxResamplePlan;
/* The plan of resampleObj_newWithWindow with the same arguments (status 0, -4, -5); qualType non-NULL: of resampleObj_new,
 * the window arguments are then not read.  afx_resample_plan_free releases the table. */
int afx_resample_plan_host(ResampleQualityType *qualType, int *zeroNum, int *nbit, WindowType *winType, float *value, float *rollOff,
                           int *isScale, int *isContinue, AfxResamplePlan *plan);
/* resampleObj_setSamplate (targetRate > 0) or resampleObj_setSamplateRatio(ratio) (sourceRate = targetRate = 0) on a plan */
int afx_resample_plan_rate(AfxResamplePlan *plan, int sourceRate, int targetRate, float ratio);
/* resampleObj_calDataLength on a plan: needs no object and no earlier call */
int afx_resample_plan_length(const AfxResamplePlan *plan, int dataLength);
void afx_resample_plan_free(AfxResamplePlan *plan);

#ifdef __cplusplus
}
#endif

#endif
