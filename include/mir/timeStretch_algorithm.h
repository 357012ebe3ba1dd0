/* timeStretch_algorithm.h -- C ABI of the time-stretch object: an STFT without padding, the phase vocoder (output frame i
 * at t = i * rate between input frames floor(t) and floor(t) + 1: interpolated magnitudes, accumulated wrapped phase
 * differences), and the weighted-overlap-add inverse STFT.
 *
 * Replaces the reference functions of the same names (src/mir/timeStretch_algorithm.h, src/mir/timeStretch_algorithm.c:34-164,
 * src/dsp/phase_vocoder.c:19-120) as bound by python/audioflux/mir/time_stretch.py.  The transforms are the STFT object's
 * kernels; the vocoder is csrc/hip/afx_phasevocoder.hip, in the reference's float32 operation order: the phase accumulator
 * is ill-conditioned by construction, two correct float32 implementations sit 1e-4 ... 3e-3 apart, so parity is
 * judged against bars measured from the reference alone.  There is no CPU compute path.
 *
 * Deviations from the reference, all where its code faults, writes out of bounds or depends on the caller's zeros:
 *  - the destination is OVERWRITTEN.  The reference accumulates the inverse transform onto dataArr2 and its wrapper passes
 *    zeros.  timeStretchObj_timeStretch writes the (T2 - 1) * slideLength + fftLength samples of the inverse transform and
 *    nothing behind them; the device call writes exactly the returned length.
 *  - rate <= 0 or not finite, dataLength < fftLength (no frame) and NULL arguments return 0 or a negative status, which is
 *    recorded (afx_error_count()); nothing is written.  The reference divides by zero or reads a zero-length allocation.
 *  - radix2Exp above 14 (the STFT backend's limit) and slideLength above fftLength (samples no frame covers) make the
 *    constructor return -4 and a NULL handle.
 *  - NaN / Inf samples: unspecified values, no fault.
 */
#ifndef TIMESTRETCH_ALGORITHM_H
#define TIMESTRETCH_ALGORITHM_H

#include "../flux_base.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueTimeStretch *TimeStretchObj;

/* radix2Exp NULL or outside 1 ... 30 -> 12; slideLength NULL or <= 0 -> fftLength / 4; windowType NULL -> Hann.
 * Returns 0, -4 (see above), -5 or a device status (afx_last_error()).  replaces timeStretch_algorithm.c:34-75 */
int timeStretchObj_new(TimeStretchObj *timeStretchObj,int *radix2Exp,int *slideLength,WindowType *windowType);

/* ceilf(dataLength / rate) + fftLength in float32: the samples a destination of the host-pointer call must hold.  0 for a
 * NULL handle or a rate that is refused.  replaces timeStretch_algorithm.c:77-80 */
int timeStretchObj_calDataCapacity(TimeStretchObj timeStretchObj,float rate,int dataLength);

/* dataArr1[dataLength] -> dataArr2[(T2 - 1) * slideLength + fftLength], T1 = (dataLength - fftLength) / slideLength + 1,
 * T2 = ceilf(T1 / rate).  Returns roundf(dataLength / rate), the length the stretched signal counts as; 0 or a negative
 * status when nothing was written.  Host pointers.  replaces timeStretch_algorithm.c:82-149 */
int timeStretchObj_timeStretch(TimeStretchObj timeStretchObj,float rate,float *dataArr1,int dataLength,float *dataArr2);

/* replaces timeStretch_algorithm.c:151-164 */
void timeStretchObj_free(TimeStretchObj timeStretchObj);

/* ---- additive: clips that already live in HBM (the contract at the top of afx_batch.h) ---------------------------------
 * `batch` clips of dataLength samples at dData + b * clipStride -> dOut[b * outStride + i], i < the returned length
 * = roundf(dataLength / rate); exactly these words are written: the inverse transform's samples, then zeros.  The words
 * both calls write are bit for bit those of timeStretchObj_timeStretch.  Asynchronous on hipStream; the batch is worked
 * through in chunks of whole clips whose scratch stays under the object's limit.  -6 for NULL / non-positive / short-stride
 * arguments, a refused rate or a clip that holds no frame. */
int timeStretchObj_timeStretchBatchDevice(TimeStretchObj timeStretchObj, float rate, const float *dData, int batch, int dataLength,
                                          long long clipStride, float *dOut, long long outStride, void *hipStream);
/* the vocoder alone on resident half- or full-spectra: re/im [batch * T1, pitch] (pitch >= N / 2 + 1, bins 0 ... N / 2 are
 * read) -> re/im [batch * T2, N], T2 = ceilf(T1 / rate), every word written.  The call owns no object to keep scratch in: it
 * allocates 2 batch T1 (N / 2 + 1) floats, waits for hipStream and frees them.  -6 for NULL / out-of-range arguments. */
int afx_phase_vocoder_device(const float *dRe, const float *dIm, int batch, int T1, int radix2Exp, long long pitch, int hop,
                             float rate, float *dRe2, float *dIm2, void *hipStream);

/* grow-only device scratch the batched call may hold, in bytes; at least one clip is always taken.  The default is
 * AFX_TIMESTRETCH_SCRATCH_BYTES, chosen for memory: 4 GiB, 1.4 % of an MI355X.  One clip of 30 s at 44.1 kHz / 4096 / 1024 needs
 * 59 ... 81 MB, so a chunk holds 53 ... 72 of them; the phase kernel runs one lane per (clip, bin) and wants many clips in a
 * launch: 1000 such clips at rate 0.8 take 102 / 90 / 81 ms at 1 / 4 / 16 GiB (profiles/timestretch_mi355x.txt). */
#define AFX_TIMESTRETCH_SCRATCH_BYTES (4ll << 30)
void timeStretchObj_setScratchLimit(TimeStretchObj timeStretchObj, long long bytes);

/* what a call decides, without a device */
typedef struct {
    int fftLength, slideLength;
    int T1, T2;                 /* input and output frames per clip                                                      */
    int istftLength;            /* (T2 - 1) slideLength + fftLength                                                      */
    int returnLength, capacity; /* roundf(dataLength / rate), ceilf(dataLength / rate) + fftLength                       */
    long long scratchBytes;     /* device scratch of one clip: half spectrum, output spectrum, inverse transform         */
    int clipsPerChunk;          /* clips of one chunk of a batch under the scratch limit                                 */
} AfxTimeStretchPlan;
/* status 0; -4 for sizes the constructor refuses; -6 for a rate or a length a call refuses (the plan then holds what was
 * decided before the refusal).  scratchLimit <= 0: the default.  kArr / alphaArr: NULL, or [T2] arrays that receive the
 * input frame and the weight of every output frame. */
int afx_timestretch_plan(int radix2Exp, int slideLength, float rate, int dataLength, int batch, long long scratchLimit,
                         AfxTimeStretchPlan *plan, int *kArr, float *alphaArr);

#ifdef __cplusplus
}
#endif
#endif /* TIMESTRETCH_ALGORITHM_H */
