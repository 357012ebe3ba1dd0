/* onset_algorithm.h -- C ABI of the onset detector: an optional max filter along frequency over the spectrogram rows, one
 * of eleven novelty functions over the frames, the normalisation (v - min) / max of the curve, and the peak picker.
 *
 * Replaces the reference functions of the same names (src/mir/onset_algorithm.h:13-62, src/mir/onset_algorithm.c:58-460)
 * as bound by python/audioflux/mir/onset.py.  The novelty is the descriptor kernels' (csrc/hip/afx_descriptors.hip, the
 * arithmetic of spectralObj_computeDevice with framesPerClip = nLength); the filter, the normalisation and the picker are
 * csrc/hip/afx_onset.hip.  The batched device-pointer calls are declared at the end of this header.
 *
 * Deviations from the reference, all on inputs where it reads or writes out of bounds or reads memory it never wrote:
 *  - onsetObj_new returns AFX_ERR_ARG (-6) for nLength < 1 or mLength < 1 (onset_algorithm.c:96-97 allocates
 *    nLength * mLength floats unchecked) and a backend status <= -2 without a device; the reference always returns 0.
 *  - onsetObj_onset returns a negative status instead of a point count, and writes nothing, for
 *      a phase kind (PD, WPD, NWPD, CD, RCD) without mDataArr2       (flux_spectral.c:557-700 dereference it),
 *      step > nLength                                                 (onset_algorithm.c:316: the memset of `step` floats runs
 *                                                                      past evnArr[nLength]),
 *      an index outside 0 ... mLength - 1, or indexLength < 1 with an index array
 *                                                                     (flux_spectral.c:76: the row is read at that index).
 *  - the envelope never depends on what evnArr held: where the reference leaves entries as it found them (frame 1 of the
 *    phase-deviation kinds at step 1, flux_spectral.c:563-564) or counts onto them (broadband, :716), the result is that of
 *    a zeroed evnArr.
 *  - NaN / Inf rows: unspecified values, no fault.
 * Kept as they are: `type` is taken unchecked and any value that is not a named kind runs flux (onset_algorithm.c:372);
 * isNorm and gamma are accepted and unused; the minimum of the curve is taken over all nLength entries, the leading
 * zeros of the difference kinds included (:379); the products of the pick parameters are evaluated in double and floored
 * as float (:125-131).
 */
#ifndef ONSET_ALGORITHM_H
#define ONSET_ALGORITHM_H

#ifdef __cplusplus
extern "C" {
#endif

/* the values are ABI (onset_algorithm.h:13-30) */
typedef enum {
    Novelty_Flux = 0,

    Novelty_HFC,
    Novelty_SD,
    Novelty_SF,
    Novelty_MKL,

    Novelty_PD,
    Novelty_WPD,
    Novelty_NWPD,

    Novelty_CD,
    Novelty_RCD,

    Novelty_Broadband,

} NoveltyType;

/* the layout is ABI (onset_algorithm.h:32-44) */
typedef struct {
    int step;        /* flux, sd, sf: frame distance, <= 0 -> 1 */
    float p;         /* flux: exponent, 0 -> 1                  */
    int isPostive;   /* flux, sd, sf: rectify (else the absolute value) */
    int isExp;       /* flux: p-th root of the sum              */
    int type;        /* flux, mkl: 0 sum, 1 mean                */

    float threshold; /* broadband, in dB                        */

    int isNorm;      /* unused */
    float gamma;     /* unused */

} NoveltyParam;

typedef struct OpaqueOnset *OnsetObj;

/* nLength frames of mLength bins.  slideLength < 1 -> 512; samplate NULL or <= 0 -> 32000; filterOrder NULL or <= 0 -> 1
 * (orders >= 2 filter, any size); type NULL -> flux.  Pick parameters from samplate / slideLength: afx_onset_plan_host
 * (afx_batch.h).  returns 0, -6 bad lengths, <= -2 backend failure.  replaces onset_algorithm.c:58-133 */
int onsetObj_new(OnsetObj *onsetObj, int nLength, int mLength, int slideLength, int *samplate, int *filterOrder,
                 NoveltyType *type);

/* mDataArr1 [nLength, mLength] (and mDataArr2, the phase, for the phase kinds) -> evnArr[nLength], the normalised novelty
 * curve, and pointArr[<= nLength], the picked frames in ascending order; returns their number.  param NULL -> step 1, p 1,
 * isPostive 1, isExp 0, type 0, threshold 0; indexArr NULL -> bins 0 ... mLength - 1, else indexLength bins in any order,
 * repeats allowed.  Host pointers.  Negative: a refusal listed above (-6) or a backend failure.
 * replaces onset_algorithm.c:135-386, :423-460 */
int onsetObj_onset(OnsetObj onsetObj, float *mDataArr1, float *mDataArr2, NoveltyParam *param, int *indexArr, int indexLength,
                   float *evnArr, int *pointArr);

/* replaces onset_algorithm.c:388-403 */
void onsetObj_free(OnsetObj onsetObj);
/* the reference's three lines (onset_algorithm.c:405-415) */
void onsetObj_debug(OnsetObj onsetObj);

/* ---- additive: rows that already live in HBM (device pointers as in afx_batch.h: plain HBM addresses, hipStream a
 * hipStream_t used as given, NULL the default stream; every call asynchronous on it) ---------------------------------------
 * batch clips of nLength rows of mLength floats back to back at dSpec (and dPhase, the phase kinds only) -> the normalised
 * novelty curve dEvn[b * outStride + t], t < nLength, the picked frames dPoint[b * pointStride + k] in ascending order and
 * dCount[b], the number of ALL points of the clip: entries beyond min(dCount[b], pointStride) are not written.  dPoint and
 * dCount may be NULL (both: the envelope alone).  param, indexArr: HOST pointers with the meaning and defaults of
 * onsetObj_onset; the index table is uploaded only when it differs from the previous call's.  Same as calling
 * onsetObj_onset per clip, bit for bit (HFC alone, on rows of a multiple of 4 bins from a base that is not 16-byte aligned:
 * to the parity bar, the rule of spectralObj_computeDevice in afx_batch.h).  Asynchronous on hipStream, no hidden
 * synchronisation and no host round trip in the
 * steady state.  Scratch: one float per frame, plus the filtered copy of the rows when the object filters (order >= 2) --
 * large batches then run in chunks of whole clips so that it stays bounded (AFX_ONSET_CHUNK_MB, default 1024); it grows on
 * the first call that needs it and is reused.  AFX_ERR_ARG (-6): NULL object / dSpec / dEvn, batch <= 0, outStride < nLength,
 * pointStride < 0, and the refusals of onsetObj_onset (a phase kind without dPhase, step > nLength, an index outside
 * 0 ... mLength - 1). */
int onsetObj_onsetBatchDevice(OnsetObj onsetObj, const float *dSpec, const float *dPhase, int batch, const NoveltyParam *param,
                              const int *indexArr, int indexLength, float *dEvn, int *dPoint, int *dCount, long long outStride,
                              long long pointStride, void *hipStream);
/* the primitive of the filter: dOut[r, j] = max of dIn[r, max(j - order / 2, 0) ... min(j - 1 + order - order / 2, cols - 1)]
 * over resident dIn [rows, cols] (flux_vector.c:3063-3081: the window of an even order leans to the left); order >= 1, any
 * size.  Exact.  In place is not allowed.  AFX_ERR_ARG: bad pointers / sizes / order < 1. */
int afx_maxFilterDevice(const float *dIn, long long rows, int cols, int order, float *dOut, void *hipStream);
/* the picker (onset_algorithm.c:423-460) on any resident envelopes dEvn[b * stride + t], t < length, with any parameters:
 * frame i is a point when e[i] == max e[max(i - preMax, 0) ... (i + postMax < length ? i - 1 + postMax : length - 1)],
 * e[i] >= mean e[max(i - preAvg, 0) ... (i + postAvg < length ? i - 1 + postAvg : length - 1)] + delta (the mean a float32 sum
 * in index order divided by the count) and i - previous point > wait.  dPoint / dCount as above (one of them may be NULL).
 * AFX_ERR_ARG: preMax, preAvg or wait < 0, postMax or postAvg < 1 (the reference's windows would be empty: it compares
 * with the previous frame's maximum), bad pointers / sizes. */
int afx_peakPickDevice(const float *dEvn, int batch, int length, long long stride, int preMax, int postMax, int preAvg,
                       int postAvg, int wait, float delta, int *dPoint, int *dCount, long long pointStride, void *hipStream);
/* util_powerToDB (afx_batch.h) on resident clips dIn[b * stride + i], i < length -> dOut[b * stride + i], ONE maximum per clip, as a loop of
 * util_powerToDB calls would take; dOut == dIn allowed.  Asynchronous on hipStream. */
int afx_powerToDbDevice(const float *dIn, int batch, long long length, long long stride, float min, float *dOut,
                        void *hipStream);

#ifdef __cplusplus
}
#endif
#endif /* ONSET_ALGORITHM_H */
