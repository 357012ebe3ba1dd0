/* st_algorithm.h -- C ABI of the S-transform object: one FFT X of the whole N = 2^radix2Exp chunk and, per requested bin k,
 * an N-point inverse transform of the spectrum rotated by k under a Gaussian window whose width follows k:
 *   c_k    = -factor 2 pi^2 / k^(2 norm)
 *   W_k[j] = exp(c_k j^2) + exp(c_k (j - N)^2),                      j = 0 ... N - 1
 *   row    = ifft_j( X[(k + j) mod N] W_k[j] )                       (with the 1 / N);   k = 0: the mean of the chunk
 *
 * Replaces the reference functions of the same names (src/st_algorithm.h, src/st_algorithm.c) as bound by
 * python/audioflux/st.py.  Execution: the forward pass of the CWT kernels for the spectrum, afx_st.hip for the rows -- the
 * window is evaluated in the kernel from c_k (the reference keeps an (N/2 + 1) x N float table: 537 MB at 2^14).
 * Three deliberate divergences:
 *   1. the row of bin 0 writes the imaginary plane too (zeros): a device call writes every documented word.  The reference
 *      leaves that row of mImageArr untouched; both Python wrappers pre-zero the planes, so it does not show there;
 *   2. stObj_useBinArr with length <= 0 or length > N is refused: a failure is counted (afx_error_count, sticky error text)
 *      and the bins stay as they were -- the reference copies `length` ints into its N-int buffer;
 *   3. radix2Exp outside 4 ... 14 is refused with -4: the forward pass starts at 2^4 points, and the transform buffer of a
 *      2^15-point row does not fit the LDS of a CU.
 * The fall-back of stObj_new to the full range 0 ... N/2 is reproduced as it is: stObj_getBinLength tells.
 */
#ifndef ST_ALGORITHM_H
#define ST_ALGORITHM_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueST *STObj;

/* (st_algorithm.c: stObj_new) chunks of 2^radix2Exp samples, radix2Exp 4 ... 14; rows of the bins minIndex ... maxIndex.
 * factor / norm NULL or <= 0 are taken as 1; minIndex >= maxIndex, minIndex < 0 or maxIndex > N/2 is taken as 0 ... N/2.
 * Returns 0, -4 for radix2Exp outside 4 ... 14 (divergence 3), -2 without a usable gfx950 device, <= -2 backend failure.
 * *stObj is NULL unless 0 is returned. */
int stObj_new(STObj *stObj,int radix2Exp,int minIndex,int maxIndex,float *factor,float *norm);

/* (st_algorithm.c: stObj_useBinArr) the rows from now on: binArr[0 ... length - 1], any order, repeats allowed.  Taken only
 * if every entry lies in 0 ... N/2, otherwise ignored silently, as the reference does; length outside 1 ... N: divergence 2 */
void stObj_useBinArr(STObj stObj,int *binArr,int length);
/* (st_algorithm.c: stObj_setValue) a new window, the values used as given (no "<= 0 is 1" here); nothing happens when both
 * are the current ones.  Calls already queued on a stream finish with the old values. */
void stObj_setValue(STObj stObj,float factor,float norm);

/* (st_algorithm.c: stObj_st) dataArr[N] -> mRealArr / mImageArr [binLength][N], host pointers, synchronous.  The spectrum is
 * computed once; the rows reach the host in passes of row blocks through a device staging buffer of at most 2^22 floats
 * (16 MB) per plane: 1024 rows a pass at radix2Exp 12, 256 at 14. */
void stObj_st(STObj stObj,float *dataArr,float *mRealArr,float *mImageArr);

/* (st_algorithm.c: stObj_free) NULL-safe */
void stObj_free(STObj stObj);

/* ---- additive ------------------------------------------------------------------------------------------------------- */
/* rows that the next stObj_st / stObj_stBatchDevice writes; 0 for a NULL object */
int stObj_getBinLength(STObj stObj);

/* Chunks that already live in HBM.  Chunk c = 2^radix2Exp samples at x + c * xStride -> outRe / outIm
 * [chunks][binLength][N].  All pointers are device pointers of any 4-byte alignment; every element of both outputs is
 * written, nothing else; of each chunk only [c * xStride, c * xStride + N) is read; asynchronous on `stream` (a HIP
 * stream, NULL: the default stream).  Spectra go through the object's scratch, large batches in passes.  AFX_ERR_ARG (-6):
 * NULL object / x / either plane, chunks <= 0, xStride < 2^radix2Exp, a stream of another device than the object's. */
int stObj_stBatchDevice(STObj stObj, const float *x, int chunks, long long xStride, float *outRe, float *outIm,
                        void *stream);

/* The window coefficients stObj_new / stObj_setValue would upload, on the host and WITHOUT a device: coef[N/2 + 1],
 * entry k = c_k by the reference's own expression (a double expression around powf(k, 2 norm), stored to float), entry 0
 * is 0.  factor and norm are used as given.  Returns 0, or -1 for radix2Exp outside 1 ... 24 or a NULL array. */
int afx_st_plan_host(int radix2Exp, float factor, float norm, float *coef);

#ifdef __cplusplus
}
#endif
#endif /* ST_ALGORITHM_H */
