/* fst_algorithm.h -- C ABI of the fast S-transform object: one FFT of the whole 2^radix2Exp chunk, per dyadic band of
 * the shifted spectrum an inverse transform of the band's own power-of-two length ("cells"), and a sample-and-hold of every
 * band's cells onto the N = 2^radix2Exp column grid.
 *
 * Replaces the reference functions of the same names (src/fst_algorithm.h, src/fst_algorithm.c) as bound by
 * python/audioflux/fst.py.  Execution: the forward pass of the CWT kernels for the spectrum, afx_fst.hip for the cells and the
 * expansion.  Row rule, the reference's, reproduced: index 0 shows bin -1, index 1 the DC bin, index 2 bin +1, indices
 * n + 1 ... 2n the band of n = 2, 4, ..., N/4 points (bins n ... 2n - 1); the negative bands are never shown and not computed.
 * Two deliberate divergences:
 *   1. fstObj_fst with minIndex > maxIndex (after clamping) writes nothing and counts a failure (afx_error_count, sticky
 *      error text) -- the reference then writes all N/2 + 1 rows into a buffer the caller sized for fewer;
 *   2. radix2Exp 15 and above is refused with -4 (the reference needs an (N/2 + 1) N int table: 8.6 GB at 16), and so is
 *      radix2Exp 3: the forward pass starts at 2^4 points.
 */
#ifndef FST_ALGORITHM_H
#define FST_ALGORITHM_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueFST *FSTObj;

/* chunks of 2^radix2Exp samples, radix2Exp 4 ... 14.  Returns 0, -1 for radix2Exp < 3 (as the reference), -4 for 3 and for
 * 15 and above, -2 without a usable gfx950 device, <= -2 backend failure.  *fstObj is NULL unless 0 is returned. */
int fstObj_new(FSTObj *fstObj, int radix2Exp);

/* dataArr[2^radix2Exp] -> mRealArr / mImageArr [maxIndex - minIndex + 1][2^radix2Exp], host pointers, synchronous.
 * minIndex < 0 is taken as 0, maxIndex > N/2 as N/2 (divergence 1 for what is left).  The cells are computed once; the
 * matrix reaches the host in passes of row blocks through a device staging buffer of at most 2^22 floats (16 MB) per
 * plane: 1024 rows a pass at radix2Exp 12, 256 at 14. */
void fstObj_fst(FSTObj fstObj, float *dataArr, int minIndex, int maxIndex, float *mRealArr, float *mImageArr);

/* NULL-safe */
void fstObj_free(FSTObj fstObj);

/* ---- additive ------------------------------------------------------------------------------------------------------- */
/* N/2 + 1: the visible cells of a chunk, in the order bin -1, DC, bin +1, band 2, band 4, ..., band N/4, each band in
 * time order (after the reference's final fftshift); 0 for a NULL object */
int fstObj_getCellLength(FSTObj fstObj);

/* Chunks that already live in HBM.  Chunk c = 2^radix2Exp samples at x + c * xStride -> outRe / outIm
 * [chunks][maxIndex - minIndex + 1][N] (both, or both NULL when the cells are given) and / or cellRe / cellIm
 * [chunks][N/2 + 1] (both or neither): the cells-only form skips the up to N/4-fold redundant matrix.  All pointers are
 * device pointers of any 4-byte alignment; every element of every requested output is written, nothing else; asynchronous
 * on `stream` (a HIP stream, NULL: the default stream).  Spectra and cells go through the object's scratch, large batches
 * in passes.  AFX_ERR_ARG (-6): NULL object / x, one pointer of a pair without the other, neither matrix nor cells,
 * chunks <= 0, xStride < 2^radix2Exp, indices outside 0 <= minIndex <= maxIndex <= N/2, a stream of another device than the
 * object's. */
int fstObj_fstBatchDevice(FSTObj fstObj, const float *x, int chunks, long long xStride, int minIndex, int maxIndex,
                          float *outRe, float *outIm, float *cellRe, float *cellIm, void *stream);

/* The plan fstObj_new would build, on the host and WITHOUT a device: rowCell / rowLen [2^radix2Exp / 2 + 1], the first
 * cell and the band length of index f (column l of its row holds cell rowCell[f] + l / (N / rowLen[f])); either may be
 * NULL.  Returns 0, or -1 for radix2Exp outside 3 ... 24. */
int afx_fst_plan_host(int radix2Exp, int *rowCell, int *rowLen);

#ifdef __cplusplus
}
#endif
#endif /* FST_ALGORITHM_H */
