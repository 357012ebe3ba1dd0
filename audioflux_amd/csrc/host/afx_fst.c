/* afx_fst.c -- the fast S-transform object (C host side) behind include/fst_algorithm.h.
 *
 * The reference (src/fst_algorithm.c) cuts the shifted spectrum into 2 r dyadic partitions, inverse-transforms each at its
 * own length and gathers the N x N matrix through an (N/2 + 1) x N int table.  Only the partitions of bin -1, DC, bin +1
 * and the positive bands of 2, 4, ..., N/4 points are ever shown (index f = 0, 1, 2 and n + 1 ... 2n: the reference's
 * off-by-one row rule, reproduced), so the plan is those N/2 + 1 "cells" and a row -> (first cell, band length) map.
 * Execution: afxk_nsgt_spectrum (afx_cwt.hip) + afxk_fst_cells + afxk_fst_expand (afx_fst.hip).
 *
 * Divergences from the reference, both deliberate: minIndex > maxIndex writes nothing and counts a failure
 * (the reference overruns the caller's buffer); radix2Exp 3 and 15 and above are refused (AFX_ERR_UNSUPPORTED).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objkit.h"
#include "fst_algorithm.h"

#define FST_STAGE_FLOATS (1ll << 22) /* per plane of the host entry's staging buffer (fst_algorithm.h) */

struct OpaqueFST {
    int radix2Exp, cellLength; /* N = 2^radix2Exp, N / 2 + 1 */
    AfxCwtPlanDims dims;
    float scale[16];
    void *stream;
    float *dTw, *dX, *dA, *dXt; /* forward twiddles, one chunk's samples / scratch / spectrum */
    int *dRowMap;               /* [N / 2 + 1][2]: first cell, column shift */
    float *dCell;               /* one chunk: [2][N / 2 + 1] */
    float *dStage;              /* [2][stage floats]: row blocks of the host entry */
    size_t capStage;
    float *dGA, *dGXt, *dGCell; /* scratch of the batched call: `pass` chunks at a time */
    size_t capGA, capGXt, capGCell;
    AfxScratchStream scratchStream;
    int status;
};

/* index f -> first cell and band length: 0, 1, 2 are the single bins -1, 0, +1 (cells 0, 1, 2); f in n + 1 ... 2n is the
 * band of n = 2, 4, ..., N/4 points, whose cells start at 3 + (2 + 4 + ... + n/2) = n + 1 */
static void row_of_index(int f, int *cell, int *len) {
    if (f < 3) {
        *cell = f;
        *len = 1;
        return;
    }
    int n = 2;
    while (2 * n < f) n *= 2;
    *cell = n + 1;
    *len = n;
}

int afx_fst_plan_host(int radix2Exp, int *rowCell, int *rowLen) {
    if (radix2Exp < 3 || radix2Exp > 24) return -1;
    const int half = 1 << (radix2Exp - 1);
    for (int f = 0; f <= half; f++) {
        int cell, len;
        row_of_index(f, &cell, &len);
        if (rowCell) rowCell[f] = cell;
        if (rowLen) rowLen[f] = len;
    }
    return 0;
}

int fstObj_new(FSTObj *fstObj, int radix2Exp) {
    if (!fstObj) return -1;
    *fstObj = NULL;
    if (radix2Exp < 3) return -1; /* fst_algorithm.c */
    if (radix2Exp < AFX_FST_MIN_EXP || radix2Exp > AFX_FST_MAX_EXP) {
        afxdev_set_error("fstObj_new: chunks of 2^%d samples are not supported (2^%d ... 2^%d)", radix2Exp, AFX_FST_MIN_EXP,
                         AFX_FST_MAX_EXP);
        return AFX_ERR_UNSUPPORTED;
    }
    FSTObj o = (FSTObj)calloc(1, sizeof(struct OpaqueFST));
    if (!o) return AFX_ERR_NOMEM;
    const size_t N = (size_t)1 << radix2Exp, cells = N / 2 + 1;
    o->radix2Exp = radix2Exp;
    o->cellLength = (int)cells;
    for (int b = 0; b <= radix2Exp - 2; b++) o->scale[b] = (float)(1.0 / sqrt((double)N * (double)(1 << b)));
    o->dims.r1 = radix2Exp / 2; /* the forward pass factors N = 2^r1 2^r2 (afx_nsgt.c) */
    o->dims.r2 = radix2Exp - radix2Exp / 2;
    o->dims.dataLength = (int)N;
    o->dims.pad = 0;
    int c = 8192 >> o->dims.r1;
    if (c > 16) c = 16;
    if (c > (1 << o->dims.r2)) c = 1 << o->dims.r2;
    o->dims.tileCols = c;
    int st = afxdev_ensure();
    float *tw = NULL;
    int *map = NULL;
    if (st == AFX_OK) {
        tw = afx_twiddle_table((int)N);
        map = (int *)malloc(sizeof(int) * 2 * cells);
        if (!tw || !map) st = AFX_ERR_NOMEM;
    }
    if (st == AFX_OK) {
        for (size_t f = 0; f < cells; f++) {
            int cell, len;
            row_of_index((int)f, &cell, &len);
            map[2 * f] = cell;
            map[2 * f + 1] = radix2Exp - afx_log2_exact(len);
        }
        st = afxdev_stream_create(&o->stream);
    }
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dTw, sizeof(float) * N);
    if (st == AFX_OK) st = afxdev_h2d(o->dTw, tw, sizeof(float) * N, o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dRowMap, sizeof(int) * 2 * cells);
    if (st == AFX_OK) st = afxdev_h2d(o->dRowMap, map, sizeof(int) * 2 * cells, o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dX, sizeof(float) * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dA, sizeof(float) * 2 * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dXt, sizeof(float) * 2 * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dCell, sizeof(float) * 2 * cells);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    free(tw);
    free(map);
    if (st != AFX_OK) {
        fstObj_free(o);
        return st;
    }
    *fstObj = o;
    return 0;
}

int fstObj_getCellLength(FSTObj o) { return o ? o->cellLength : 0; }

static int run_cells(FSTObj o, const float *Xt, int chunks, float *cellRe, float *cellIm, void *stream) {
    AfxFstCellArgs a;
    memset(&a, 0, sizeof(a));
    a.r1 = o->dims.r1;
    a.r2 = o->dims.r2;
    a.Xt = Xt;
    a.twiddle = o->dTw;
    a.chunks = chunks;
    memcpy(a.scale, o->scale, sizeof(a.scale));
    a.cellRe = cellRe;
    a.cellIm = cellIm;
    return afxk_fst_cells(&a, stream);
}

static int run_expand(FSTObj o, int minIndex, int rows, int chunks, const float *cellRe, const float *cellIm, float *outRe,
                      float *outIm, void *stream) {
    AfxFstExpandArgs a;
    memset(&a, 0, sizeof(a));
    a.radix2Exp = o->radix2Exp;
    a.minIndex = minIndex;
    a.rows = rows;
    a.chunks = chunks;
    a.rowMap = o->dRowMap;
    a.cellRe = cellRe;
    a.cellIm = cellIm;
    a.outRe = outRe;
    a.outIm = outIm;
    return afxk_fst_expand(&a, stream);
}

int fstObj_fstBatchDevice(FSTObj o, const float *x, int chunks, long long xStride, int minIndex, int maxIndex, float *outRe,
                          float *outIm, float *cellRe, float *cellIm, void *stream) {
    AFX_ENTER(o);
    if (!o || !x || (outRe == NULL) != (outIm == NULL) || (cellRe == NULL) != (cellIm == NULL) || (!outRe && !cellRe) ||
        chunks <= 0 || xStride < o->dims.dataLength || minIndex < 0 || minIndex > maxIndex ||
        maxIndex > o->dims.dataLength / 2) {
        afxdev_set_error("fstObj_fstBatchDevice: bad argument");
        return AFX_ERR_ARG;
    }
    if (stream) { /* the plan lives on the object's device */
        const int dev = afxdev_current_device();
        int st = afxdev_bind_stream(stream);
        if (st == AFX_OK && afxdev_current_device() != dev) {
            (void)afxdev_bind_stream(o->stream);
            afxdev_set_error("fstObj_fstBatchDevice: the stream belongs to another device than the object");
            st = AFX_ERR_ARG;
        }
        if (st != AFX_OK) return st;
    }
    const size_t N = (size_t)o->dims.dataLength, cells = (size_t)o->cellLength;
    const size_t rows = (size_t)(maxIndex - minIndex + 1);
    int st = afx_scratch_wait(&o->scratchStream, stream);
    /* spectra of a pass: at most 128 MB each for the scratch and the result, and a launch takes 65535 chunks */
    long long pass = (long long)((128u << 20) / (8 * N));
    if (pass > 65535) pass = 65535;
    if (pass > chunks) pass = chunks;
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dGA, &o->capGA, sizeof(float) * 2 * N * (size_t)pass);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dGXt, &o->capGXt, sizeof(float) * 2 * N * (size_t)pass);
    if (st == AFX_OK && !cellRe) st = afxdev_reserve((void **)&o->dGCell, &o->capGCell, sizeof(float) * 2 * cells * (size_t)pass);
    for (long long c = 0; c < chunks && st == AFX_OK; c += pass) {
        const int n = (int)(chunks - c < pass ? chunks - c : pass);
        float *cr = cellRe ? cellRe + (size_t)c * cells : o->dGCell;
        float *ci = cellIm ? cellIm + (size_t)c * cells : o->dGCell + cells * (size_t)pass;
        st = afxk_nsgt_spectrum(&o->dims, o->dTw, x + c * xStride, xStride, n, o->dGA, o->dGXt, stream);
        if (st == AFX_OK) st = run_cells(o, o->dGXt, n, cr, ci, stream);
        if (st == AFX_OK && outRe)
            st = run_expand(o, minIndex, (int)rows, n, cr, ci, outRe + (size_t)c * rows * N, outIm + (size_t)c * rows * N, stream);
    }
    afx_scratch_mark(&o->scratchStream, stream);
    if (st != AFX_OK) AFX_FAIL(o, st, "fstObj_fstBatchDevice");
    return st;
}

void fstObj_fst(FSTObj o, float *dataArr, int minIndex, int maxIndex, float *mRealArr, float *mImageArr) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("fstObj_fst: NULL object");
        return;
    }
    if (!dataArr || !mRealArr || !mImageArr) {
        afxdev_set_error("fstObj_fst: NULL array");
        AFX_FAIL(o, AFX_ERR_ARG, "fstObj_fst");
        return;
    }
    const size_t N = (size_t)o->dims.dataLength, cells = (size_t)o->cellLength;
    if (minIndex < 0) minIndex = 0; /* fst_algorithm.c */
    if (maxIndex > (int)(N / 2)) maxIndex = (int)(N / 2);
    if (minIndex > maxIndex) { /* divergence 1: the reference writes N/2 + 1 rows here */
        afxdev_set_error("fstObj_fst: minIndex %d is above maxIndex %d: nothing is written", minIndex, maxIndex);
        AFX_FAIL(o, AFX_ERR_ARG, "fstObj_fst");
        return;
    }
    const long long rows = (long long)maxIndex - minIndex + 1;
    long long block = FST_STAGE_FLOATS / (long long)N; /* rows of a pass */
    if (block > rows) block = rows;
    const size_t plane = (size_t)block * N;
    int st = afxdev_reserve((void **)&o->dStage, &o->capStage, sizeof(float) * 2 * plane);
    if (st == AFX_OK) st = afxdev_h2d(o->dX, dataArr, sizeof(float) * N, o->stream);
    if (st == AFX_OK) st = afxk_nsgt_spectrum(&o->dims, o->dTw, o->dX, (long long)N, 1, o->dA, o->dXt, o->stream);
    if (st == AFX_OK) st = run_cells(o, o->dXt, 1, o->dCell, o->dCell + cells, o->stream);
    for (long long k = 0; k < rows && st == AFX_OK; k += block) {
        const long long n = rows - k < block ? rows - k : block;
        st = run_expand(o, minIndex + (int)k, (int)n, 1, o->dCell, o->dCell + cells, o->dStage, o->dStage + plane, o->stream);
        if (st == AFX_OK) st = afxdev_d2h(mRealArr + (size_t)k * N, o->dStage, sizeof(float) * (size_t)n * N, o->stream);
        if (st == AFX_OK) st = afxdev_d2h(mImageArr + (size_t)k * N, o->dStage + plane, sizeof(float) * (size_t)n * N, o->stream);
    }
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) AFX_FAIL(o, st, "fstObj_fst");
}

void fstObj_free(FSTObj o) {
    if (!o) return;
    if (o->stream) {
        (void)afxdev_bind_stream(o->stream);
        afxdev_stream_sync(o->stream);
    }
    afx_scratch_drain(&o->scratchStream); /* the caller's stream may still run our kernels */
    afxdev_free(o->dTw);
    afxdev_free(o->dX);
    afxdev_free(o->dA);
    afxdev_free(o->dXt);
    afxdev_free(o->dRowMap);
    afxdev_free(o->dCell);
    afxdev_free(o->dStage);
    afxdev_free(o->dGA);
    afxdev_free(o->dGXt);
    afxdev_free(o->dGCell);
    afxdev_stream_destroy(o->stream);
    free(o);
}
