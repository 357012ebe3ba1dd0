/* afx_st.c -- the S-transform object (C host side) behind include/st_algorithm.h.
 *
 * The reference (src/st_algorithm.c) keeps the spectrum twice in a row and an (N/2 + 1) x N float table of the Gaussian
 * windows, and runs one N-point inverse transform per requested bin on one thread.  Here the plan is what the kernel needs
 * to evaluate a window itself: the N/2 + 1 coefficients c_k and the list of requested bins, both on the device.  The
 * contiguous range of stObj_new is simply a list, so stObj_useBinArr has no code path of its own.
 * Execution: afxk_nsgt_spectrum (afx_cwt.hip) + afxk_st_rows (afx_st.hip).
 *
 * Divergences from the reference, all deliberate (st_algorithm.h): the row of bin 0 writes zeros to the
 * imaginary plane; stObj_useBinArr with length <= 0 or > N is refused and counted; radix2Exp outside 4 ... 14 is refused.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objkit.h"
#include "st_algorithm.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

#define ST_STAGE_FLOATS (1ll << 22) /* per plane of the host entry's staging buffer (st_algorithm.h) */

struct OpaqueST {
    int radix2Exp, binLength;
    float factor, norm;
    AfxCwtPlanDims dims;
    void *stream;
    float *dTw, *dX, *dA, *dXt; /* forward twiddles, one chunk's samples / scratch / spectrum */
    float *dCoef;               /* [N / 2 + 1]: c_k */
    int *dBins;                 /* [N]: the first binLength entries are the rows */
    float *dStage;              /* [2][stage floats]: row blocks of the host entry */
    size_t capStage;
    float *dGA, *dGXt;          /* scratch of the batched call: `pass` chunks at a time */
    size_t capGA, capGXt;
    AfxScratchStream scratchStream;
    int status;
};

int afx_st_plan_host(int radix2Exp, float factor, float norm, float *coef) {
    if (radix2Exp < 1 || radix2Exp > 24 || !coef) return -1;
    const int half = 1 << (radix2Exp - 1);
    coef[0] = 0.f;
    for (int i = 1; i <= half; i++) coef[i] = -factor * 2 * M_PI * M_PI / (powf(i, 2 * norm)); /* st_algorithm.c:235 */
    return 0;
}

/* the plan (c_k or the bins) changes under batched calls that may still run on their caller's stream -- the default
 * stream included, which the object's own non-blocking stream does not wait for: drain it first */
static int upload(STObj o, void *dst, const void *src, size_t bytes) {
    int st = o->scratchStream.used ? afxdev_stream_sync(o->scratchStream.stream) : AFX_OK;
    if (st == AFX_OK) st = afxdev_h2d(dst, src, bytes, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    return st;
}

static int upload_coef(STObj o, float factor, float norm) {
    const size_t n = ((size_t)1 << (o->radix2Exp - 1)) + 1;
    float *coef = (float *)malloc(sizeof(float) * n);
    if (!coef) return AFX_ERR_NOMEM;
    (void)afx_st_plan_host(o->radix2Exp, factor, norm, coef);
    const int st = upload(o, o->dCoef, coef, sizeof(float) * n);
    free(coef);
    if (st == AFX_OK) o->factor = factor, o->norm = norm;
    return st;
}

int stObj_new(STObj *stObj, int radix2Exp, int minIndex, int maxIndex, float *factor, float *norm) {
    if (!stObj) return -1;
    *stObj = NULL;
    if (radix2Exp < AFX_FST_MIN_EXP || radix2Exp > AFX_FST_MAX_EXP) {
        afxdev_set_error("stObj_new: chunks of 2^%d samples are not supported (2^%d ... 2^%d)", radix2Exp, AFX_FST_MIN_EXP,
                         AFX_FST_MAX_EXP);
        return AFX_ERR_UNSUPPORTED;
    }
    STObj o = (STObj)calloc(1, sizeof(struct OpaqueST));
    if (!o) return AFX_ERR_NOMEM;
    const size_t N = (size_t)1 << radix2Exp;
    float _factor = 1, _norm = 1; /* st_algorithm.c:59-74 */
    if (factor && *factor > 0) _factor = *factor;
    if (norm && *norm > 0) _norm = *norm;
    if (minIndex >= maxIndex || minIndex < 0 || maxIndex > (int)(N / 2)) { /* st_algorithm.c:90-93 */
        minIndex = 0;
        maxIndex = (int)(N / 2);
    }
    o->radix2Exp = radix2Exp;
    o->binLength = maxIndex - minIndex + 1;
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
    int *bins = NULL;
    if (st == AFX_OK) {
        tw = afx_twiddle_table((int)N);
        bins = (int *)malloc(sizeof(int) * (size_t)o->binLength);
        if (!tw || !bins) st = AFX_ERR_NOMEM;
    }
    if (st == AFX_OK) {
        for (int i = 0; i < o->binLength; i++) bins[i] = minIndex + i;
        st = afxdev_stream_create(&o->stream);
    }
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dTw, sizeof(float) * N);
    if (st == AFX_OK) st = afxdev_h2d(o->dTw, tw, sizeof(float) * N, o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dBins, sizeof(int) * N);
    if (st == AFX_OK) st = afxdev_h2d(o->dBins, bins, sizeof(int) * (size_t)o->binLength, o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dCoef, sizeof(float) * (N / 2 + 1));
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dX, sizeof(float) * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dA, sizeof(float) * 2 * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dXt, sizeof(float) * 2 * N);
    if (st == AFX_OK) st = upload_coef(o, _factor, _norm); /* ends in a synchronise: tw and bins have arrived */
    free(tw);
    free(bins);
    if (st != AFX_OK) {
        stObj_free(o);
        return st;
    }
    *stObj = o;
    return 0;
}

int stObj_getBinLength(STObj o) { return o ? o->binLength : 0; }

void stObj_useBinArr(STObj o, int *binArr, int length) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("stObj_useBinArr: NULL object");
        return;
    }
    const int N = o->dims.dataLength;
    if (!binArr || length <= 0 || length > N) { /* divergence 2: the reference copies `length` ints into N */
        afxdev_set_error("stObj_useBinArr: %d bins do not fit the object's 1 ... %d: the bins stay as they were", length, N);
        AFX_FAIL(o, AFX_ERR_ARG, "stObj_useBinArr");
        return;
    }
    for (int i = 0; i < length; i++)
        if (binArr[i] > N / 2 || binArr[i] < 0) return; /* st_algorithm.c:120-125: ignored silently */
    const int st = upload(o, o->dBins, binArr, sizeof(int) * (size_t)length);
    if (st != AFX_OK) {
        AFX_FAIL(o, st, "stObj_useBinArr");
        return;
    }
    o->binLength = length;
}

void stObj_setValue(STObj o, float factor, float norm) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("stObj_setValue: NULL object");
        return;
    }
    if (o->factor == factor && o->norm == norm) return; /* st_algorithm.c:137-139 */
    const int st = upload_coef(o, factor, norm);
    if (st != AFX_OK) AFX_FAIL(o, st, "stObj_setValue");
}

static int run_rows(STObj o, const float *Xt, int firstRow, int rows, int chunks, float *outRe, float *outIm, void *stream) {
    AfxStArgs a;
    memset(&a, 0, sizeof(a));
    a.r1 = o->dims.r1;
    a.r2 = o->dims.r2;
    a.Xt = Xt;
    a.twiddle = o->dTw;
    a.coef = o->dCoef;
    a.bins = o->dBins + firstRow;
    a.rows = rows;
    a.chunks = chunks;
    a.outRe = outRe;
    a.outIm = outIm;
    return afxk_st_rows(&a, stream);
}

int stObj_stBatchDevice(STObj o, const float *x, int chunks, long long xStride, float *outRe, float *outIm, void *stream) {
    AFX_ENTER(o);
    if (!o || !x || !outRe || !outIm || chunks <= 0 || xStride < o->dims.dataLength) {
        afxdev_set_error("stObj_stBatchDevice: bad argument");
        return AFX_ERR_ARG;
    }
    if (stream) { /* the plan lives on the object's device */
        const int dev = afxdev_current_device();
        int st = afxdev_bind_stream(stream);
        if (st == AFX_OK && afxdev_current_device() != dev) {
            (void)afxdev_bind_stream(o->stream);
            afxdev_set_error("stObj_stBatchDevice: the stream belongs to another device than the object");
            st = AFX_ERR_ARG;
        }
        if (st != AFX_OK) return st;
    }
    const size_t N = (size_t)o->dims.dataLength, rows = (size_t)o->binLength;
    int st = afx_scratch_wait(&o->scratchStream, stream);
    /* spectra of a pass: at most 128 MB each for the scratch and the result, and a launch takes 65535 chunks */
    long long pass = (long long)((128u << 20) / (8 * N));
    if (pass > 65535) pass = 65535;
    if (pass > chunks) pass = chunks;
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dGA, &o->capGA, sizeof(float) * 2 * N * (size_t)pass);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dGXt, &o->capGXt, sizeof(float) * 2 * N * (size_t)pass);
    for (long long c = 0; c < chunks && st == AFX_OK; c += pass) {
        const int n = (int)(chunks - c < pass ? chunks - c : pass);
        st = afxk_nsgt_spectrum(&o->dims, o->dTw, x + c * xStride, xStride, n, o->dGA, o->dGXt, stream);
        if (st == AFX_OK)
            st = run_rows(o, o->dGXt, 0, (int)rows, n, outRe + (size_t)c * rows * N, outIm + (size_t)c * rows * N, stream);
    }
    afx_scratch_mark(&o->scratchStream, stream);
    if (st != AFX_OK) AFX_FAIL(o, st, "stObj_stBatchDevice");
    return st;
}

void stObj_st(STObj o, float *dataArr, float *mRealArr, float *mImageArr) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("stObj_st: NULL object");
        return;
    }
    if (!dataArr || !mRealArr || !mImageArr) {
        afxdev_set_error("stObj_st: NULL array");
        AFX_FAIL(o, AFX_ERR_ARG, "stObj_st");
        return;
    }
    const size_t N = (size_t)o->dims.dataLength;
    const long long rows = o->binLength;
    long long block = ST_STAGE_FLOATS / (long long)N; /* rows of a pass */
    if (block > rows) block = rows;
    const size_t plane = (size_t)block * N;
    int st = afxdev_reserve((void **)&o->dStage, &o->capStage, sizeof(float) * 2 * plane);
    if (st == AFX_OK) st = afxdev_h2d(o->dX, dataArr, sizeof(float) * N, o->stream);
    if (st == AFX_OK) st = afxk_nsgt_spectrum(&o->dims, o->dTw, o->dX, (long long)N, 1, o->dA, o->dXt, o->stream);
    for (long long k = 0; k < rows && st == AFX_OK; k += block) {
        const long long n = rows - k < block ? rows - k : block;
        st = run_rows(o, o->dXt, (int)k, (int)n, 1, o->dStage, o->dStage + plane, o->stream);
        if (st == AFX_OK) st = afxdev_d2h(mRealArr + (size_t)k * N, o->dStage, sizeof(float) * (size_t)n * N, o->stream);
        if (st == AFX_OK) st = afxdev_d2h(mImageArr + (size_t)k * N, o->dStage + plane, sizeof(float) * (size_t)n * N, o->stream);
    }
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) AFX_FAIL(o, st, "stObj_st");
}

void stObj_free(STObj o) {
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
    afxdev_free(o->dCoef);
    afxdev_free(o->dBins);
    afxdev_free(o->dStage);
    afxdev_free(o->dGA);
    afxdev_free(o->dGXt);
    afxdev_stream_destroy(o->stream);
    free(o);
}
