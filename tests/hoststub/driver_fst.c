/* driver_fst.c -- the FST host object under AddressSanitizer / UBSan, as a program of its own: fstObj_new / fst /
 * fstBatchDevice / free for every supported radix2Exp against the generated stand-in of the device layer (gen_stub.py
 * --omit=afxk_fst_cells --omit=afxk_fst_expand --omit=afxk_nsgt_spectrum).  The three launchers are supplied HERE: they do no
 * arithmetic but walk the uploaded plan exactly as the kernels index it -- every twiddle, spectrum, row-map and cell element a
 * workgroup would read is read, every cell and matrix element it would write is written -- so a table
 * that is too short or an index past a band, a row, a block or a chunk is a sanitizer report.  "Device" buffers are exactly
 * sized. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"

static volatile float sink;
static int expands, cellLaunches, maxExpandRows;

int afxk_nsgt_spectrum(const AfxCwtPlanDims *d, const float *tw, const float *x, long long xStride, int chunks,
                       float *scratchA, float *Xt, void *stream) {
    (void)stream;
    const long long N = 1LL << (d->r1 + d->r2);
    float s = 0;
    if (d->pad != 0 || d->dataLength != N) return AFX_ERR_ARG;
    for (long long m = 0; m < N; m++) s += tw[m];
    for (int c = 0; c < chunks; c++)
        for (long long n = 0; n < N; n++) s += x[c * xStride + n];
    for (long long i = 0; i < 2 * N * chunks; i++) scratchA[i] = 0.f, Xt[i] = 1.f;
    sink = s;
    return AFX_OK;
}

int afxk_fst_cells(const AfxFstCellArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->Xt || !a->twiddle || !a->cellRe || !a->cellIm) return AFX_ERR_ARG;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const int r = a->r1 + a->r2, m1 = (1 << a->r1) - 1;
    const long long N = 1LL << r, cells = N / 2 + 1;
    float s = 0;
    cellLaunches++;
    for (int c = 0; c < a->chunks; c++)
        for (int b = 0; b <= r - 2; b++) {
            if (!(a->scale[b] > 0)) return AFX_ERR_ARG;
            if (b == 0) {
                const long long k[3] = {N - 1, 0, 1};
                for (int t = 0; t < 3; t++) {
                    s += a->Xt[2 * (c * N + (((k[t] & m1) << a->r2) | (k[t] >> a->r1)))];
                    a->cellRe[c * cells + t] = 1.f;
                    a->cellIm[c * cells + t] = 2.f;
                }
                continue;
            }
            const long long n = 1LL << b, twStride = N >> b;
            for (long long j = 0; j < n; j++) {
                const long long k = n + j;
                s += a->Xt[2 * (c * N + (((k & m1) << a->r2) | (k >> a->r1))) + 1];
                a->cellRe[c * cells + n + 1 + j] = 1.f;
                a->cellIm[c * cells + n + 1 + j] = 2.f;
            }
            for (long long p = 0; p < n / 4; p++) s += a->twiddle[2 * (2 * p * twStride) + 1]; /* afx_ldsfft.h: tw[2 ta], ta < N / 4 */
        }
    sink = s;
    return AFX_OK;
}

int afxk_fst_expand(const AfxFstExpandArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->rowMap || !a->cellRe || !a->cellIm || !a->outRe || !a->outIm) return AFX_ERR_ARG;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const int r = a->radix2Exp;
    const long long N = 1LL << r, cells = N / 2 + 1;
    if (a->minIndex < 0 || a->rows <= 0 || a->minIndex + a->rows > cells) return AFX_ERR_ARG;
    float s = 0;
    expands++;
    if (a->rows > maxExpandRows) maxExpandRows = a->rows;
    for (int c = 0; c < a->chunks; c++)
        for (long long k = 0; k < a->rows; k++) {
            const int first = a->rowMap[2 * (a->minIndex + k)], shift = a->rowMap[2 * (a->minIndex + k) + 1];
            for (long long l = 0; l < N; l += 4) {
                s += a->cellRe[c * cells + first + (l >> shift)] + a->cellIm[c * cells + first + (l >> shift)];
                for (int e = 0; e < 4; e++) {
                    a->outRe[(c * a->rows + k) * N + l + e] = 1.f;
                    a->outIm[(c * a->rows + k) * N + l + e] = 2.f;
                }
            }
        }
    sink = s;
    return AFX_OK;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, afxdev_last_error()); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int all_written(const float *p, long long n, float v) {
    for (long long i = 0; i < n; i++)
        if (p[i] != v) return 0;
    return 1;
}

/* host entry over lo ... hi into exactly sized arrays; the stand-in cells are 1 / 2 after ONE cell launch */
static int host_rows(FSTObj o, int r, int lo, int hi, int passes) {
    const long long N = 1LL << r, rows = (long long)hi - lo + 1;
    float *x = (float *)calloc((size_t)N, sizeof(float));
    float *re = (float *)calloc((size_t)(rows * N), sizeof(float)), *im = (float *)calloc((size_t)(rows * N), sizeof(float));
    CHECK(x && re && im);
    const int before = afxdev_error_count(), e0 = expands, c0 = cellLaunches;
    fstObj_fst(o, x, lo, hi, re, im);
    CHECK(afxdev_error_count() == before);
    CHECK(cellLaunches - c0 == 1 && expands - e0 == passes);
    CHECK(all_written(re, rows * N, 1.f) && all_written(im, rows * N, 2.f));
    free(x);
    free(re);
    free(im);
    return 0;
}

static int run_exp(int r) {
    FSTObj o = NULL;
    CHECK(fstObj_new(&o, r) == 0 && o);
    const long long N = 1LL << r, cells = N / 2 + 1;
    const int half = (int)(N / 2);
    CHECK(fstObj_getCellLength(o) == cells);
    /* the host entry: row windows at both ends, one row, and the passes of 2^22 floats a plane */
    const int full = half + 1, stage = (int)((1LL << 22) / N);
    if (host_rows(o, r, 0, half < 40 ? half : 40, 1)) return 1;
    if (host_rows(o, r, half - (half < 40 ? half : 40), half, 1)) return 1;
    if (host_rows(o, r, half, half, 1)) return 1;
    if (r == 14) { /* 256 rows a pass: 700 rows in three passes, the last one short */
        maxExpandRows = 0;
        if (host_rows(o, r, half - 699, half, 3)) return 1;
        CHECK(maxExpandRows == stage && stage == 256);
    } else if (r <= 10) {
        if (host_rows(o, r, 0, half, (full + stage - 1) / stage)) return 1;
    }
    /* "device" pointers: 3 chunks, odd stride, exactly sized outputs; matrix + cells, matrix only, cells only */
    const int chunks = 3, lo = r < 6 ? 0 : 3, hi = r < 6 ? half : (half < 30 ? half : 30);
    const long long stride = N + 3, rows = hi - lo + 1;
    float *xs = (float *)calloc((size_t)((chunks - 1) * stride + N), sizeof(float));
    float *dre = (float *)calloc((size_t)(chunks * rows * N), sizeof(float)), *dim = (float *)calloc((size_t)(chunks * rows * N), sizeof(float));
    float *dcr = (float *)calloc((size_t)(chunks * cells), sizeof(float)), *dci = (float *)calloc((size_t)(chunks * cells), sizeof(float));
    CHECK(xs && dre && dim && dcr && dci);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, hi, dre, dim, dcr, dci, NULL) == 0);
    CHECK(all_written(dre, chunks * rows * N, 1.f) && all_written(dim, chunks * rows * N, 2.f));
    CHECK(all_written(dcr, chunks * cells, 1.f) && all_written(dci, chunks * cells, 2.f));
    memset(dre, 0, sizeof(float) * (size_t)(chunks * rows * N));
    memset(dim, 0, sizeof(float) * (size_t)(chunks * rows * N));
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, hi, dre, dim, NULL, NULL, NULL) == 0);
    CHECK(all_written(dre, chunks * rows * N, 1.f) && all_written(dim, chunks * rows * N, 2.f));
    CHECK(all_written(dcr, chunks * cells, 1.f)); /* untouched */
    memset(dcr, 0, sizeof(float) * (size_t)(chunks * cells));
    memset(dci, 0, sizeof(float) * (size_t)(chunks * cells));
    const int e0 = expands;
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, hi, NULL, NULL, dcr, dci, NULL) == 0);
    CHECK(expands == e0 && all_written(dcr, chunks * cells, 1.f) && all_written(dci, chunks * cells, 2.f));
    /* refusals */
    CHECK(fstObj_fstBatchDevice(NULL, xs, chunks, stride, lo, hi, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, NULL, chunks, stride, lo, hi, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, hi, dre, NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, hi, dre, dim, dcr, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, hi, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, 0, stride, lo, hi, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, N - 1, lo, hi, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, -1, hi, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, hi, lo, dre, dim, NULL, NULL, NULL) == (lo == hi ? 0 : AFX_ERR_ARG));
    CHECK(fstObj_fstBatchDevice(o, xs, chunks, stride, lo, half + 1, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
    /* minIndex > maxIndex on the host entry: nothing written, counted */
    {
        const int errs = afxdev_error_count(), e1 = expands;
        float one = 0.f;
        fstObj_fst(o, xs, 7, 3, &one, &one);
        fstObj_fst(o, xs, half + 5, half + 9, &one, &one); /* clamped to half + 5 ... half */
        CHECK(afxdev_error_count() >= errs + 2 && expands == e1 && one == 0.f);
        fstObj_fst(o, NULL, 0, 1, &one, &one);
        CHECK(afxdev_error_count() >= errs + 3);
    }
    free(xs);
    free(dre);
    free(dim);
    free(dcr);
    free(dci);
    fstObj_free(o);
    printf("fst 2^%d: new / fst windows / batch of 3 in three forms / refusals / free\n", r);
    return 0;
}

int main(void) {
    for (int r = AFX_FST_MIN_EXP; r <= AFX_FST_MAX_EXP; r++)
        if (run_exp(r)) return 1;
    /* a large batch goes through the scratch in passes: 2^14 samples per chunk -> 1024 chunks per pass */
    {
        FSTObj o = NULL;
        const int r = 14, chunks = 1030, before = cellLaunches;
        CHECK(fstObj_new(&o, r) == 0);
        const long long cells = (1LL << r) / 2 + 1;
        float *xs = (float *)calloc((size_t)chunks << r, sizeof(float));
        float *dcr = (float *)calloc((size_t)(chunks * cells), sizeof(float)), *dci = (float *)calloc((size_t)(chunks * cells), sizeof(float));
        float *dre = (float *)calloc((size_t)chunks << r, sizeof(float)), *dim = (float *)calloc((size_t)chunks << r, sizeof(float));
        CHECK(xs && dcr && dci && dre && dim);
        CHECK(fstObj_fstBatchDevice(o, xs, chunks, 1LL << r, 0, 0, NULL, NULL, dcr, dci, NULL) == 0);
        CHECK(cellLaunches - before == 2 && all_written(dcr, chunks * cells, 1.f) && all_written(dci, chunks * cells, 2.f));
        /* matrix only: the cells of a pass live in the object's scratch */
        CHECK(fstObj_fstBatchDevice(o, xs, chunks, 1LL << r, 8192, 8192, dre, dim, NULL, NULL, NULL) == 0);
        CHECK(all_written(dre, (long long)chunks << r, 1.f) && all_written(dim, (long long)chunks << r, 2.f));
        free(xs);
        free(dcr);
        free(dci);
        free(dre);
        free(dim);
        fstObj_free(o);
        printf("fst 2^14: %d chunks in two passes\n", chunks);
    }
    /* refused constructions leave no object; NULL objects are reported, not crashed on; the plan without a device */
    {
        FSTObj o = (FSTObj)(size_t)1;
        CHECK(fstObj_new(&o, 2) == -1 && !o);
        o = (FSTObj)(size_t)1;
        CHECK(fstObj_new(&o, 3) == AFX_ERR_UNSUPPORTED && !o);
        CHECK(fstObj_new(&o, 15) == AFX_ERR_UNSUPPORTED && !o);
        CHECK(fstObj_new(NULL, 10) == -1);
        const int errs = afxdev_error_count();
        fstObj_fst(NULL, NULL, 0, 1, NULL, NULL);
        CHECK(afxdev_error_count() == errs + 1 && fstObj_getCellLength(NULL) == 0);
        fstObj_free(NULL);
        int cell[9], len[9];
        CHECK(afx_fst_plan_host(4, cell, len) == 0 && cell[8] == 5 && len[8] == 4 && cell[3] == 3 && len[4] == 2);
        CHECK(afx_fst_plan_host(2, NULL, NULL) == -1 && afx_fst_plan_host(14, NULL, NULL) == 0);
    }
    printf("OK\n");
    return 0;
}
