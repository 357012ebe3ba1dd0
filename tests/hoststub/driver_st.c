/* driver_st.c -- the ST host object under AddressSanitizer / UBSan, as a program of its own: stObj_new / useBinArr /
 * setValue / st / stBatchDevice / free for every supported radix2Exp against the generated stand-in of the device layer
 * (gen_stub.py --omit=afxk_st_rows --omit=afxk_nsgt_spectrum).  The two launchers are supplied HERE: they do no arithmetic but
 * walk the uploaded plan exactly as the kernels index it -- every twiddle, spectrum, bin and coefficient a workgroup would read
 * is read, every element it would write is written -- so a table that is too short or an index past a row, a block or a
 * chunk is a sanitizer report.  "Device" buffers are exactly sized.  The row launcher writes bin + coefficient into the real
 * plane, so the driver sees which plan a call ran with. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"

static volatile float sink;
static int rowLaunches, maxRows;

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

int afxk_st_rows(const AfxStArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->Xt || !a->twiddle || !a->coef || !a->bins || !a->outRe || !a->outIm || a->rows <= 0) return AFX_ERR_ARG;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const int r = a->r1 + a->r2;
    const long long N = 1LL << r;
    float s = 0;
    rowLaunches++;
    if (a->rows > maxRows) maxRows = a->rows;
    for (long long p = 0; p < N / 4; p++) s += a->twiddle[2 * (2 * p) + 1]; /* afx_ldsfft.h: tw[2 ta], ta < N / 4 */
    for (int c = 0; c < a->chunks; c++) {
        for (long long m = 0; m < 2 * N; m++) s += a->Xt[2 * c * N + m];
        for (long long i = 0; i < a->rows; i++) {
            const int k = a->bins[i];
            if (k < 0 || k > N / 2) return AFX_ERR_ARG;
            const float v = (float)k + (k ? a->coef[k] : 0.f);
            for (long long n = 0; n < N; n++) {
                a->outRe[(c * a->rows + i) * N + n] = v;
                a->outIm[(c * a->rows + i) * N + n] = 2.f;
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

/* every row i of `chunks` chunks holds bins[i] + coef[bins[i]] in the real plane and 2 in the imaginary one */
static int rows_hold(const float *re, const float *im, int chunks, const int *bins, int rows, long long N, const float *coef) {
    for (int c = 0; c < chunks; c++)
        for (int i = 0; i < rows; i++)
            for (long long n = 0; n < N; n++) {
                const long long at = ((long long)c * rows + i) * N + n;
                if (re[at] != (float)bins[i] + (bins[i] ? coef[bins[i]] : 0.f) || im[at] != 2.f) return 0;
            }
    return 1;
}

/* host entry into exactly sized arrays */
static int host_rows(STObj o, int r, const int *bins, int rows, const float *coef, int passes) {
    const long long N = 1LL << r;
    float *x = (float *)calloc((size_t)N, sizeof(float));
    float *re = (float *)calloc((size_t)(rows * N), sizeof(float)), *im = (float *)calloc((size_t)(rows * N), sizeof(float));
    CHECK(x && re && im);
    const int before = afxdev_error_count(), l0 = rowLaunches;
    CHECK(stObj_getBinLength(o) == rows);
    stObj_st(o, x, re, im);
    CHECK(afxdev_error_count() == before);
    CHECK(rowLaunches - l0 == passes);
    CHECK(rows_hold(re, im, 1, bins, rows, N, coef));
    free(x);
    free(re);
    free(im);
    return 0;
}

static int run_exp(int r) {
    const long long N = 1LL << r;
    const int half = (int)(N / 2), stage = (int)((1LL << 22) / N);
    float *coef = (float *)calloc((size_t)half + 1, sizeof(float)), *coef2 = (float *)calloc((size_t)half + 1, sizeof(float));
    int *all = (int *)calloc((size_t)N + 1, sizeof(int));
    CHECK(coef && coef2 && all);
    CHECK(afx_st_plan_host(r, 1.f, 1.f, coef) == 0 && afx_st_plan_host(r, 2.5f, 0.8f, coef2) == 0);
    CHECK(coef[0] == 0.f && coef[1] < -19.7f && coef[1] > -19.8f && coef2[half] != coef[half]);
    for (int i = 0; i <= half; i++) all[i] = i;
    STObj o = NULL;
    /* a range; factor / norm NULL and <= 0 are 1 */
    float zero = 0.f, neg = -3.f;
    const int lo = 1, hi = half < 40 ? half - 1 : 40;
    CHECK(stObj_new(&o, r, lo, hi, &zero, &neg) == 0 && o);
    if (host_rows(o, r, all + lo, hi - lo + 1, coef, 1)) return 1;
    /* setValue: the same values change nothing, new ones are uploaded */
    stObj_setValue(o, 1.f, 1.f);
    if (host_rows(o, r, all + lo, hi - lo + 1, coef, 1)) return 1;
    stObj_setValue(o, 2.5f, 0.8f);
    if (host_rows(o, r, all + lo, hi - lo + 1, coef2, 1)) return 1;
    /* useBinArr: good (unordered, repeated, both ends), out of range (ignored silently), over-long and empty (counted) */
    int list[5] = {0, half, 7, 7, half - 1}, bad1[2] = {3, half + 1}, bad2[1] = {-1};
    stObj_useBinArr(o, list, 5);
    if (host_rows(o, r, list, 5, coef2, 1)) return 1;
    {
        const int errs = afxdev_error_count();
        stObj_useBinArr(o, bad1, 2);
        stObj_useBinArr(o, bad2, 1);
        CHECK(afxdev_error_count() == errs && stObj_getBinLength(o) == 5);
        stObj_useBinArr(o, all, (int)N + 1);
        stObj_useBinArr(o, all, 0);
        stObj_useBinArr(o, NULL, 3);
        CHECK(afxdev_error_count() >= errs + 3 && stObj_getBinLength(o) == 5);
    }
    if (host_rows(o, r, list, 5, coef2, 1)) return 1;
    /* "device" pointers: 3 chunks, odd stride, exactly sized outputs */
    const int chunks = 3;
    const long long stride = N + 3;
    float *xs = (float *)calloc((size_t)((chunks - 1) * stride + N), sizeof(float));
    float *dre = (float *)calloc((size_t)(chunks * 5 * N), sizeof(float)), *dim = (float *)calloc((size_t)(chunks * 5 * N), sizeof(float));
    CHECK(xs && dre && dim);
    CHECK(stObj_stBatchDevice(o, xs, chunks, stride, dre, dim, NULL) == 0);
    CHECK(rows_hold(dre, dim, chunks, list, 5, N, coef2));
    /* refusals */
    CHECK(stObj_stBatchDevice(NULL, xs, chunks, stride, dre, dim, NULL) == AFX_ERR_ARG);
    CHECK(stObj_stBatchDevice(o, NULL, chunks, stride, dre, dim, NULL) == AFX_ERR_ARG);
    CHECK(stObj_stBatchDevice(o, xs, chunks, stride, NULL, dim, NULL) == AFX_ERR_ARG);
    CHECK(stObj_stBatchDevice(o, xs, chunks, stride, dre, NULL, NULL) == AFX_ERR_ARG);
    CHECK(stObj_stBatchDevice(o, xs, 0, stride, dre, dim, NULL) == AFX_ERR_ARG);
    CHECK(stObj_stBatchDevice(o, xs, chunks, N - 1, dre, dim, NULL) == AFX_ERR_ARG);
    {
        const int errs = afxdev_error_count();
        float one = 0.f;
        stObj_st(o, NULL, &one, &one);
        stObj_st(o, xs, NULL, &one);
        CHECK(afxdev_error_count() >= errs + 2 && one == 0.f);
    }
    free(xs);
    free(dre);
    free(dim);
    stObj_free(o);
    /* the fall-back to the full range; the host entry's passes of 2^22 floats a plane; the longest list, N rows */
    o = NULL;
    CHECK(stObj_new(&o, r, 7, 7, NULL, NULL) == 0 && stObj_getBinLength(o) == half + 1);
    if (r <= 10) {
        if (host_rows(o, r, all, half + 1, coef, (half + 1 + stage - 1) / stage)) return 1;
        for (int i = 0; i < N; i++) all[i] = i % (half + 1);
        stObj_useBinArr(o, all, (int)N);
        if (host_rows(o, r, all, (int)N, coef, ((int)N + stage - 1) / stage)) return 1;
    } else if (r == 14) { /* 256 rows a pass: 700 rows in three passes, the last one short */
        maxRows = 0;
        stObj_useBinArr(o, all + half - 699, 700);
        if (host_rows(o, r, all + half - 699, 700, coef, 3)) return 1;
        CHECK(maxRows == stage && stage == 256);
    }
    stObj_free(o);
    free(coef);
    free(coef2);
    free(all);
    printf("st 2^%d: new / setValue / useBinArr good, out of range, over-long / st / batch of 3 / refusals / free\n", r);
    return 0;
}

int main(void) {
    for (int r = AFX_FST_MIN_EXP; r <= AFX_FST_MAX_EXP; r++)
        if (run_exp(r)) return 1;
    /* a large batch goes through the scratch in passes: 2^14 samples per chunk -> 1024 chunks per pass */
    {
        STObj o = NULL;
        const int r = 14, chunks = 1030, before = rowLaunches;
        float coef[8193];
        int bin[1] = {8192};
        CHECK(afx_st_plan_host(r, 1.f, 1.f, coef) == 0);
        CHECK(stObj_new(&o, r, 8191, 8192, NULL, NULL) == 0 && stObj_getBinLength(o) == 2);
        stObj_useBinArr(o, bin, 1);
        float *xs = (float *)calloc((size_t)chunks << r, sizeof(float));
        float *dre = (float *)calloc((size_t)chunks << r, sizeof(float)), *dim = (float *)calloc((size_t)chunks << r, sizeof(float));
        CHECK(xs && dre && dim);
        CHECK(stObj_stBatchDevice(o, xs, chunks, 1LL << r, dre, dim, NULL) == 0);
        CHECK(rowLaunches - before == 2 && rows_hold(dre, dim, chunks, bin, 1, 1LL << r, coef));
        free(xs);
        free(dre);
        free(dim);
        stObj_free(o);
        printf("st 2^14: %d chunks in two passes\n", chunks);
    }
    /* refused constructions leave no object; NULL objects are reported, not crashed on */
    {
        STObj o = (STObj)(size_t)1;
        CHECK(stObj_new(&o, 3, 0, 4, NULL, NULL) == AFX_ERR_UNSUPPORTED && !o);
        o = (STObj)(size_t)1;
        CHECK(stObj_new(&o, 15, 0, 4, NULL, NULL) == AFX_ERR_UNSUPPORTED && !o);
        CHECK(stObj_new(NULL, 10, 0, 4, NULL, NULL) == -1);
        const int errs = afxdev_error_count();
        int b[1] = {1};
        stObj_st(NULL, NULL, NULL, NULL);
        stObj_useBinArr(NULL, b, 1);
        stObj_setValue(NULL, 1.f, 1.f);
        CHECK(afxdev_error_count() == errs + 3 && stObj_getBinLength(NULL) == 0);
        stObj_free(NULL);
        float c[3];
        CHECK(afx_st_plan_host(0, 1.f, 1.f, c) == -1 && afx_st_plan_host(25, 1.f, 1.f, c) == -1 &&
              afx_st_plan_host(4, 1.f, 1.f, NULL) == -1 && afx_st_plan_host(2, 1.f, 1.f, c) == 0 && c[0] == 0.f && c[2] < 0.f);
    }
    printf("OK\n");
    return 0;
}
