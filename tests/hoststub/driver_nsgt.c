/* driver_nsgt.c -- the NSGT host object under AddressSanitizer / UBSan, as a program of its own: nsgtObj_new / nsgt /
 * setMinLength / nsgtBatchDevice / free over the plans of tests/nsgt_cases.py against the generated stand-in of the device
 * layer (gen_stub.py --omit=afxk_nsgt_bands --omit=afxk_nsgt_spectrum).  The two launchers are supplied HERE: they do no
 * arithmetic but walk the uploaded plan exactly as k_nsgt_bands indexes it -- every table, window, twiddle, column-map and
 * spectrum element a wave would read is read, every cell and matrix element it would write is written -- so a table that
 * is too short or an index past a band, a row or a chunk is a sanitizer report.  "Device" buffers are exactly sized. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"

static volatile float sink;
static int launches;

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

int afxk_nsgt_bands(const AfxNsgtArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->outRe || !a->outIm || (a->cellRe == NULL) != (a->cellIm == NULL)) return AFX_ERR_ARG;
    if (a->chunks > 65535) return AFX_ERR_UNSUPPORTED;
    const long long N = 1LL << (a->r1 + a->r2);
    const int m1 = (1 << a->r1) - 1;
    float s = 0;
    launches++;
    for (int c = 0; c < a->chunks; c++)
        for (int it = 0; it < a->nItems; it++) {
            const int band = a->items[2 * it], n0 = a->items[2 * it + 1];
            const AfxNsgtBand b = a->bands[band];
            const int L = b.len, n1 = n0 + AFX_NSGT_BLOCK < L ? n0 + AFX_NSGT_BLOCK : L;
            if (band < 0 || band >= a->num || n0 < 0 || n0 >= L) return AFX_ERR_ARG;
            for (int j = 0; j < L && (n0 == 0 || j < 8); j++) { /* (every block forms the whole band: walked once) */
                long long f = (long long)b.offset + j;
                f = f < 0 ? 0 : (f > N - 1 ? N - 1 : f);
                const long long at = (((f & m1) << a->r2) | (f >> a->r1));
                s += a->Xt[2 * ((long long)c * N + at)] + a->Xt[2 * ((long long)c * N + at) + 1];
                s += a->window[b.cell + j] + a->twiddle[2 * ((long long)b.twiddle + j)] + a->twiddle[2 * ((long long)b.twiddle + j) + 1];
            }
            for (int n = n0; n < n1 && a->cellRe; n++) {
                a->cellRe[(long long)c * a->totalLength + b.cell + n] = 1.f;
                a->cellIm[(long long)c * a->totalLength + b.cell + n] = 2.f;
            }
            const int c0 = a->cellCol[b.cellCol + n0], c1 = a->cellCol[b.cellCol + n1];
            for (int col = c0; col < c1; col++) {
                const int idx = a->colMap[(long long)band * a->maxLength + col] - n0;
                if (idx < 0 || idx >= n1 - n0) {
                    printf("column %d of band %d maps outside its block\n", col, band);
                    return AFX_ERR_ARG;
                }
                a->outRe[((long long)c * a->num + band) * a->maxLength + col] += 1.f; /* (+=: every element exactly once) */
                a->outIm[((long long)c * a->num + band) * a->maxLength + col] += 2.f;
            }
        }
    sink = s;
    return AFX_OK;
}

typedef struct {
    const char *name;
    int num, r, sr;
    float low;
    int bpo, minLen, bank, scale, style, normal;
} Case;

/* tests/nsgt_cases.py */
static const Case CASES[] = {
    {"oct84", 84, 15, 32000, 32.703f, 12, 3, 0, 5, 0, 2}, {"mel12", 12, 9, 16000, 0.f, 12, 3, 0, 2, 0, 2},
    {"bark12std", 12, 9, 16000, 0.f, 12, 3, 1, 3, 7, 0},  {"oct24min", 24, 12, 32000, 32.703f, 12, 3, 0, 5, 0, 2},
    {"oct36rect", 36, 13, 32000, 32.703f, 6, 1, 0, 5, 4, 0}, {"log20std", 20, 11, 16000, 40.f, 12, 3, 1, 6, 9, 2},
    {"lin10", 10, 10, 16000, 0.f, 12, 3, 0, 0, 6, 0},     {"mel40", 40, 13, 32000, 0.f, 12, 3, 0, 2, 8, 2},
    {"bark2", 2, 10, 16000, 0.f, 12, 3, 0, 3, 4, 2},      {"linspace6", 6, 8, 16000, 100.f, 12, 3, 0, 1, 10, 2},
};

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

static int run_case(const Case *k, int minLen2) {
    NSGTObj o = NULL;
    int sr = k->sr, bpo = k->bpo, minLen = k->minLen;
    float low = k->low;
    NSGTFilterBankType bank = (NSGTFilterBankType)k->bank;
    SpectralFilterBankScaleType scale = (SpectralFilterBankScaleType)k->scale;
    SpectralFilterBankStyleType style = (SpectralFilterBankStyleType)k->style;
    SpectralFilterBankNormalType normal = (SpectralFilterBankNormalType)k->normal;
    CHECK(nsgtObj_new(&o, k->num, k->r, &sr, &low, NULL, &bpo, &minLen, &bank, &scale, &style, &normal) == 0 && o);
    const long long N = 1LL << k->r;
    for (int round = 0; round < 2; round++) {
        const int mx = nsgtObj_getMaxTimeLength(o), tot = nsgtObj_getTotalTimeLength(o);
        int sum = 0, longest = 0;
        for (int i = 0; i < k->num; i++) {
            const int L = nsgtObj_getTimeLengthArr(o)[i];
            sum += L;
            if (L > longest) longest = L;
            sink = nsgtObj_getFreBandArr(o)[i] + (float)nsgtObj_getBinBandArr(o)[i];
        }
        CHECK(sum == tot && longest == mx);
        /* host pointers, exactly sized */
        float *x = (float *)calloc((size_t)N, sizeof(float));
        float *re = (float *)calloc((size_t)k->num * mx, sizeof(float)), *im = (float *)calloc((size_t)k->num * mx, sizeof(float));
        CHECK(x && re && im);
        const int before = afxdev_error_count();
        nsgtObj_nsgt(o, x, re, im);
        CHECK(afxdev_error_count() == before);
        float *cr = NULL, *ci = NULL;
        nsgtObj_getCellData(o, &cr, &ci);
        CHECK(cr && ci && all_written(cr, tot, 1.f) && all_written(ci, tot, 2.f));
        free(re);
        free(im);
        /* "device" pointers: 3 chunks, odd stride, exactly sized outputs, with and without the cells */
        const int chunks = 3;
        const long long stride = N + 3;
        float *xs = (float *)calloc((size_t)((chunks - 1) * stride + N), sizeof(float));
        float *dre = (float *)calloc((size_t)chunks * k->num * mx, sizeof(float));
        float *dim = (float *)calloc((size_t)chunks * k->num * mx, sizeof(float));
        float *dcr = (float *)calloc((size_t)chunks * tot, sizeof(float)), *dci = (float *)calloc((size_t)chunks * tot, sizeof(float));
        CHECK(xs && dre && dim && dcr && dci);
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, chunks, stride, dre, dim, dcr, dci, NULL) == 0);
        CHECK(all_written(dre, (long long)chunks * k->num * mx, 1.f) && all_written(dim, (long long)chunks * k->num * mx, 2.f));
        CHECK(all_written(dcr, (long long)chunks * tot, 1.f) && all_written(dci, (long long)chunks * tot, 2.f));
        memset(dre, 0, sizeof(float) * (size_t)chunks * k->num * mx);
        memset(dim, 0, sizeof(float) * (size_t)chunks * k->num * mx);
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, chunks, stride, dre, dim, NULL, NULL, NULL) == 0);
        CHECK(all_written(dre, (long long)chunks * k->num * mx, 1.f));
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, chunks, N - 1, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, 0, stride, dre, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, chunks, stride, NULL, dim, NULL, NULL, NULL) == AFX_ERR_ARG);
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, chunks, stride, dre, dim, dcr, NULL, NULL) == AFX_ERR_ARG);
        free(x);
        free(xs);
        free(dre);
        free(dim);
        free(dcr);
        free(dci);
        if (round == 0) { /* the whole plan again, then a refused one: the object stays */
            const int errs = afxdev_error_count();
            nsgtObj_setMinLength(o, minLen2);
            CHECK(afxdev_error_count() == errs);
            int shortest = 1 << 30;
            for (int i = 0; i < k->num; i++)
                if (nsgtObj_getTimeLengthArr(o)[i] < shortest) shortest = nsgtObj_getTimeLengthArr(o)[i];
            CHECK(shortest >= minLen2);
            nsgtObj_setMinLength(o, (int)N + 1);
            CHECK(afxdev_error_count() > errs && nsgtObj_getTotalTimeLength(o) >= minLen2 * k->num);
            nsgtObj_setMinLength(o, 0); /* ignored */
        }
    }
    nsgtObj_free(o);
    printf("nsgt %s: new / nsgt / batch of 3 / setMinLength(%d) / refusal / free\n", k->name, minLen2);
    return 0;
}

int main(void) {
    for (size_t i = 0; i < sizeof(CASES) / sizeof(CASES[0]); i++)
        if (run_case(&CASES[i], i % 2 ? 40 : 7)) return 1;
    /* a large batch goes through the scratch in passes: 2^20 samples per chunk -> 16 chunks per pass */
    {
        NSGTObj o = NULL;
        int sr = 48000, scale = SpectralFilterBankScale_Mel;
        const int r = 20, num = 3, chunks = 20, before = launches;
        CHECK(nsgtObj_new(&o, num, r, &sr, NULL, NULL, NULL, NULL, NULL, (SpectralFilterBankScaleType *)&scale, NULL, NULL) == 0);
        const int mx = nsgtObj_getMaxTimeLength(o);
        float *xs = (float *)calloc((size_t)chunks << r, sizeof(float));
        float *dre = (float *)calloc((size_t)chunks * num * mx, sizeof(float)), *dim = (float *)calloc((size_t)chunks * num * mx, sizeof(float));
        CHECK(xs && dre && dim);
        CHECK(nsgtObj_nsgtBatchDevice(o, xs, chunks, 1LL << r, dre, dim, NULL, NULL, NULL) == 0);
        CHECK(launches - before == 2 && all_written(dre, (long long)chunks * num * mx, 1.f));
        free(xs);
        free(dre);
        free(dim);
        nsgtObj_free(o);
        printf("nsgt 2^20: %d chunks in two passes\n", chunks);
    }
    /* refused constructions leave no object; NULL objects are reported, not crashed on */
    {
        NSGTObj o = (NSGTObj)(size_t)1;
        int minLen = 300, scale = SpectralFilterBankScale_Mel, sr = 16000;
        CHECK(nsgtObj_new(&o, 12, 8, &sr, NULL, NULL, NULL, &minLen, NULL, (SpectralFilterBankScaleType *)&scale, NULL, NULL) == AFX_ERR_UNSUPPORTED && !o);
        CHECK(nsgtObj_new(&o, 12, 31, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -100 && !o);
        CHECK(nsgtObj_new(&o, 1, 10, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1 && !o);
        const int errs = afxdev_error_count();
        nsgtObj_nsgt(NULL, NULL, NULL, NULL);
        nsgtObj_setMinLength(NULL, 3);
        nsgtObj_getCellData(NULL, NULL, NULL);
        CHECK(afxdev_error_count() == errs + 3);
        nsgtObj_free(NULL);
    }
    printf("OK\n");
    return 0;
}
