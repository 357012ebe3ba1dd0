/* driver_onset.c -- the onset host object under AddressSanitizer / UBSan, as a program of its own: onsetObj_new / onset /
 * onsetBatchDevice / debug / free, afx_onset_plan_host, afx_maxFilterDevice, afx_peakPickDevice, afx_powerToDbDevice and
 * util_powerToDB against the generated stand-in of the device layer (gen_stub.py --omit=afxk_descriptors,
 * --omit=afxk_max_filter, --omit=afxk_onset_pick, --omit=afxk_power_to_db).  The four launchers are supplied HERE: they do no
 * novelty arithmetic but read every row, every index-table entry and every scratch word and write every output the kernels
 * would, so a scratch buffer, a staging buffer or a chunk that is too small is a sanitizer report ("device" buffers are
 * exactly sized).  The stand-in envelope of a clip is a checksum of its rows, the points are the frames 0, 2, 4, ...: a
 * chunked batch must reproduce the one-pass result exactly. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "mir/onset_algorithm.h"

static volatile float sink;
static int filterLaunches, descLaunches, pickLaunches, dbLaunches;
static long long maxFilterRows;

int afxk_max_filter(const float *in, long long rows, int cols, int order, float *out, void *stream) {
    (void)stream;
    if (!in || !out || in == out || rows < 0 || cols < 1 || order < 1) return AFX_ERR_ARG;
    for (long long i = 0; i < rows * cols; i++) out[i] = in[i] + 1.f;
    filterLaunches++;
    if (rows > maxFilterRows) maxFilterRows = rows;
    return AFX_OK;
}

int afxk_descriptors(const AfxDescArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->spec || !a->out || !a->fre || !a->req || a->count != 1 || a->rows <= 0 || a->len < 1) return AFX_ERR_ARG;
    if (a->idx0 < 0 || a->idx0 >= a->num || (!a->idx && a->start + a->len > a->num)) return AFX_ERR_ARG;
    const int kind = a->req[0].kind;
    const int phase = kind >= AFX_DESC_PD && kind <= AFX_DESC_RCD;
    if (phase && !a->phase) return AFX_ERR_ARG;
    if (a->outStride < a->rows || a->framesPerClip < 1 || a->rows % a->framesPerClip) return AFX_ERR_ARG;
    float f = 0;
    for (int j = 0; j < a->num; j++) f += a->fre[j];
    for (long long r = 0; r < a->rows; r++) {
        float s = f;
        for (int p = 0; p < a->len; p++) {
            const int j = a->idx ? a->idx[p] : a->start + p;
            if (j < 0 || j >= a->num) return AFX_ERR_ARG;
            s += a->spec[r * a->num + j] * (float)(p + 1);
            if (phase) s += a->phase[r * a->num + j];
        }
        a->out[(long long)a->req[0].slot * a->outStride + r] = s;
    }
    descLaunches++;
    return AFX_OK;
}

int afxk_onset_pick(const AfxOnsetPickArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->src || a->batch <= 0 || a->length <= 0 || (a->normalise && !a->evn)) return AFX_ERR_ARG;
    if (a->preMax < 0 || a->preAvg < 0 || a->wait < 0 || a->postMax < 1 || a->postAvg < 1) return AFX_ERR_ARG;
    for (int b = 0; b < a->batch; b++) {
        int cnt = 0;
        for (int t = 0; t < a->length; t++) {
            const float v = a->src[b * a->srcStride + t];
            if (a->normalise) a->evn[b * a->evnStride + t] = v;
            sink = v;
            if (t % 2 == 0) {
                if (a->point && cnt < a->pointStride) a->point[b * a->pointStride + cnt] = t;
                cnt++;
            }
        }
        if (a->count) a->count[b] = cnt;
    }
    pickLaunches++;
    return AFX_OK;
}

int afxk_power_to_db(const float *in, int batch, long long length, long long stride, float min, float *out, void *stream) {
    (void)stream;
    if (!in || !out || batch <= 0 || batch > 65535 || length <= 0) return AFX_ERR_ARG;
    for (int b = 0; b < batch; b++)
        for (long long i = 0; i < length; i++) out[b * stride + i] = in[b * stride + i] + min;
    dbLaunches++;
    return AFX_OK;
}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            exit(1);                                               \
        }                                                          \
    } while (0)

static float *plane(size_t n) {
    float *x = (float *)malloc(sizeof(float) * n);
    CHECK(x);
    unsigned v = 4242u;
    for (size_t i = 0; i < n; i++) {
        v = v * 1664525u + 1013904223u;
        x[i] = (float)(v >> 8) / 16777216.f - 0.5f;
    }
    return x;
}

int main(void) {
    OnsetObj o = NULL;
    /* construction with every default, the pick parameters, debug print, release; NULL-safe calls */
    CHECK(onsetObj_new(&o, 30, 7, 0, NULL, NULL, NULL) == 0 && o);
    onsetObj_debug(o);
    onsetObj_free(o);
    onsetObj_free(NULL);
    onsetObj_debug(NULL);
    CHECK(onsetObj_new(NULL, 30, 7, 512, NULL, NULL, NULL) == -1);
    o = (OnsetObj)&sink;
    CHECK(onsetObj_new(&o, 0, 7, 512, NULL, NULL, NULL) == AFX_ERR_ARG && !o);
    CHECK(onsetObj_new(&o, 30, -2, 512, NULL, NULL, NULL) == AFX_ERR_ARG && !o);
    int pick[5];
    float delta = 0;
    CHECK(afx_onset_plan_host(0, 0, pick, &delta) == 0 && pick[0] == 1 && pick[1] == 1 && pick[2] == 6 && pick[3] == 7 && pick[4] == 1 &&
          delta == 0.07f);
    CHECK(afx_onset_plan_host(44100, 441, pick, NULL) == 0 && pick[0] == 3 && pick[2] == 10 && pick[3] == 11 && pick[4] == 3);
    CHECK(afx_onset_plan_host(32000, 1024, pick, NULL) == 0 && pick[0] == 0 && pick[4] == 0 && pick[2] == 3 && pick[3] == 4);
    CHECK(afx_onset_plan_host(32000, 512, NULL, NULL) == AFX_ERR_ARG);
    printf("onset construction, defaults, plan\n");

    /* host-pointer calls: exactly sized staging, the index table uploaded, replaced, reused, dropped; a phase kind */
    {
        const int T = 41, M = 9;
        float *x = plane((size_t)T * M), *ph = plane((size_t)T * M), *evn = plane(T), *evn2 = plane(T);
        int *pts = (int *)malloc(sizeof(int) * T);
        CHECK(pts);
        int order = 3, sr = 44100;
        NoveltyType type = Novelty_Flux;
        CHECK(onsetObj_new(&o, T, M, 441, &sr, &order, &type) == 0 && o);
        CHECK(onsetObj_onset(o, x, NULL, NULL, NULL, 0, evn, pts) == (T + 1) / 2 && pts[0] == 0 && pts[(T + 1) / 2 - 1] == T - 1);
        int idx1[] = {8, 0, 0, 3}, idx2[] = {1, 2, 3, 4, 5, 6, 7, 8, 0, 1, 2};
        const int d0 = descLaunches;
        CHECK(onsetObj_onset(o, x, NULL, NULL, idx1, 4, evn, pts) == (T + 1) / 2);
        CHECK(onsetObj_onset(o, x, NULL, NULL, idx2, 11, evn2, pts) == (T + 1) / 2);
        CHECK(onsetObj_onset(o, x, NULL, NULL, idx1, 4, evn2, pts) == (T + 1) / 2 && memcmp(evn, evn2, sizeof(float) * T) == 0);
        CHECK(descLaunches == d0 + 3 && filterLaunches >= 4);
        NoveltyParam par = {T + 1, 0.f, 1, 0, 0, 0.f, 0, 1.f};
        CHECK(onsetObj_onset(o, x, NULL, &par, NULL, 0, evn, pts) == AFX_ERR_ARG); /* step > nLength */
        par.step = T;
        CHECK(onsetObj_onset(o, x, NULL, &par, NULL, 0, evn, pts) >= 0);
        par.step = -4; /* -> 1 */
        CHECK(onsetObj_onset(o, x, NULL, &par, NULL, 0, evn, pts) >= 0);
        int bad1[] = {0, 9}, bad2[] = {-1};
        CHECK(onsetObj_onset(o, x, NULL, NULL, bad1, 2, evn, pts) == AFX_ERR_ARG);
        CHECK(onsetObj_onset(o, x, NULL, NULL, bad2, 1, evn, pts) == AFX_ERR_ARG);
        CHECK(onsetObj_onset(o, x, NULL, NULL, idx1, 0, evn, pts) == AFX_ERR_ARG);
        CHECK(onsetObj_onset(o, NULL, NULL, NULL, NULL, 0, evn, pts) == AFX_ERR_ARG);
        CHECK(onsetObj_onset(o, x, NULL, NULL, NULL, 0, NULL, pts) == AFX_ERR_ARG);
        CHECK(onsetObj_onset(NULL, x, NULL, NULL, NULL, 0, evn, pts) == AFX_ERR_ARG);
        onsetObj_debug(o);
        onsetObj_free(o);
        type = Novelty_NWPD;
        CHECK(onsetObj_new(&o, T, M, 441, &sr, NULL, &type) == 0 && o);
        CHECK(onsetObj_onset(o, x, NULL, NULL, NULL, 0, evn, pts) == AFX_ERR_ARG); /* a phase kind without the phase */
        CHECK(onsetObj_onset(o, x, ph, NULL, idx1, 4, evn, pts) == (T + 1) / 2);
        onsetObj_free(o);
        type = (NoveltyType)77; /* no named kind: flux */
        CHECK(onsetObj_new(&o, 1, 1, 441, &sr, NULL, &type) == 0 && o);
        CHECK(onsetObj_onset(o, x, NULL, NULL, NULL, 0, evn, pts) == 1 && pts[0] == 0);
        onsetObj_free(o);
        free(x);
        free(ph);
        free(evn);
        free(evn2);
        free(pts);
        printf("onset host-pointer calls, index tables, refusals\n");
    }

    /* batched calls: exactly sized buffers, strides, NULL outputs, chunks of whole clips == one pass */
    {
        const int T = 300, M = 512, B = 5, os = T + 3, ps = 7; /* 600 KB per clip */
        float *x = plane((size_t)B * T * M), *e1 = plane((size_t)(B - 1) * os + T), *e2 = plane((size_t)(B - 1) * os + T);
        int *p1 = (int *)malloc(sizeof(int) * B * ps), *c1 = (int *)malloc(sizeof(int) * B);
        CHECK(p1 && c1);
        int order = 2;
        CHECK(onsetObj_new(&o, T, M, 512, NULL, &order, NULL) == 0 && o);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, e1, p1, c1, os, ps, NULL) == 0);
        CHECK(maxFilterRows == (long long)B * T && c1[B - 1] == T / 2 && p1[(B - 1) * ps + ps - 1] == 2 * (ps - 1));
        CHECK(setenv("AFX_ONSET_CHUNK_MB", "1", 1) == 0); /* one clip per chunk */
        maxFilterRows = 0;
        const int f0 = filterLaunches;
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, e2, NULL, NULL, os, 0, NULL) == 0);
        CHECK(filterLaunches == f0 + B && maxFilterRows == T);
        for (int b = 0; b < B; b++) CHECK(memcmp(e1 + (size_t)b * os, e2 + (size_t)b * os, sizeof(float) * T) == 0);
        CHECK(unsetenv("AFX_ONSET_CHUNK_MB") == 0);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, e2, NULL, c1, os, 0, NULL) == 0);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, e2, p1, NULL, os, ps, NULL) == 0);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, e2, p1, c1, T - 1, ps, NULL) == AFX_ERR_ARG);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, e2, p1, c1, os, -1, NULL) == AFX_ERR_ARG);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, 0, NULL, NULL, 0, e2, p1, c1, os, ps, NULL) == AFX_ERR_ARG);
        CHECK(onsetObj_onsetBatchDevice(o, NULL, NULL, B, NULL, NULL, 0, e2, p1, c1, os, ps, NULL) == AFX_ERR_ARG);
        CHECK(onsetObj_onsetBatchDevice(o, x, NULL, B, NULL, NULL, 0, NULL, p1, c1, os, ps, NULL) == AFX_ERR_ARG);
        CHECK(onsetObj_onsetBatchDevice(NULL, x, NULL, B, NULL, NULL, 0, e2, p1, c1, os, ps, NULL) == AFX_ERR_ARG);
        onsetObj_free(o);
        free(x);
        free(e1);
        free(e2);
        free(p1);
        free(c1);
        printf("onset batched calls, chunks, argument errors\n");
    }

    /* the primitives */
    {
        const int n = 50;
        float *x = plane(3 * n), *y = plane(3 * n);
        int pts[12], cnt[3];
        CHECK(afx_maxFilterDevice(x, 3, n, 4, y, NULL) == 0 && afx_maxFilterDevice(x, 3, n, 4, x, NULL) == AFX_ERR_ARG);
        CHECK(afx_maxFilterDevice(x, 3, n, 0, y, NULL) == AFX_ERR_ARG && afx_maxFilterDevice(NULL, 3, n, 4, y, NULL) == AFX_ERR_ARG);
        CHECK(afx_peakPickDevice(x, 3, n - 2, n, 0, 1, 0, 1, 0, -1.f, pts, cnt, 4, NULL) == 0 && cnt[2] == (n - 1) / 2 && pts[11] == 6);
        CHECK(afx_peakPickDevice(x, 3, n, n, 0, 0, 0, 1, 0, 0.f, pts, cnt, 4, NULL) == AFX_ERR_ARG);
        CHECK(afx_peakPickDevice(x, 3, n, n, 0, 1, 0, 1, -1, 0.f, pts, cnt, 4, NULL) == AFX_ERR_ARG);
        CHECK(afx_peakPickDevice(x, 3, n, n - 1, 0, 1, 0, 1, 0, 0.f, pts, cnt, 4, NULL) == AFX_ERR_ARG);
        CHECK(afx_peakPickDevice(x, 3, n, n, 0, 1, 0, 1, 0, 0.f, NULL, NULL, 4, NULL) == AFX_ERR_ARG);
        CHECK(afx_powerToDbDevice(x, 3, n - 1, n, 3.f, y, NULL) == 0 && y[1] == x[1] - 80.f && afx_powerToDbDevice(x, 3, n, n, -20.f, x, NULL) == 0);
        CHECK(afx_powerToDbDevice(x, 3, n, n - 1, -80.f, y, NULL) == AFX_ERR_ARG && afx_powerToDbDevice(x, 0, n, n, -80.f, y, NULL) == AFX_ERR_ARG);
        const int d0 = dbLaunches;
        float *big = plane(70000 * 2);
        CHECK(afx_powerToDbDevice(big, 70000, 2, 2, -80.f, big, NULL) == 0 && dbLaunches == d0 + 2); /* more clips than a launch takes */
        const float before = y[5];
        util_powerToDB(y, 3 * n, -10.f, NULL);
        CHECK(y[5] == before - 10.f);
        util_powerToDB(y, 3 * n, 0.f, x);
        CHECK(x[5] == y[5] - 80.f);
        util_powerToDB(NULL, 5, 0.f, x);
        util_powerToDB(y, 0, 0.f, x);
        free(big);
        free(x);
        free(y);
        printf("onset primitives\n");
    }
    CHECK(pickLaunches > 10);
    printf("OK\n");
    return 0;
}
