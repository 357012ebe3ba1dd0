/* driver_resample.c -- the resampler host object under AddressSanitizer / UBSan, as a program of its own: resampleObj_new /
 * newWithWindow / calDataLength / setSamplate / setSamplateRatio / enableContinue / resample / resampleBatchDevice / debug /
 * free and the afx_resample_plan_* functions against the generated stand-in of the device layer (gen_stub.py
 * --omit=afxk_resample).  The launcher is supplied HERE: per output it walks the taps the kernel walks -- the same table
 * entries (and each one's neighbour), the same samples -- and stores the float32 sum, so a table, a staging buffer or an
 * output row that is too small is a sanitizer report ("device" buffers are exactly sized).  It also states the phase
 * arithmetic of the reference loop verbatim and requires afx_resample_phase (afx_device.h) to give the same integers. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "dsp/resample_algorithm.h"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            exit(1);                                               \
        }                                                          \
    } while (0)

static int launches, lastInLds, lastGroup;
static long long lastTaps;

int afxk_resample(const AfxResampleArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->x || !a->out || !a->table) return AFX_ERR_ARG;
    if (a->batch <= 0 || a->sourceLength <= 0 || a->targetLength <= 0) return AFX_ERR_ARG;
    if (a->batch > 1 && (a->clipStride < a->sourceLength || a->outStride < a->targetLength)) return AFX_ERR_ARG;
    AfxResampleLaunch l;
    const int st = afx_resample_launch_plan(a->batch, a->ratio, a->bitLength, a->interpLength, &l);
    if (st != AFX_OK) return st;
    CHECK(l.ldsBytes <= AFX_RESAMPLE_LDS_BUDGET && l.group >= 1 && l.group <= AFX_RESAMPLE_GROUP);
    const int L = a->interpLength, S = a->sourceLength, bitLength = a->bitLength;
    CHECK(a->table[L] == a->table[L - 1]); /* the repeated last entry: the difference table ends in 0 */
    const float ratio = a->ratio;
    const float scale = afx_resample_scale(ratio);
    const int step = afx_resample_step(ratio, bitLength);
    launches++;
    lastInLds = l.tableInLds;
    lastGroup = l.group;
    lastTaps = 0;
    for (int b = 0; b < a->batch; b++) {
        const float *x = a->x + (long long)b * a->clipStride;
        float *out = a->out + (long long)b * a->outStride;
        for (int i = 0; i < a->targetLength; i++) {
            const AfxResamplePhase p = afx_resample_phase(i, ratio, scale, bitLength);
            /* resample_algorithm.c:483-507, verbatim */
            float t = i * 1.0 / ratio;
            int n = floorf(t);
            float factor = scale * (t - n);
            float factorValue = factor * bitLength;
            int offset = floorf(factorValue);
            float delta = factorValue - offset;
            CHECK(p.n == n && p.offL == offset && p.deltaL == delta);
            factor = scale - factor;
            factorValue = factor * bitLength;
            offset = floorf(factorValue);
            delta = factorValue - offset;
            CHECK(p.offR == offset && p.deltaR == delta);
            float acc = 0;
            int count = (L - p.offL) / step;
            if (n + 1 < count) count = n + 1;
            for (int j = n - (S - 1) > 0 ? n - (S - 1) : 0; j < count; j++) {
                const int o = p.offL + j * step;
                acc += (a->table[o] + p.deltaL * (a->table[o + 1] - a->table[o])) * x[n - j];
                lastTaps++;
            }
            count = (L - p.offR) / step;
            if (S - n - 1 < count) count = S - n - 1;
            for (int j = 0; j < count; j++) {
                const int o = p.offR + j * step;
                acc += (a->table[o] + p.deltaR * (a->table[o + 1] - a->table[o])) * x[n + 1 + j];
                lastTaps++;
            }
            out[i] = acc / a->outScale;
        }
    }
    return AFX_OK;
}

static float *signal(int n) {
    float *x = (float *)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
    CHECK(x);
    unsigned v = 12345u;
    for (int i = 0; i < n; i++) {
        v = v * 1664525u + 1013904223u;
        x[i] = (float)(v >> 8) / 16777216.f - 0.5f;
    }
    return x;
}

/* resample into an exactly sized buffer (plus a guard value behind it): the length */
static int run(ResampleObj o, float *x, int n, float **out) {
    const int m = resampleObj_calDataLength(o, n);
    float *y = (float *)malloc(sizeof(float) * ((size_t)m + 1));
    CHECK(y);
    for (int i = 0; i <= m; i++) y[i] = 9.f;
    CHECK(resampleObj_resample(o, x, n, y) == m);
    CHECK(y[m] == 9.f);
    if (out) *out = y;
    else free(y);
    return m;
}

int main(void) {
    float *x = signal(200000);

    /* 1. construct / free: the three qualities, window tables in and above LDS, the plan of each */
    for (int q = 0; q < 3; q++) {
        ResampleQualityType qt = (ResampleQualityType)q;
        int scale = q & 1;
        ResampleObj o = (ResampleObj)x; /* a non-NULL value the call must replace */
        CHECK(resampleObj_new(&o, &qt, &scale, NULL) == 0 && o);
        AfxResamplePlan p;
        CHECK(afx_resample_plan_host(&qt, NULL, NULL, NULL, NULL, NULL, &scale, NULL, &p) == 0);
        CHECK(p.zeroNum == 64 >> q && p.interpLength == (64 >> q) * 512 + 1 && p.ratio == 0.5f && p.p == 1 && p.q == 2);
        CHECK(p.tableInLds == 1 && p.step == 256 && p.isScale == scale);
        CHECK(resampleObj_calDataLength(o, 4001) == 2000 && afx_resample_plan_length(&p, 4001) == 2000);
        CHECK(run(o, x, 4001, NULL) == 2000 && lastInLds == 1 && lastGroup == 1);
        resampleObj_debug(o);
        resampleObj_free(o);
        afx_resample_plan_free(&p);
        afx_resample_plan_free(&p);
        printf("resample quality %d: table of %d entries, born at ratio 0.5\n", q, (64 >> q) * 512 + 1);
    }
    {
        int zero = 80, nbit = 9, small = 16, nb5 = 5;
        WindowType hann = Window_Hann, gauss = Window_Gauss, tukey = Window_Tukey, kaiser = Window_Kaiser;
        float v = 3.f, a = 0.4f, zeroValue = 0.f, ro = 0.9f;
        ResampleObj o = NULL;
        CHECK(resampleObj_newWithWindow(&o, &zero, &nbit, &hann, NULL, NULL, NULL, NULL) == 0 && o);
        resampleObj_setSamplate(o, 44100, 16000);
        CHECK(run(o, x, 3000, NULL) == 1088 && lastInLds == 0); /* 40961 entries: read from global memory */
        resampleObj_free(o);
        WindowType *types[4] = {&hann, &gauss, &tukey, &kaiser};
        float *values[4] = {NULL, &v, &a, &zeroValue};
        for (int k = 0; k < 4; k++) {
            CHECK(resampleObj_newWithWindow(&o, &small, &nb5, types[k], values[k], &ro, NULL, NULL) == 0 && o);
            resampleObj_setSamplate(o, 48000, 16000);
            CHECK(run(o, x, 999, NULL) == 333 && lastInLds == 1);
            resampleObj_free(o);
        }
        for (int t = -2; t <= (int)Window_Tukey + 1; t++) { /* every window type, and values around the enum */
            WindowType wt = (WindowType)t;
            CHECK(resampleObj_newWithWindow(&o, &small, &nb5, &wt, NULL, NULL, NULL, NULL) == 0 && o);
            CHECK(run(o, x, 100, NULL) == 50);
            resampleObj_free(o);
        }
        resampleObj_free(NULL);
        printf("resample windows: Hann 80 x 2^9 from global memory, Hann / Gauss / Tukey / Kaiser 16 x 2^5, every type\n");
    }

    /* 2. the ratio sequence on one object: lengths, p / q through the plan, the table uploaded again each time */
    {
        ResampleObj o = NULL;
        CHECK(resampleObj_new(&o, NULL, NULL, NULL) == 0 && o);
        const int before = launches;
        CHECK(run(o, x, 3000, NULL) == 1500);
        resampleObj_setSamplate(o, 44100, 16000);
        CHECK(run(o, x, 3000, NULL) == 1088);
        resampleObj_setSamplate(o, 44100, 44100); /* ignored */
        resampleObj_setSamplate(o, 0, 16000);
        resampleObj_setSamplate(o, 16000, -3);
        CHECK(resampleObj_calDataLength(o, 3000) == 1088);
        resampleObj_setSamplate(o, 16000, 32000);
        CHECK(run(o, x, 3000, NULL) == 6000);
        resampleObj_setSamplateRatio(o, -1.f); /* ignored */
        CHECK(resampleObj_calDataLength(o, 3000) == 6000);
        resampleObj_setSamplateRatio(o, 0.7123f);
        CHECK(run(o, x, 3000, NULL) == 2136);
        resampleObj_setSamplateRatio(o, 3.7f);
        CHECK(run(o, x, 1, NULL) == 3);
        CHECK(launches == before + 5);
        resampleObj_free(o);
        printf("resample ratio sequence: 0.5 -> 16000/44100 -> 2 -> 0.7123 -> 3.7, ignored settings in between\n");
    }

    /* 3. streaming in pieces with a growing q: (n - n %% q) p / q outputs, nothing carried */
    {
        int cont = 1;
        ResampleObj o = NULL;
        CHECK(resampleObj_new(&o, NULL, NULL, &cont) == 0 && o);
        const int rates[3][2] = {{32000, 16000}, {48000, 44100}, {44100, 16000}}; /* q = 2, 160, 441 */
        const int pq[3][2] = {{1, 2}, {147, 160}, {160, 441}};
        const int pieces[6] = {1000, 37, 4411, 1, 440, 882};
        for (int r = 0; r < 3; r++) {
            if (r) resampleObj_setSamplate(o, rates[r][0], rates[r][1]);
            int at = 0;
            for (int k = 0; k < 6; k++) {
                const int n = pieces[k], want = (n - n % pq[r][1]) * pq[r][0] / pq[r][1];
                CHECK(resampleObj_calDataLength(o, n) == want);
                CHECK(run(o, x + at, n, NULL) == want);
                at += n;
            }
        }
        float y[8];
        CHECK(resampleObj_resampleBatchDevice(o, x, 1, 1000, 1000, y, 1000, NULL) == AFX_ERR_UNSUPPORTED);
        resampleObj_setSamplate(o, 16000, 32000); /* q = 1: nothing */
        CHECK(resampleObj_calDataLength(o, 1000) == 0 && resampleObj_resample(o, x, 1000, y) == 0);
        resampleObj_setSamplateRatio(o, 0.4f); /* q = 0: nothing */
        CHECK(resampleObj_calDataLength(o, 1000) == 0 && resampleObj_resample(o, x, 1000, y) == 0);
        resampleObj_enableContinue(o, 0);
        CHECK(run(o, x, 1000, NULL) == 400);
        resampleObj_free(o);
        printf("resample streaming: pieces of 1000 / 37 / 4411 / 1 / 440 / 882 samples at q = 2, 160, 441; q <= 1 gives nothing\n");
    }

    /* 4. refusals */
    {
        ResampleObj o = (ResampleObj)x;
        int zero = 1 << 16, nbit = 9;
        float y[64];
        CHECK(resampleObj_newWithWindow(&o, &zero, &nbit, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_UNSUPPORTED && !o);
        CHECK(resampleObj_new(NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
        AfxResamplePlan p;
        CHECK(afx_resample_plan_host(NULL, &zero, &nbit, NULL, NULL, NULL, NULL, NULL, &p) == AFX_ERR_UNSUPPORTED && !p.table);
        afx_resample_plan_free(&p);
        CHECK(afx_resample_plan_rate(NULL, 1, 2, 0.f) == AFX_ERR_ARG && afx_resample_plan_length(NULL, 5) == 0);
        CHECK(resampleObj_new(&o, NULL, NULL, NULL) == 0 && o);
        const int errs = afxdev_error_count();
        CHECK(resampleObj_resample(NULL, x, 10, y) == AFX_ERR_ARG && resampleObj_resample(o, NULL, 10, y) == AFX_ERR_ARG);
        CHECK(resampleObj_resample(o, x, 10, NULL) == AFX_ERR_ARG && resampleObj_resample(o, x, 0, y) == AFX_ERR_ARG);
        CHECK(resampleObj_resample(o, x, -4, y) == AFX_ERR_ARG && afxdev_error_count() >= errs + 5);
        CHECK(resampleObj_calDataLength(NULL, 10) == 0 && resampleObj_calDataLength(o, 0) == 0 && resampleObj_calDataLength(o, -1) == 0);
        CHECK(resampleObj_resampleBatchDevice(NULL, x, 1, 10, 10, y, 10, NULL) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, NULL, 1, 10, 10, y, 10, NULL) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, x, 1, 10, 10, NULL, 10, NULL) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, x, 0, 10, 10, y, 10, NULL) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, x, 2, 10, 9, y, 10, NULL) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, x, 2, 10, 10, y, 4, NULL) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, x, 2, 1, 10, y, 0, NULL) == 0);
        resampleObj_setSamplateRatio(o, 0.001f); /* less than one table entry per tap */
        CHECK(resampleObj_calDataLength(o, 100000) == 100 && resampleObj_resample(o, x, 100000, y) == AFX_ERR_ARG);
        CHECK(resampleObj_resampleBatchDevice(o, x, 1, 100000, 100000, y, 100, NULL) == AFX_ERR_ARG);
        resampleObj_setSamplateRatio(o, 0.f);
        CHECK(resampleObj_resample(o, x, 1000, y) == 0);
        resampleObj_setSamplateRatio(o, 1e9f); /* beyond an int of outputs */
        CHECK(resampleObj_resample(o, x, 1000, y) == AFX_ERR_ARG && resampleObj_calDataLength(o, 1000) == 0);
        resampleObj_setSamplate(NULL, 1, 2);
        resampleObj_setSamplateRatio(NULL, 1.f);
        resampleObj_enableContinue(NULL, 1);
        resampleObj_debug(NULL);
        resampleObj_free(o);
        printf("resample refusals: NULL and non-positive arguments, short strides, the table cap, ratios without a step\n");
    }

    /* 5. staging-buffer growth: short, long, short, longer; up-sampling makes the output buffer the larger one */
    {
        ResampleQualityType fast = ResampleQuality_Fast;
        ResampleObj o = NULL;
        CHECK(resampleObj_new(&o, &fast, NULL, NULL) == 0 && o);
        resampleObj_setSamplate(o, 44100, 16000);
        const int sizes[6] = {100, 150000, 40, 1, 199990, 3};
        for (int k = 0; k < 6; k++) CHECK(run(o, x + k, sizes[k], NULL) == (int)floorf(sizes[k] * (16000 / (float)44100)));
        resampleObj_setSamplate(o, 16000, 44100);
        CHECK(run(o, x, 50000, NULL) == 137812 && run(o, x, 7, NULL) == 19);
        CHECK(lastTaps > 0);
        resampleObj_free(o);
        printf("resample staging: calls of 100 / 150000 / 40 / 1 / 199990 / 3 samples down, 50000 / 7 up on one object\n");
    }

    /* 6. the batch: rows at strides above their lengths are the single calls bit for bit, padding untouched */
    {
        ResampleQualityType mid = ResampleQuality_Mid;
        int scale = 1;
        ResampleObj o = NULL;
        CHECK(resampleObj_new(&o, &mid, &scale, NULL) == 0 && o);
        resampleObj_setSamplate(o, 44100, 16000);
        const int clips = 5, n = 1500, cs = 1517, m = 544, os = 549;
        float *y = (float *)malloc(sizeof(float) * (size_t)(clips * os));
        CHECK(y);
        for (int i = 0; i < clips * os; i++) y[i] = 7.5f;
        CHECK(resampleObj_resampleBatchDevice(o, x, clips, n, cs, y, os, NULL) == m && lastGroup == AFX_RESAMPLE_GROUP);
        for (int c = 0; c < clips; c++) {
            float *one = NULL;
            CHECK(run(o, x + c * cs, n, &one) == m);
            CHECK(memcmp(one, y + c * os, sizeof(float) * (size_t)m) == 0);
            for (int i = m; i < os; i++) CHECK(y[c * os + i] == 7.5f);
            free(one);
        }
        free(y);
        resampleObj_free(o);
        printf("resample batch: 5 clips of 1500 samples every 1517 into rows of 549: bitwise the single calls\n");
    }
    free(x);
    printf("OK\n");
    return 0;
}
