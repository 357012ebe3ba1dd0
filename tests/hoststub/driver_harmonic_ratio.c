/* driver_harmonic_ratio.c -- the harmonic-ratio host object under AddressSanitizer / UBSan, as a program of its own:
 * harmonicRatioObj_new / calTimeLength / harmonicRatio / harmonicRatioBatchDevice / curveBatchDevice / free and
 * afx_harmonic_ratio_plan_host against the generated stand-in of the device layer (gen_stub.py --omit=afxk_harmonic_ratio).
 * The launcher is supplied HERE: it does no transform but reads every entry of every table, every sample of every frame,
 * writes every word of the scratch and touches every output the kernels would, so a table, a scratch or a staging buffer
 * that is too small is a sanitizer report ("device" buffers are exactly sized).  value[t] is a checksum of frame t's
 * samples. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "mir/harmonicRatio_algorithm.h"

static volatile float sink;
static int launches, lastMaxLength;

int afxk_harmonic_ratio(const AfxHarmonicRatioArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->x || !a->window || !a->twiddle || !a->scratch) return AFX_ERR_ARG;
    const int N = 1 << a->radix2Exp;
    if (a->maxLength < 2 || a->maxLength > N - 1) return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    float s = 0;
    for (int n = 0; n < N; n++) s += a->window[n];
    for (int n = 0; n < 2 * N; n++) s += a->twiddle[n];
    const long long rows = (long long)a->batch * a->timeLength;
    for (long long i = 0; i < afx_harmonic_ratio_scratch_ints(rows); i++) a->scratch[i] = (int)i;
    launches++;
    lastMaxLength = a->maxLength;
    for (int b = 0; b < a->batch; b++)
        for (int t = 0; t < a->timeLength; t++) {
            const float *x = a->x + (long long)b * a->clipStride + (long long)t * a->hop;
            double c = 0;
            for (int n = 0; n < N; n++) c += (double)x[n] * (n + 1);
            const long long row = (long long)b * a->timeLength + t, at = (long long)b * a->outStride + t;
            if (a->value) a->value[at] = (float)c;
            if (a->lag) a->lag[at] = 2;
            if (a->first) a->first[at] = 1;
            for (int k = 0; a->curve && k < a->maxLength; k++) a->curve[row * a->maxLength + k] = 3.f;
        }
    sink = s;
    return AFX_OK;
}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            exit(1);                                               \
        }                                                          \
    } while (0)

static float *signal(int n) {
    float *x = (float *)malloc(sizeof(float) * (size_t)n);
    CHECK(x);
    unsigned v = 12345u;
    for (int i = 0; i < n; i++) {
        v = v * 1664525u + 1013904223u;
        x[i] = (float)(v >> 8) / 16777216.f - 0.5f;
    }
    return x;
}

int main(void) {
    HarmonicRatioObj o = (HarmonicRatioObj)&sink; /* a non-NULL value the call must clear */
    /* construction with every default (window 2048), the wrapper's size, release; NULL-safe calls */
    CHECK(harmonicRatioObj_new(&o, NULL, NULL, NULL, NULL, NULL) == 0 && o);
    CHECK(harmonicRatioObj_windowLength(o) == 2048 && harmonicRatioObj_maxLength(o) == 1280);
    CHECK(harmonicRatioObj_calTimeLength(o, 2047) == 0 && harmonicRatioObj_calTimeLength(o, 2048 + 512) == 2);
    harmonicRatioObj_free(o);
    int r = 12;
    CHECK(harmonicRatioObj_new(&o, NULL, NULL, &r, NULL, NULL) == 0 && o && harmonicRatioObj_windowLength(o) == 4096);
    harmonicRatioObj_free(o);
    harmonicRatioObj_free(NULL);
    CHECK(harmonicRatioObj_calTimeLength(NULL, 100) == 0 && harmonicRatioObj_maxLength(NULL) == 0 && harmonicRatioObj_windowLength(NULL) == 0);
    float one[1] = {0.f};
    const int before = afxdev_error_count();
    harmonicRatioObj_harmonicRatio(NULL, one, 1, one); /* reported, no fault */
    CHECK(afxdev_error_count() > before);
    /* refusals */
    o = (HarmonicRatioObj)&sink;
    r = 5;
    CHECK(harmonicRatioObj_new(&o, NULL, NULL, &r, NULL, NULL) == -100 && !o);
    r = 13;
    CHECK(harmonicRatioObj_new(&o, NULL, NULL, &r, NULL, NULL) == -100 && !o);
    CHECK(harmonicRatioObj_new(NULL, NULL, NULL, NULL, NULL, NULL) == -1);
    {
        AfxHarmonicRatioPlan p;
        CHECK(afx_harmonic_ratio_plan_host(NULL, NULL, &r, NULL, NULL, &p) == -100 && !p.window);
        afx_harmonic_ratio_plan_free(&p);
        CHECK(afx_harmonic_ratio_plan_host(NULL, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
        for (r = AFX_PITCH_LAG_MIN_EXP; r <= AFX_PITCH_LAG_MAX_EXP; r++) {
            float low = 1000.f;
            WindowType w = Window_Bartlett;
            CHECK(afx_harmonic_ratio_plan_host(NULL, &low, &r, &w, NULL, &p) == 0);
            CHECK(p.ldsBytes == afx_pitch_lag_lds_bytes(r) && p.ldsBytes <= 80 * 1024 && p.fftLength == 2 << r && p.windowLength == 1 << r &&
                  p.maxLength == 32 && p.slideLength == (1 << r) / 4 && p.window);
            afx_harmonic_ratio_plan_free(&p);
            afx_harmonic_ratio_plan_free(&p);
        }
    }
    printf("harmonic_ratio construction, defaults, refusals, plans\n");

    /* host-pointer calls of different lengths on one object: NULL output, fewer samples than a window, long / short / long */
    {
        int rr = 8, hop = 64, sr = 16000;
        float lo = 64.f;
        const int few = 256 + 64 * 6, many = 256 + 64 * 1099;
        float *x = signal(many), *f = (float *)malloc(sizeof(float) * 1100);
        CHECK(f);
        CHECK(harmonicRatioObj_new(&o, &sr, &lo, &rr, NULL, &hop) == 0 && o && harmonicRatioObj_maxLength(o) == 250);
        const int launched = launches;
        f[0] = 5.f;
        harmonicRatioObj_harmonicRatio(o, x, 255, f); /* writes nothing, launches nothing */
        CHECK(f[0] == 5.f && launches == launched);
        const int errs = afxdev_error_count();
        harmonicRatioObj_harmonicRatio(o, x, few, NULL); /* reported */
        CHECK(afxdev_error_count() > errs && launches == launched);
        harmonicRatioObj_harmonicRatio(o, NULL, few, f);
        harmonicRatioObj_harmonicRatio(o, x, 0, f);
        CHECK(launches == launched);
        harmonicRatioObj_harmonicRatio(o, x, few, f);
        double c = 0;
        for (int n = 0; n < 256; n++) c += (double)x[64 * 6 + n] * (n + 1);
        CHECK(launches == launched + 1 && lastMaxLength == 250 && f[6] == (float)c);
        harmonicRatioObj_harmonicRatio(o, x, many, f);
        harmonicRatioObj_harmonicRatio(o, x + 3, few, f);
        CHECK(launches == launched + 3 && harmonicRatioObj_calTimeLength(o, many) == 1100);
        harmonicRatioObj_free(o);
        free(f);
        free(x);
        printf("harmonic_ratio host-pointer calls of 0, 7, 1100 and 7 frames, NULL output\n");
    }

    /* batched calls: exactly sized buffers, optional outputs, argument errors, the short clip */
    {
        int rr = 9, hop = 128, sr = 16000;
        const int n = 512 + 128 * 5 + 5, clips = 3, stride = n + 12;
        float *x = signal(clips * stride - 12); /* the last clip ends with its data */
        CHECK(harmonicRatioObj_new(&o, &sr, NULL, &rr, NULL, &hop) == 0 && o);
        const int T = harmonicRatioObj_calTimeLength(o, n), mx = harmonicRatioObj_maxLength(o);
        CHECK(T == 6 && mx == 511);
        const size_t outs = (size_t)((clips - 1) * (T + 2) + T);
        float *v = (float *)malloc(sizeof(float) * outs), *cv = (float *)malloc(sizeof(float) * (size_t)clips * T * mx);
        int *lag = (int *)malloc(sizeof(int) * outs), *first = (int *)malloc(sizeof(int) * outs);
        CHECK(v && cv && lag && first);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, clips, n, stride, v, lag, first, T + 2, NULL) == 0);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, clips, n, stride, v, NULL, NULL, T + 2, NULL) == 0);
        CHECK(harmonicRatioObj_curveBatchDevice(o, x, clips, n, stride, cv, NULL) == 0);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, clips, n, stride, NULL, lag, first, T, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, NULL, clips, n, stride, v, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(NULL, x, clips, n, stride, v, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, 0, n, stride, v, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, clips, -1, stride, v, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, clips, n, n - 1, v, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, clips, n, stride, v, NULL, NULL, T - 1, NULL) == AFX_ERR_ARG);
        CHECK(harmonicRatioObj_curveBatchDevice(o, x, clips, n, stride, NULL, NULL) == AFX_ERR_ARG);
        const int launched = launches;
        CHECK(harmonicRatioObj_harmonicRatioBatchDevice(o, x, 1, 511, stride, v, NULL, NULL, 1, NULL) == 0 && launches == launched);
        harmonicRatioObj_free(o);
        free(v);
        free(cv);
        free(lag);
        free(first);
        free(x);
        printf("harmonic_ratio batched calls, optional outputs, argument errors\n");
    }
    printf("OK\n");
    return 0;
}
