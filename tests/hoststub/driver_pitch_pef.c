/* driver_pitch_pef.c -- the PEF pitch host object under AddressSanitizer / UBSan, as a program of its own:
 * pitchPEFObj_new / calTimeLength / setFilterParams / pitch / pitchBatchDevice / curveBatchDevice / free and
 * afx_pitch_pef_plan_host against the generated stand-in of the device layer (gen_stub.py --omit=afxk_pitch_pef).  The
 * launcher is supplied HERE: it does no transform but reads every entry of every table, every sample of every frame and
 * touches every output the kernel would, so a table or a staging buffer that is too small is a sanitizer report ("device"
 * buffers are exactly sized).  fre[t] is a checksum of frame t's samples: a streamed signal must reproduce the one-call
 * sequence exactly -- same frames, same take / keep sequence. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "mir/_pitch_pef.h"

static volatile float sink;
static int launches;
static float lastTableSum;

int afxk_pitch_pef(const AfxPitchPefArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->x || !a->window || !a->twiddle || !a->taps || !a->filterSpec || !a->lg) return AFX_ERR_ARG;
    const int N = 1 << a->radix2Exp;
    if (a->minIndex < 0 || a->maxIndex < a->minIndex || a->maxIndex >= 2 * N || a->filterPadNum < 0 || a->filterPadNum > N)
        return AFX_ERR_ARG;
    if (((size_t)a->taps & 15) != 0 || a->pwLength < 2 || a->pwLength > N + 1) return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    float s = 0;
    for (int n = 0; n < N; n++) s += a->window[n];
    for (int n = 0; n < 4 * N; n++) s += a->twiddle[n];
    for (int m = 0; m < 2 * N; m++) {
        if (a->taps[m].index < -1 || a->taps[m].index >= N) return AFX_ERR_ARG;
        if ((a->taps[m].index < 0 ? N + 1 : a->taps[m].index + 2) > a->pwLength) return AFX_ERR_ARG; /* a bin the kernel would not keep */
        s += a->taps[m].dx + a->taps[m].dl + a->taps[m].bw + a->lg[m];
    }
    for (int k = 0; k < 2 * (2 * N + 1); k++) s += a->filterSpec[k];
    lastTableSum = s;
    launches++;
    for (int b = 0; b < a->batch; b++)
        for (int t = 0; t < a->timeLength; t++) {
            const float *x = a->x + (long long)b * a->clipStride + (long long)t * a->hop;
            double c = 0;
            for (int n = 0; n < N; n++) c += (double)x[n] * (n + 1);
            const long long row = (long long)b * a->timeLength + t;
            if (a->fre) a->fre[(long long)b * a->outStride + t] = (float)c;
            if (a->value) a->value[(long long)b * a->outStride + t] = 2.f;
            for (int k = 0; a->curve && k <= a->maxIndex; k++) a->curve[row * (a->maxIndex + 1) + k] = 3.f;
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

/* one call against the signal in pieces: the same frames in the same order */
static void streaming(int r, int hop) {
    const int N = 1 << r, n = N + hop * 11 + 29;
    float *x = signal(n);
    int sr = 16000, cont = 1;
    float lo = 60.f, hi = 2000.f;
    PitchPEFObj one = NULL, obj = NULL;
    CHECK(pitchPEFObj_new(&one, &sr, &lo, &hi, NULL, &r, &hop, NULL, NULL, NULL, NULL, NULL) == 0 && one);
    const int T = pitchPEFObj_calTimeLength(one, n);
    CHECK(T == (n - N) / hop + 1);
    float *whole = (float *)malloc(sizeof(float) * (size_t)T), *got = (float *)malloc(sizeof(float) * (size_t)T);
    CHECK(whole && got);
    pitchPEFObj_pitch(one, x, n, whole);
    pitchPEFObj_free(one);
    CHECK(pitchPEFObj_new(&obj, &sr, &lo, &hi, NULL, &r, &hop, NULL, NULL, NULL, NULL, &cont) == 0 && obj);
    const int pieces[] = {N / 3, 1, N + hop / 2, 7, 2 * N + hop + 5, 3 * hop, n};
    int at = 0, frames = 0;
    for (unsigned i = 0; i < sizeof pieces / sizeof *pieces && at < n; i++) {
        const int len = pieces[i] < n - at ? pieces[i] : n - at;
        const int t = pitchPEFObj_calTimeLength(obj, len);
        CHECK(t >= 0 && frames + t <= T);
        pitchPEFObj_pitch(obj, x + at, len, got + frames);
        frames += t;
        at += len;
    }
    CHECK(at == n && frames == T);
    CHECK(memcmp(whole, got, sizeof(float) * (size_t)T) == 0);
    float dummy[4];
    CHECK(pitchPEFObj_pitchBatchDevice(obj, x, 1, n, n, dummy, NULL, 4, NULL) == AFX_ERR_UNSUPPORTED);
    pitchPEFObj_free(obj);
    free(whole);
    free(got);
    free(x);
    printf("pitch_pef streaming r %d hop %d: %d frames in pieces == one call\n", r, hop, T);
}

int main(void) {
    PitchPEFObj o = NULL;
    /* construction with every default, debug print, release; NULL-safe calls */
    CHECK(pitchPEFObj_new(&o, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 && o);
    CHECK(pitchPEFObj_minIndex(o) == 1590 && pitchPEFObj_maxIndex(o) == 7243 && pitchPEFObj_filterPadNum(o) == 933 &&
          pitchPEFObj_logLength(o) == 8192);
    CHECK(pitchPEFObj_calTimeLength(o, 4095) == 0 && pitchPEFObj_calTimeLength(o, 4096 + 1024) == 2);
    pitchPEFObj_enableDebug(o, 1);
    pitchPEFObj_free(o);
    pitchPEFObj_free(NULL);
    pitchPEFObj_setFilterParams(NULL, 1.f, 1.f, 2.f);
    CHECK(pitchPEFObj_calTimeLength(NULL, 100) == 0 && pitchPEFObj_maxIndex(NULL) == 0);
    /* refusals: radix2Exp, an empty candidate range, highFre at the last log frequency, NULL handle pointer */
    int r = 5, sr = 16000;
    float lo = 100.f, hi = 100.5f, cut = 100.5f;
    o = (PitchPEFObj)&r;
    CHECK(pitchPEFObj_new(&o, NULL, NULL, NULL, NULL, &r, NULL, NULL, NULL, NULL, NULL, NULL) == -100 && !o);
    r = 13;
    CHECK(pitchPEFObj_new(&o, NULL, NULL, NULL, NULL, &r, NULL, NULL, NULL, NULL, NULL, NULL) == -100 && !o);
    r = 6;
    CHECK(pitchPEFObj_new(&o, &sr, &lo, &hi, NULL, &r, NULL, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_ARG && !o);
    r = 9, hi = 2000.f, cut = 2000.f;
    CHECK(pitchPEFObj_new(&o, &sr, &lo, &hi, &cut, &r, NULL, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_ARG && !o);
    CHECK(pitchPEFObj_new(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
    {
        AfxPitchPefPlan p;
        CHECK(afx_pitch_pef_plan_host(&sr, &lo, &hi, &cut, &r, NULL, NULL, NULL, NULL, NULL, NULL, &p) == AFX_ERR_ARG);
        CHECK(p.maxIndex == 0 && p.lg && p.h);
        afx_pitch_pef_plan_free(&p);
        afx_pitch_pef_plan_free(&p);
        r = 13;
        CHECK(afx_pitch_pef_plan_host(NULL, NULL, NULL, NULL, &r, NULL, NULL, NULL, NULL, NULL, NULL, &p) == -100 && !p.lg);
        afx_pitch_pef_plan_free(&p);
        CHECK(afx_pitch_pef_plan_host(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
        /* the LDS budget of every size the constructor accepts */
        for (r = AFX_PITCH_PEF_MIN_EXP; r <= AFX_PITCH_PEF_MAX_EXP; r++) {
            float beta = 1.f;
            CHECK(afx_pitch_pef_plan_host(NULL, NULL, NULL, NULL, &r, NULL, NULL, NULL, &beta, NULL, NULL, &p) == 0);
            CHECK(p.ldsBytes == afx_pitch_pef_lds_bytes(r, p.pwLength) && p.ldsBytes <= 160 * 1024 && p.corrLength == 4 << r &&
                  p.pwLength >= (1 << r) / 4 + 1 && p.pwLength <= (1 << r) / 4 + 2 && afx_pitch_pef_lds_bytes(r, (1 << r) + 1) <= 160 * 1024 &&
                  p.filterPadNum == 0 && p.refXcorrLength == 4 << r);
            afx_pitch_pef_plan_free(&p);
        }
        CHECK(afx_pitch_pef_lds_bytes(13, 8193) > 160 * 1024); /* a plan that reads every bin would not fit */
    }
    printf("pitch_pef construction, defaults, refusals, plans\n");

    streaming(8, 64);
    streaming(8, 100);
    streaming(8, 300); /* hop above fftLength: samples to skip carry over */
    streaming(6, 700);

    /* batched calls: exactly sized buffers, argument errors, the short clip; setFilterParams leaves the tables alone */
    {
        int rr = 9, hop = 128, srr = 16000;
        const int n = 512 + 128 * 5 + 5, clips = 3, stride = n + 12;
        float *x = signal(clips * stride - 12); /* the last clip ends with its data */
        CHECK(pitchPEFObj_new(&o, &srr, NULL, NULL, NULL, &rr, &hop, NULL, NULL, NULL, NULL, NULL) == 0 && o);
        const int T = pitchPEFObj_calTimeLength(o, n);
        float *f = (float *)malloc(sizeof(float) * (size_t)((clips - 1) * (T + 2) + T));
        float *cv = (float *)malloc(sizeof(float) * (size_t)clips * T * (pitchPEFObj_maxIndex(o) + 1));
        CHECK(f && cv);
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, clips, n, stride, f, NULL, T + 2, NULL) == 0);
        const float before = lastTableSum;
        pitchPEFObj_setFilterParams(o, 5.f, 0.7f, 2.5f);
        pitchPEFObj_setFilterParams(o, -1.f, 0.7f, 2.5f);
        CHECK(pitchPEFObj_curveBatchDevice(o, x, clips, n, stride, cv, NULL) == 0);
        CHECK(lastTableSum == before && pitchPEFObj_filterPadNum(o) == 117);
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, clips, n, stride, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(pitchPEFObj_pitchBatchDevice(o, NULL, clips, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, 0, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, clips, -1, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, clips, n, n - 1, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, clips, n, stride, f, NULL, T - 1, NULL) == AFX_ERR_ARG);
        CHECK(pitchPEFObj_curveBatchDevice(o, x, clips, n, stride, NULL, NULL) == AFX_ERR_ARG);
        const int launched = launches;
        CHECK(pitchPEFObj_pitchBatchDevice(o, x, 1, 511, stride, f, NULL, 1, NULL) == 0 && launches == launched);
        pitchPEFObj_free(o);
        free(f);
        free(cv);
        free(x);
        printf("pitch_pef batched calls, argument errors, setFilterParams\n");
    }

    /* device memory does not grow with the frame count beyond the staged samples and one float per frame: 1100 frames at
     * the default size run through the exactly sized staging buffers, then a short call reuses them */
    {
        int rr = 12, hop = 64;
        const int few = 4096 + 64 * 6, many = 4096 + 64 * 1099;
        float *x = signal(many), *f = (float *)malloc(sizeof(float) * 1100);
        CHECK(f);
        CHECK(pitchPEFObj_new(&o, NULL, NULL, NULL, NULL, &rr, &hop, NULL, NULL, NULL, NULL, NULL) == 0 && o);
        pitchPEFObj_pitch(o, x, few, f);
        pitchPEFObj_pitch(o, x, many, f);
        pitchPEFObj_pitch(o, x, few, f);
        pitchPEFObj_free(o);
        free(f);
        free(x);
        printf("pitch_pef staging of 7, 1100 and 7 frames at the default size\n");
    }
    printf("OK\n");
    return 0;
}
