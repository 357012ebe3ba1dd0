/* driver_pitch_hs.c -- the HPS / LHS pitch host object under AddressSanitizer / UBSan, as a program of its own:
 * pitch{HPS,LHS}Obj_new / calTimeLength / pitch / pitchBatchDevice / curveBatchDevice / free against the generated stand-in
 * of the device layer (gen_stub.py --omit=afxk_pitch_hs).  The launcher is supplied HERE: it does no transform but reads
 * every table, every sample of every frame and touches every output and the whole scratch slice of every workgroup the
 * kernel would use, so a table, a staging buffer or a scratch reservation that is too small is a sanitizer report
 * ("device" buffers are exactly sized).  fre[t] is a checksum of frame t's samples: a streamed signal must reproduce the
 * one-call sequence exactly -- same frames, same take / keep sequence. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "mir/_pitch_hps.h"
#include "mir/_pitch_lhs.h"

static volatile float sink;
static int launches, lastGroups;
static long long lastSliceFloats;

int afxk_pitch_hs(const AfxPitchHsArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->x || !a->window || !a->twiddle || !a->roots) return AFX_ERR_ARG;
    const int N = 1 << a->radix2Exp;
    const long long M = 1LL << a->interpExp, rows = (long long)a->batch * a->timeLength;
    const long long lastBin = (long long)a->maxIndex * a->harmonicCount, sf = afx_pitch_hs_slice_floats(lastBin);
    if (lastBin >= M || (long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    float s = 0;
    for (int n = 0; n < N; n++) s += a->window[n] + a->twiddle[n];
    for (long long m = 0; m < 2 * M; m++) s += a->roots[m];
    launches++;
    lastGroups = a->slice ? a->groups : 0;
    lastSliceFloats = a->slice ? sf : 0;
    if (a->slice) {
        if (a->groups < 1 || a->groups > AFX_PITCH_HS_SCRATCH_GROUPS || a->groups > rows) return AFX_ERR_ARG;
        for (long long i = 0; i < (long long)a->groups * sf; i++) a->slice[i] = 1.f;
    } else if (afx_pitch_hs_lds_fixed(a->radix2Exp) + 4 * sf > AFX_PITCH_HS_LDS_BUDGET) {
        return AFX_ERR_ARG;
    }
    for (int b = 0; b < a->batch; b++)
        for (int t = 0; t < a->timeLength; t++) {
            const float *x = a->x + (long long)b * a->clipStride + (long long)t * a->hop;
            double c = 0;
            for (int n = 0; n < N; n++) c += (double)x[n] * (n + 1);
            const long long row = (long long)b * a->timeLength + t;
            if (a->fre) a->fre[(long long)b * a->outStride + t] = (float)c;
            if (a->value) a->value[(long long)b * a->outStride + t] = 2.f;
            for (int j = 0; a->curve && j <= a->maxIndex; j++) a->curve[row * (a->maxIndex + 1) + j] = 3.f;
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

typedef struct OpaquePitchHS *Obj;
typedef struct {
    const char *name;
    int (*create)(Obj *, int *, float *, float *, int *, int *, WindowType *, int *, int *);
    int (*frames)(Obj, int);
    void (*pitch)(Obj, float *, int, float *);
    void (*debug)(Obj, int);
    void (*release)(Obj);
    int (*batch)(Obj, const float *, int, int, long long, float *, float *, long long, void *);
    int (*curve)(Obj, const float *, int, int, long long, float *, void *);
    int (*maxIndex)(Obj);
    int (*count)(Obj);
} Api;
static const Api API[2] = {
    {"HPS", pitchHPSObj_new, pitchHPSObj_calTimeLength, pitchHPSObj_pitch, pitchHPSObj_enableDebug, pitchHPSObj_free,
     pitchHPSObj_pitchBatchDevice, pitchHPSObj_curveBatchDevice, pitchHPSObj_maxIndex, pitchHPSObj_harmonicCount},
    {"LHS", pitchLHSObj_new, pitchLHSObj_calTimeLength, pitchLHSObj_pitch, pitchLHSObj_enableDebug, pitchLHSObj_free,
     pitchLHSObj_pitchBatchDevice, pitchLHSObj_curveBatchDevice, pitchLHSObj_maxIndex, pitchLHSObj_harmonicCount},
};

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
static void streaming(const Api *api, int r, int hop) {
    const int N = 1 << r, n = N + hop * 11 + 29;
    float *x = signal(n);
    int sr = 16000, count = 3, cont = 1;
    float lo = 60.f, hi = 2000.f;
    Obj one = NULL, obj = NULL;
    CHECK(api->create(&one, &sr, &lo, &hi, &r, &hop, NULL, &count, NULL) == 0 && one);
    const int T = api->frames(one, n);
    CHECK(T == (n - N) / hop + 1);
    float *whole = (float *)malloc(sizeof(float) * (size_t)T), *got = (float *)malloc(sizeof(float) * (size_t)T);
    CHECK(whole && got);
    api->pitch(one, x, n, whole);
    api->release(one);
    CHECK(api->create(&obj, &sr, &lo, &hi, &r, &hop, NULL, &count, &cont) == 0 && obj);
    const int pieces[] = {N / 3, 1, N + hop / 2, 7, 2 * N + hop + 5, 3 * hop, n};
    int at = 0, frames = 0;
    for (unsigned i = 0; i < sizeof pieces / sizeof *pieces && at < n; i++) {
        const int len = pieces[i] < n - at ? pieces[i] : n - at;
        const int t = api->frames(obj, len);
        CHECK(t >= 0 && frames + t <= T);
        api->pitch(obj, x + at, len, got + frames);
        frames += t;
        at += len;
    }
    CHECK(at == n && frames == T);
    CHECK(memcmp(whole, got, sizeof(float) * (size_t)T) == 0);
    float dummy[4];
    CHECK(api->batch(obj, x, 1, n, n, dummy, NULL, 4, NULL) == AFX_ERR_UNSUPPORTED);
    api->release(obj);
    free(whole);
    free(got);
    free(x);
    printf("pitch_hs %s streaming r %d hop %d: %d frames in pieces == one call\n", api->name, r, hop, T);
}

int main(void) {
    for (int k = 0; k < 2; k++) {
        const Api *api = &API[k];
        Obj o = NULL;
        /* construction with every default, debug print, release; NULL-safe calls */
        CHECK(api->create(&o, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 && o);
        CHECK(api->maxIndex(o) == 2000 && api->count(o) == 5 && api->frames(o, 4095) == 0 && api->frames(o, 4096 + 1024) == 2);
        api->debug(o, 1);
        api->release(o);
        api->release(NULL);
        CHECK(api->frames(NULL, 100) == 0);
        /* refusals: radix2Exp, fftLength above M, bins beyond M, NULL handle pointer */
        int r = 5, sr = 2000, one = 1, five = 5;
        float hi = 900.f;
        o = (Obj)&r;
        CHECK(api->create(&o, NULL, NULL, NULL, &r, NULL, NULL, NULL, NULL) == -100 && !o);
        r = 12;
        CHECK(api->create(&o, &sr, NULL, &hi, &r, NULL, NULL, &one, NULL) == AFX_ERR_ARG && !o);
        sr = 44100, hi = 8000.f, r = 10;
        CHECK(api->create(&o, &sr, NULL, &hi, &r, NULL, NULL, &five, NULL) == AFX_ERR_ARG && !o);
        CHECK(api->create(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
        printf("pitch_hs %s construction, defaults, refusals\n", api->name);

        streaming(api, 8, 64);
        streaming(api, 8, 100);
        streaming(api, 8, 300); /* hop above fftLength: samples to skip carry over */
        streaming(api, 6, 700);

        /* batched calls: exactly sized buffers, argument errors, the short clip */
        {
            int rr = 9, hop = 128, srr = 16000, cnt = 4;
            const int n = 512 + 128 * 5 + 5, clips = 3, stride = n + 12;
            float *x = signal(clips * stride - 12); /* the last clip ends with its data */
            CHECK(api->create(&o, &srr, NULL, NULL, &rr, &hop, NULL, &cnt, NULL) == 0 && o);
            const int T = api->frames(o, n);
            float *f = (float *)malloc(sizeof(float) * (size_t)((clips - 1) * (T + 2) + T));
            float *cv = (float *)malloc(sizeof(float) * (size_t)clips * T * (api->maxIndex(o) + 1));
            CHECK(f && cv);
            CHECK(api->batch(o, x, clips, n, stride, f, NULL, T + 2, NULL) == 0);
            CHECK(api->curve(o, x, clips, n, stride, cv, NULL) == 0);
            CHECK(api->batch(o, x, clips, n, stride, NULL, NULL, T, NULL) == AFX_ERR_ARG);
            CHECK(api->batch(o, NULL, clips, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
            CHECK(api->batch(o, x, 0, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
            CHECK(api->batch(o, x, clips, -1, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
            CHECK(api->batch(o, x, clips, n, n - 1, f, NULL, T, NULL) == AFX_ERR_ARG);
            CHECK(api->batch(o, x, clips, n, stride, f, NULL, T - 1, NULL) == AFX_ERR_ARG);
            CHECK(api->curve(o, x, clips, n, stride, NULL, NULL) == AFX_ERR_ARG);
            const int before = launches;
            CHECK(api->batch(o, x, 1, 511, stride, f, NULL, 1, NULL) == 0 && launches == before);
            api->release(o);
            free(f);
            free(cv);
            free(x);
            printf("pitch_hs %s batched calls and argument errors\n", api->name);
        }

        /* the plan whose slice lives in scratch: one slice per workgroup, at most AFX_PITCH_HS_SCRATCH_GROUPS of them */
        {
            int rr = 12, hop = 64, srr = 32000, cnt = 2;
            float hi2 = 15000.f;
            AfxPitchHsPlan p;
            CHECK(afx_pitch_hs_plan_host(k, &srr, NULL, &hi2, &rr, &hop, NULL, &cnt, NULL, &p) == 0);
            CHECK(!p.sliceInLds && p.lastBin == 30000 && p.sliceFloats == afx_pitch_hs_slice_floats(30000));
            CHECK(api->create(&o, &srr, NULL, &hi2, &rr, &hop, NULL, &cnt, NULL) == 0 && o);
            const int few = 4096 + 64 * 6, many = 4096 + 64 * 1099;
            float *x = signal(many), *f = (float *)malloc(sizeof(float) * 1100);
            CHECK(f);
            api->pitch(o, x, few, f);
            CHECK(lastGroups == 7 && lastSliceFloats == p.sliceFloats);
            CHECK(api->batch(o, x, 1, many, many, f, NULL, 1100, NULL) == 0);
            CHECK(lastGroups == AFX_PITCH_HS_SCRATCH_GROUPS);
            api->pitch(o, x, few, f); /* the grown scratch is kept */
            CHECK(lastGroups == 7);
            api->release(o);
            free(f);
            free(x);
            printf("pitch_hs %s scratch slices: 7 and %d workgroups of %lld floats\n", api->name, AFX_PITCH_HS_SCRATCH_GROUPS,
                   p.sliceFloats);
        }
    }
    printf("OK\n");
    return 0;
}
