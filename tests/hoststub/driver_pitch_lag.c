/* driver_pitch_lag.c -- the NCF and cepstrum pitch host objects under AddressSanitizer / UBSan, as a program of its own:
 * pitch{NCF,CEP}Obj_new / calTimeLength / pitch / pitchBatchDevice / curveBatchDevice / enableDebug / free and
 * afx_pitch_{ncf,cep}_plan_host against the generated stand-in of the device layer (gen_stub.py --omit=afxk_pitch_lag).
 * The launcher is supplied HERE: it does no transform but reads every entry of every table, every sample of every frame
 * and touches every output the kernel would, so a table or a staging buffer that is too small is a sanitizer report
 * ("device" buffers are exactly sized).  fre[t] is a checksum of frame t's samples: a streamed signal must reproduce the
 * one-call sequence exactly -- same frames, same take / keep sequence. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "mir/_pitch_cep.h"
#include "mir/_pitch_ncf.h"

static volatile float sink;
static int launches, lastMode, lastHadWindow;

int afxk_pitch_lag(const AfxPitchLagArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->x || !a->twiddle) return AFX_ERR_ARG;
    if (a->mode != AFX_PITCH_LAG_NCF && a->mode != AFX_PITCH_LAG_CEP) return AFX_ERR_ARG;
    const int N = 1 << a->radix2Exp, ncf = a->mode == AFX_PITCH_LAG_NCF;
    if (a->minIndex < (ncf ? 1 : 0) || a->maxIndex < a->minIndex || a->maxIndex > (ncf ? N - 1 : 2 * N - 1)) return AFX_ERR_ARG;
    if ((long long)(a->timeLength - 1) * a->hop + N > a->dataLength) return AFX_ERR_ARG;
    float s = 0;
    for (int n = 0; a->window && n < N; n++) s += a->window[n];
    for (int n = 0; n < 2 * N; n++) s += a->twiddle[n];
    launches++;
    lastMode = a->mode;
    lastHadWindow = a->window != NULL;
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

/* the two objects behind one set of calls */
typedef struct {
    const char *name;
    int mode, defaultWindow;
    int (*create)(void **, int *, float *, float *, int *, int *, WindowType *, int *);
    int (*frames)(void *, int);
    void (*pitch)(void *, float *, int, float *);
    int (*batch)(void *, const float *, int, int, long long, float *, float *, long long, void *);
    int (*curve)(void *, const float *, int, int, long long, float *, void *);
    void (*debug)(void *, int);
    void (*release)(void *);
    int (*minIndex)(void *);
    int (*maxIndex)(void *);
    int (*plan)(int *, float *, float *, int *, int *, WindowType *, int *, AfxPitchLagPlan *);
    void (*planFree)(AfxPitchLagPlan *);
} Kind;

#define WRAP(X, x)                                                                                                              \
    static int x##_create(void **o, int *sr, float *lo, float *hi, int *r, int *hop, WindowType *w, int *cont) {                \
        Pitch##X##Obj h = (Pitch##X##Obj)o; /* a non-NULL value the call must clear */                                          \
        const int st = pitch##X##Obj_new(&h, sr, lo, hi, r, hop, w, cont);                                                      \
        *o = h;                                                                                                                 \
        return st;                                                                                                              \
    }                                                                                                                           \
    static int x##_frames(void *o, int n) { return pitch##X##Obj_calTimeLength((Pitch##X##Obj)o, n); }                          \
    static void x##_pitch(void *o, float *d, int n, float *f) { pitch##X##Obj_pitch((Pitch##X##Obj)o, d, n, f); }               \
    static int x##_batch(void *o, const float *d, int b, int n, long long cs, float *f, float *v, long long os, void *s) {      \
        return pitch##X##Obj_pitchBatchDevice((Pitch##X##Obj)o, d, b, n, cs, f, v, os, s);                                      \
    }                                                                                                                           \
    static int x##_curve(void *o, const float *d, int b, int n, long long cs, float *c, void *s) {                              \
        return pitch##X##Obj_curveBatchDevice((Pitch##X##Obj)o, d, b, n, cs, c, s);                                             \
    }                                                                                                                           \
    static void x##_debug(void *o, int on) { pitch##X##Obj_enableDebug((Pitch##X##Obj)o, on); }                                 \
    static void x##_release(void *o) { pitch##X##Obj_free((Pitch##X##Obj)o); }                                                  \
    static int x##_min(void *o) { return pitch##X##Obj_minIndex((Pitch##X##Obj)o); }                                            \
    static int x##_max(void *o) { return pitch##X##Obj_maxIndex((Pitch##X##Obj)o); }
WRAP(NCF, ncf)
WRAP(CEP, cep)

static const Kind kinds[2] = {
    {"NCF", AFX_PITCH_LAG_NCF, (int)Window_Rect, ncf_create, ncf_frames, ncf_pitch, ncf_batch, ncf_curve, ncf_debug, ncf_release, ncf_min,
     ncf_max, afx_pitch_ncf_plan_host, afx_pitch_ncf_plan_free},
    {"CEP", AFX_PITCH_LAG_CEP, (int)Window_Hamm, cep_create, cep_frames, cep_pitch, cep_batch, cep_curve, cep_debug, cep_release, cep_min,
     cep_max, afx_pitch_cep_plan_host, afx_pitch_cep_plan_free},
};

/* one call against the signal in pieces: the same frames in the same order */
static void streaming(const Kind *k, int r, int hop) {
    const int N = 1 << r, n = N + hop * 11 + 29;
    float *x = signal(n);
    int sr = 16000, cont = 1;
    float lo = 260.f, hi = 2000.f; /* maxIndex 62: inside N = 64 */
    void *one = NULL, *obj = NULL;
    CHECK(k->create(&one, &sr, &lo, &hi, &r, &hop, NULL, NULL) == 0 && one);
    const int T = k->frames(one, n);
    CHECK(T == (n - N) / hop + 1);
    float *whole = (float *)malloc(sizeof(float) * (size_t)T), *got = (float *)malloc(sizeof(float) * (size_t)T);
    CHECK(whole && got);
    k->pitch(one, x, n, whole);
    k->release(one);
    CHECK(k->create(&obj, &sr, &lo, &hi, &r, &hop, NULL, &cont) == 0 && obj);
    const int pieces[] = {N / 3, 1, N + hop / 2, 7, 2 * N + hop + 5, 3 * hop, n};
    int at = 0, frames = 0;
    for (unsigned i = 0; i < sizeof pieces / sizeof *pieces && at < n; i++) {
        const int len = pieces[i] < n - at ? pieces[i] : n - at;
        const int t = k->frames(obj, len);
        CHECK(t >= 0 && frames + t <= T);
        k->pitch(obj, x + at, len, got + frames);
        frames += t;
        at += len;
    }
    CHECK(at == n && frames == T);
    CHECK(memcmp(whole, got, sizeof(float) * (size_t)T) == 0);
    float dummy[4];
    CHECK(k->batch(obj, x, 1, n, n, dummy, NULL, 4, NULL) == AFX_ERR_UNSUPPORTED);
    k->release(obj);
    free(whole);
    free(got);
    free(x);
    printf("pitch_lag %s streaming r %d hop %d: %d frames in pieces == one call\n", k->name, r, hop, T);
}

static void run(const Kind *k) {
    void *o = NULL;
    /* construction with every default, debug print, release; NULL-safe calls */
    CHECK(k->create(&o, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0 && o);
    CHECK(k->minIndex(o) == 16 && k->maxIndex(o) == 1000);
    CHECK(k->frames(o, 4095) == 0 && k->frames(o, 4096 + 1024) == 2);
    k->debug(o, 1);
    k->release(o);
    k->release(NULL);
    k->debug(NULL, 1);
    CHECK(k->frames(NULL, 100) == 0 && k->maxIndex(NULL) == 0 && k->minIndex(NULL) == 0);
    float one[1] = {0.f};
    k->pitch(NULL, one, 1, one); /* reported, no fault */
    /* refusals: radix2Exp, maxIndex beyond the last lag / quefrency, NULL handle pointer */
    int r = 5, sr = 8000;
    float lo = 32.f;
    CHECK(k->create(&o, NULL, NULL, NULL, &r, NULL, NULL, NULL) == -100 && !o);
    r = 13;
    CHECK(k->create(&o, NULL, NULL, NULL, &r, NULL, NULL, NULL) == -100 && !o);
    r = 6;
    CHECK(k->create(&o, &sr, &lo, NULL, &r, NULL, NULL, NULL) == AFX_ERR_ARG && !o); /* maxIndex 250 of N = 64 */
    CHECK(pitchNCFObj_new(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1 && pitchCEPObj_new(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
    {
        AfxPitchLagPlan p;
        CHECK(k->plan(&sr, &lo, NULL, &r, NULL, NULL, NULL, &p) == AFX_ERR_ARG);
        CHECK(p.maxIndex == 250 && p.minIndex == 4 && p.window && p.windowType == k->defaultWindow);
        k->planFree(&p);
        k->planFree(&p);
        r = 13;
        CHECK(k->plan(NULL, NULL, NULL, &r, NULL, NULL, NULL, &p) == -100 && !p.window);
        k->planFree(&p);
        CHECK(k->plan(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
        /* the LDS budget of every size the constructor accepts: two workgroups to a CU */
        for (r = AFX_PITCH_LAG_MIN_EXP; r <= AFX_PITCH_LAG_MAX_EXP; r++) {
            float low = 1000.f, high = 3000.f;
            WindowType w = Window_Bartlett;
            CHECK(k->plan(NULL, &low, &high, &r, NULL, &w, NULL, &p) == 0);
            CHECK(p.ldsBytes == afx_pitch_lag_lds_bytes(r) && p.ldsBytes <= 80 * 1024 && p.lagLength == 2 << r && p.maxIndex == 32 &&
                  p.minIndex == 11 && p.windowType == (k->mode == AFX_PITCH_LAG_NCF ? (int)Window_Bartlett : (int)Window_Hamm));
            k->planFree(&p);
        }
    }
    printf("pitch_lag %s construction, defaults, refusals, plans\n", k->name);

    streaming(k, 6, 16);
    streaming(k, 6, 40);
    streaming(k, 6, 100); /* hop above fftLength: samples to skip carry over */
    streaming(k, 6, 700);

    /* batched calls: exactly sized buffers, argument errors, the short clip; Rect uploads no window table */
    {
        int rr = 9, hop = 128, srr = 16000;
        const int n = 512 + 128 * 5 + 5, clips = 3, stride = n + 12;
        float *x = signal(clips * stride - 12); /* the last clip ends with its data */
        WindowType rect = Window_Rect, hann = Window_Hann;
        CHECK(k->create(&o, &srr, NULL, NULL, &rr, &hop, &rect, NULL) == 0 && o);
        const int T = k->frames(o, n);
        float *f = (float *)malloc(sizeof(float) * (size_t)((clips - 1) * (T + 2) + T));
        float *cv = (float *)malloc(sizeof(float) * (size_t)clips * T * (k->maxIndex(o) + 1));
        CHECK(f && cv && k->maxIndex(o) == 500);
        CHECK(k->batch(o, x, clips, n, stride, f, NULL, T + 2, NULL) == 0);
        CHECK(lastMode == k->mode && !lastHadWindow);
        CHECK(k->curve(o, x, clips, n, stride, cv, NULL) == 0);
        CHECK(k->batch(o, x, clips, n, stride, NULL, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(k->batch(o, NULL, clips, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(k->batch(NULL, x, clips, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(k->batch(o, x, 0, n, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(k->batch(o, x, clips, -1, stride, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(k->batch(o, x, clips, n, n - 1, f, NULL, T, NULL) == AFX_ERR_ARG);
        CHECK(k->batch(o, x, clips, n, stride, f, NULL, T - 1, NULL) == AFX_ERR_ARG);
        CHECK(k->curve(o, x, clips, n, stride, NULL, NULL) == AFX_ERR_ARG);
        const int launched = launches;
        CHECK(k->batch(o, x, 1, 511, stride, f, NULL, 1, NULL) == 0 && launches == launched);
        k->release(o);
        CHECK(k->create(&o, &srr, NULL, NULL, &rr, &hop, &hann, NULL) == 0 && o);
        CHECK(k->batch(o, x, clips, n, stride, f, NULL, T + 2, NULL) == 0 && lastHadWindow);
        k->release(o);
        free(f);
        free(cv);
        free(x);
        printf("pitch_lag %s batched calls, argument errors, window tables\n", k->name);
    }

    /* device memory does not grow with the frame count beyond the staged samples and one float per frame: 1100 frames at
     * the default size run through the exactly sized staging buffers, then a short call reuses them */
    {
        int rr = 12, hop = 64;
        const int few = 4096 + 64 * 6, many = 4096 + 64 * 1099;
        float *x = signal(many), *f = (float *)malloc(sizeof(float) * 1100);
        CHECK(f);
        CHECK(k->create(&o, NULL, NULL, NULL, &rr, &hop, NULL, NULL) == 0 && o);
        k->pitch(o, x, few, f);
        k->pitch(o, x, many, f);
        k->pitch(o, x, few, f);
        k->release(o);
        free(f);
        free(x);
        printf("pitch_lag %s staging of 7, 1100 and 7 frames at the default size\n", k->name);
    }
}

int main(void) {
    run(&kinds[0]);
    run(&kinds[1]);
    printf("OK\n");
    return 0;
}
