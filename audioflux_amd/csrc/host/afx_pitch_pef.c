/* afx_pitch_pef.c -- the pitch-estimation-filter tracker object (C host side) behind include/mir/_pitch_pef.h.
 *
 * Mirrors the parameter semantics of the reference object (src/mir/_pitch_pef.c:106-231, :428-522, :696-785): the tables
 * are built in the reference's float32 arithmetic and operation order, bit for bit.  Execution: ONE kernel launch per call
 * (k_pitch_pef, afx_pitch_pef.hip) from the samples to the frequency per frame.  The host-pointer call is the batch of one
 * through staging buffers and carries the isContinue tail (afx_frametail.h).  Device memory: the tables, uploaded once, and
 * the staged samples / frequencies of the host-pointer call -- nothing scales with timeLength * N.  There is no CPU
 * compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "afx_frametail.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/_pitch_pef.h"

/* __vlogspace (flux_vector.c:2164-2173) */
static float *logspace(float start, float stop, int length) {
    float *arr = afx_linspace(start, stop, length, 0);
    if (!arr) return NULL;
    for (int i = 0; i < length; i++) arr[i] = powf(10, arr[i]);
    return arr;
}

/* __vsum (flux_vector.c:1493-1501): accumulated in double, returned as float */
static float vsum(const float *v, int length) {
    double s = 0;
    for (int i = 0; i < length; i++) s += v[i];
    return (float)s;
}

void afx_pitch_pef_plan_free(AfxPitchPefPlan *p) {
    if (!p) return;
    free(p->lg);
    free(p->bw);
    free(p->h);
    free(p->window);
    p->lg = p->bw = p->h = p->window = NULL;
}

static AfxPitchPefTap *pef_taps(const AfxPitchPefPlan *p);

/* bins of the power spectrum the interpolation reads: up to the last tap's index + 1; all N + 1 when a log frequency
 * lies past the last linear one.  0: out of memory */
static int pef_pw_length(const AfxPitchPefPlan *p) {
    AfxPitchPefTap *taps = pef_taps(p);
    if (!taps) return 0;
    int len = 2;
    for (int m = 0; m < 2 * p->fftLength; m++) {
        const int need = taps[m].index < 0 ? p->fftLength + 1 : taps[m].index + 2;
        if (need > len) len = need;
    }
    free(taps);
    return len;
}

/* defaults, fallbacks, tables and refusals of the constructor: needs no device */
static int pef_plan(const int *samplate, const float *lowFre, const float *highFre, const float *cutFre, const int *radix2Exp,
                    const int *slideLength, const WindowType *windowType, const float *alpha, const float *beta,
                    const float *gamma, const int *isContinue, AfxPitchPefPlan *p) {
    memset(p, 0, sizeof(*p));
    p->samplate = 32000;
    p->lowFre = 32.f;
    p->highFre = 2000.f;
    p->cutFre = 4000.f;
    p->radix2Exp = 12;
    p->windowType = (int)Window_Hamm;
    p->alpha = 10.f;
    p->beta = 0.5f;
    p->gamma = 1.8f;
    if (samplate && *samplate > 0 && *samplate <= 196000) p->samplate = *samplate;
    if (lowFre && *lowFre >= 27) p->lowFre = *lowFre;
    if (highFre) {
        if (*highFre > p->lowFre && *highFre < p->samplate / 2) {
            p->highFre = *highFre;
        } else {
            p->lowFre = 32.f;
            p->highFre = 2000.f;
        }
    }
    if (cutFre) p->cutFre = *cutFre >= p->highFre ? *cutFre : p->highFre;
    if (radix2Exp) {
        if (*radix2Exp < AFX_PITCH_PEF_MIN_EXP || *radix2Exp > AFX_PITCH_PEF_MAX_EXP) return -100;
        p->radix2Exp = *radix2Exp;
    }
    if (windowType) p->windowType = (int)*windowType;
    if (alpha && *alpha > 0) p->alpha = *alpha;
    if (beta && *beta > 0) p->beta = *beta;
    if (gamma && *gamma > 1) p->gamma = *gamma;
    const int N = p->fftLength = 1 << p->radix2Exp;
    p->slideLength = (slideLength && *slideLength > 0) ? *slideLength : N / 4;
    p->isContinue = isContinue ? *isContinue : 0;
    p->logLength = 2 * N;
    p->corrLength = 4 * N;

    /* __pitchPEFObj_initData (:428-522) */
    p->window = afx_window_fft((WindowType)p->windowType, N);
    const float fre1 = p->samplate / 2 > p->cutFre ? p->cutFre : p->samplate / 2 - 1;
    p->lg = logspace(1, log10f(fre1), 2 * N);
    p->bw = (float *)calloc((size_t)2 * N, sizeof(float));
    p->h = (float *)calloc((size_t)N, sizeof(float));
    if (!p->window || !p->lg || !p->bw || !p->h) {
        afx_pitch_pef_plan_free(p);
        return AFX_ERR_NOMEM;
    }
    const float *lg = p->lg;
    int minIndex = -1, maxIndex = 0;
    for (int i = 1; i < 2 * N; i++) {
        if (p->highFre < lg[i]) {
            maxIndex = lg[i] - p->highFre < p->highFre - lg[i - 1] ? i : i - 1;
            break;
        }
        if (minIndex != -1) continue;
        if (p->lowFre < lg[i]) minIndex = lg[i] - p->lowFre < p->lowFre - lg[i - 1] ? i : i - 1;
    }
    p->minIndex = minIndex;
    p->maxIndex = maxIndex;
    for (int i = 2, j = 1; i < 2 * N; i++, j++) p->bw[j] = (lg[i] - lg[i - 2]) / (2 * N * 2);
    p->bw[0] = p->bw[1];
    p->bw[2 * N - 1] = p->bw[2 * N - 2];

    p->pwLength = pef_pw_length(p);
    if (!p->pwLength) {
        afx_pitch_pef_plan_free(p);
        return AFX_ERR_NOMEM;
    }
    p->ldsBytes = afx_pitch_pef_lds_bytes(p->radix2Exp, p->pwLength);

    /* __pitchPEFObj_calEstimateFilter (:696-785) */
    float *q = logspace(log10f(p->beta), log10f(p->alpha + p->beta), N);
    float *d = (float *)calloc((size_t)N + 1, sizeof(float));
    if (!q || !d) {
        free(q);
        free(d);
        afx_pitch_pef_plan_free(p);
        return AFX_ERR_NOMEM;
    }
    int pad = 0;
    for (int i = 0; i < N; i++) {
        if (q[i] < 1) pad++;
        p->h[i] = 1 / (p->gamma - cosf(2 * M_PI * q[i]));
    }
    d[0] = q[0];
    for (int i = 1; i < N; i++) d[i] = (q[i - 1] + q[i]) / 2;
    d[N] = q[N - 1];
    for (int i = 1; i < N + 1; i++) d[i - 1] = d[i] - d[i - 1];
    const float value1 = vsum(d, N);
    for (int i = 0; i < N; i++) d[i] *= p->h[i];
    const float value2 = vsum(d, N);
    const float det = value2 / value1;
    for (int i = 0; i < N; i++) p->h[i] = p->h[i] - det;
    free(q);
    free(d);
    p->filterPadNum = pad;
    p->refXcorrLength = pad ? 8 * N : 4 * N;

    /* where the reference reads out of bounds (the header's deviations) */
    if (minIndex < 0 || maxIndex <= minIndex) {
        afxdev_set_error("pitchPEFObj_new: lowFre %g / highFre %g / cutFre %g give the candidate range %d ... %d of the %d log "
                         "frequencies", p->lowFre, p->highFre, p->cutFre, minIndex, maxIndex, 2 * N);
        return AFX_ERR_ARG;
    }
    if (maxIndex + 1 > 2 * N + pad - 1) {
        afxdev_set_error("pitchPEFObj_new: maxIndex %d beyond the %d correlation lags", maxIndex, 2 * N + pad - 1);
        return AFX_ERR_ARG;
    }
    return 0;
}

int afx_pitch_pef_plan_host(int *samplate, float *lowFre, float *highFre, float *cutFre, int *radix2Exp, int *slideLength,
                            WindowType *windowType, float *alpha, float *beta, float *gamma, int *isContinue,
                            AfxPitchPefPlan *plan) {
    if (!plan) return AFX_ERR_ARG;
    return pef_plan(samplate, lowFre, highFre, cutFre, radix2Exp, slideLength, windowType, alpha, beta, gamma, isContinue, plan);
}

/* the operands of __vinterp_linear (flux_vectorOp.c:580-610) per log frequency, its walk over the linear grid included */
static AfxPitchPefTap *pef_taps(const AfxPitchPefPlan *p) {
    const int N = p->fftLength;
    float *lin = afx_linspace(0, p->samplate / 2, N + 1, 0);
    AfxPitchPefTap *taps = (AfxPitchPefTap *)calloc((size_t)2 * N, sizeof(*taps));
    if (!lin || !taps) {
        free(lin);
        free(taps);
        return NULL;
    }
    int index1 = 0;
    for (int m = 0; m < 2 * N; m++) {
        while (index1 < N && p->lg[m] > lin[index1 + 1]) index1++;
        if (index1 < N) {
            taps[m].index = index1;
            taps[m].dx = p->lg[m] - lin[index1];
            taps[m].dl = lin[index1 + 1] - lin[index1];
        } else {
            taps[m].index = -1;
            taps[m].dl = 1.f;
        }
        taps[m].bw = p->bw[m];
    }
    free(lin);
    return taps;
}

/* conj of the 4N-point spectrum of the zero-padded filter, bins 0 ... 2N, times the 1 / 2N of the 2N-point inverse:
 * evaluated in double, rounded once */
static float *pef_filter_spec(const AfxPitchPefPlan *p) {
    const int N = p->fftLength;
    double *re = (double *)calloc((size_t)4 * N, sizeof(double)), *im = (double *)calloc((size_t)4 * N, sizeof(double));
    float *g = (float *)malloc(sizeof(float) * 2 * ((size_t)2 * N + 1));
    int ok = re && im && g;
    if (ok) {
        for (int i = 0; i < N; i++) re[i] = p->h[i];
        ok = afx_fft_f64(p->radix2Exp + 2, re, im, 0) == 0;
    }
    if (ok) {
        const double scale = 1.0 / (2.0 * N);
        for (int k = 0; k <= 2 * N; k++) {
            g[2 * k] = (float)(re[k] * scale);
            g[2 * k + 1] = (float)(-im[k] * scale);
        }
    } else {
        free(g);
        g = NULL;
    }
    free(re);
    free(im);
    return g;
}

static void pef_free(struct OpaquePitchPEF *o) {
    if (!o) return;
    afx_pitch_head_sync(&o->head);
    afxdev_free(o->dWindow);
    afxdev_free(o->dTwiddle);
    afxdev_free(o->dTaps);
    afxdev_free(o->dFilterSpec);
    afxdev_free(o->dLg);
    afx_pitch_head_release(&o->head);
    free(o);
}

int pitchPEFObj_new(PitchPEFObj *pitchPEFObj, int *samplate, float *lowFre, float *highFre, float *cutFre, int *radix2Exp,
                    int *slideLength, WindowType *windowType, float *alpha, float *beta, float *gamma, int *isContinue) {
    if (!pitchPEFObj) return -1;
    *pitchPEFObj = NULL;
    AfxPitchPefPlan p;
    int st = pef_plan(samplate, lowFre, highFre, cutFre, radix2Exp, slideLength, windowType, alpha, beta, gamma, isContinue, &p);
    if (st == 0) st = afxdev_ensure();
    if (st != AFX_OK) {
        afx_pitch_pef_plan_free(&p);
        return st;
    }
    struct OpaquePitchPEF *o = (struct OpaquePitchPEF *)calloc(1, sizeof(*o));
    if (!o) {
        afx_pitch_pef_plan_free(&p);
        return AFX_ERR_NOMEM;
    }
    o->minIndex = p.minIndex;
    o->maxIndex = p.maxIndex;
    o->filterPadNum = p.filterPadNum;
    o->pwLength = p.pwLength;
    o->lowFre = p.lowFre;
    o->highFre = p.highFre;
    o->cutFre = p.cutFre;
    o->alpha = p.alpha;
    o->beta = p.beta;
    o->gamma = p.gamma;
    o->windowType = (WindowType)p.windowType;
    st = afx_pitch_head_init(&o->head, p.radix2Exp, p.slideLength, p.samplate, p.isContinue);
    const size_t N = (size_t)p.fftLength;
    float *tw = NULL, *spec = NULL;
    AfxPitchPefTap *taps = NULL;
    if (st == AFX_OK) {
        tw = afx_twiddle_table(4 * p.fftLength);
        taps = pef_taps(&p);
        spec = pef_filter_spec(&p);
        if (!tw || !taps || !spec) st = AFX_ERR_NOMEM;
    }
    const size_t specB = sizeof(float) * 2 * (2 * N + 1);
    st = afx_pitch_table(st, &o->dWindow, p.window, sizeof(float) * N, o->head.stream);
    st = afx_pitch_table(st, &o->dTwiddle, tw, sizeof(float) * 4 * N, o->head.stream);
    st = afx_pitch_table(st, &o->dTaps, taps, sizeof(*taps) * 2 * N, o->head.stream);
    st = afx_pitch_table(st, &o->dFilterSpec, spec, specB, o->head.stream);
    st = afx_pitch_table(st, &o->dLg, p.lg, sizeof(float) * 2 * N, o->head.stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->head.stream);
    free(tw);
    free(taps);
    free(spec);
    afx_pitch_pef_plan_free(&p);
    if (st != AFX_OK) {
        pef_free(o);
        return st;
    }
    *pitchPEFObj = o;
    return 0;
}

/* one launch over `batch` clips */
static int pef_run(void *ctx, const float *dData, int batch, int dataLength, long long clipStride, int T, float *dFre, float *dValue,
                   long long outStride, float *dCurve, void *stream) {
    const struct OpaquePitchPEF *o = (const struct OpaquePitchPEF *)ctx;
    AfxPitchPefArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dData;
    a.clipStride = clipStride;
    a.batch = batch;
    a.dataLength = dataLength;
    a.timeLength = T;
    a.radix2Exp = o->head.radix2Exp;
    a.hop = o->head.slideLength;
    a.minIndex = o->minIndex;
    a.maxIndex = o->maxIndex;
    a.filterPadNum = o->filterPadNum;
    a.pwLength = o->pwLength;
    a.window = o->dWindow;
    a.twiddle = o->dTwiddle;
    a.taps = (const AfxPitchPefTap *)o->dTaps;
    a.filterSpec = o->dFilterSpec;
    a.lg = o->dLg;
    a.fre = dFre;
    a.value = dValue;
    a.outStride = outStride;
    a.curve = dCurve;
    return afxk_pitch_pef(&a, stream);
}

int pitchPEFObj_pitchBatchDevice(PitchPEFObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dFre,
                                 float *dValue, long long outStride, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "pitchPEFObj", dData, batch, dataLength, clipStride, dFre, hipStream, &T);
    if (go <= 0) return go;
    if (outStride < T) return AFX_ERR_ARG;
    return pef_run(o, dData, batch, dataLength, clipStride, T, dFre, dValue, outStride, NULL, hipStream);
}

int pitchPEFObj_curveBatchDevice(PitchPEFObj o, const float *dData, int batch, int dataLength, long long clipStride,
                                 float *dCurve, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "pitchPEFObj", dData, batch, dataLength, clipStride, dCurve, hipStream, &T);
    if (go <= 0) return go;
    return pef_run(o, dData, batch, dataLength, clipStride, T, NULL, NULL, 0, dCurve, hipStream);
}

void pitchPEFObj_pitch(PitchPEFObj o, float *dataArr, int dataLength, float *freArr) {
    afx_pitch_call(AFX_PITCH_HEAD(o), dataArr, dataLength, freArr, pef_run, o, "pitchPEFObj_pitch");
}

int pitchPEFObj_calTimeLength(PitchPEFObj o, int dataLength) { return afx_pitch_frames(AFX_PITCH_HEAD(o), dataLength); }

/* _pitch_pef.c:685-694: the reference validates, then rebuilds the filter from the values it STORED at construction: no
 * observable change, so none here */
void pitchPEFObj_setFilterParams(PitchPEFObj o, float alpha, float beta, float gamma) {
    if (!o || !(alpha > 0 && beta > 0 && gamma > 1)) return;
}

void pitchPEFObj_enableDebug(PitchPEFObj o, int isDebug) {
    if (!o) return;
    o->head.isDebug = isDebug;
    if (isDebug)
        printf("pitchPEF params is: samplate=%d, fftLength=%d, slideLength=%d, lowFre=%g, highFre=%g, cutFre=%g, minIndex=%d, "
               "maxIndex=%d, alpha=%g, beta=%g, gamma=%g, filterPadNum=%d, windowType=%d\n",
               o->head.samplate, o->head.fftLength, o->head.slideLength, o->lowFre, o->highFre, o->cutFre, o->minIndex, o->maxIndex, o->alpha,
               o->beta, o->gamma, o->filterPadNum, (int)o->windowType);
}

void pitchPEFObj_free(PitchPEFObj o) { pef_free(o); }
int pitchPEFObj_minIndex(PitchPEFObj o) { return o ? o->minIndex : 0; }
int pitchPEFObj_maxIndex(PitchPEFObj o) { return o ? o->maxIndex : 0; }
int pitchPEFObj_filterPadNum(PitchPEFObj o) { return o ? o->filterPadNum : 0; }
int pitchPEFObj_logLength(PitchPEFObj o) { return o ? 2 * o->head.fftLength : 0; }
