/* afx_pitch_lag.c -- the lag-domain pitch tracker objects (C host side) behind include/mir/_pitch_ncf.h and
 * include/mir/_pitch_cep.h: the normalised autocorrelation and the cepstrum, one layout and one kernel, `mode` apart.
 *
 * Mirrors the parameter semantics of the reference objects (src/mir/_pitch_ncf.c:77-235, src/mir/_pitch_cep.c:77-237):
 * defaults, fallbacks, the candidate range in float32, the window from afx_window.c.  Execution: ONE kernel launch per call
 * (k_pitch_lag, afx_pitch_lag.hip) from the samples to the frequency per frame.  The host-pointer call is the batch of one
 * through staging buffers and carries the isContinue tail (afx_pitchkit.h).  Device memory: the window and the twiddles,
 * uploaded once, and the staged samples / frequencies of the host-pointer call.  There is no CPU compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/_pitch_cep.h"
#include "mir/_pitch_ncf.h"

static const char *const lag_name[2] = {"pitchNCFObj", "pitchCEPObj"};

static void lag_plan_free(AfxPitchLagPlan *p) {
    if (!p) return;
    free(p->window);
    p->window = NULL;
}

/* defaults, fallbacks, the window and refusals of the two constructors: needs no device */
static int lag_plan(int mode, const int *samplate, const float *lowFre, const float *highFre, const int *radix2Exp,
                    const int *slideLength, const WindowType *windowType, const int *isContinue, AfxPitchLagPlan *p) {
    if (!p) return AFX_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->samplate = 32000;
    p->lowFre = 32.f;
    p->highFre = 2000.f;
    p->radix2Exp = 12;
    p->windowType = (int)(mode == AFX_PITCH_LAG_NCF ? Window_Rect : Window_Hamm);
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
    if (radix2Exp) {
        if (*radix2Exp < AFX_PITCH_LAG_MIN_EXP || *radix2Exp > AFX_PITCH_LAG_MAX_EXP) return -100;
        p->radix2Exp = *radix2Exp;
    }
    /* NCF takes any type; CEP only Rect, Hann, Hamm (_pitch_cep.c:127-131) */
    if (windowType && (mode == AFX_PITCH_LAG_NCF || *windowType <= Window_Hamm)) p->windowType = (int)*windowType;
    const int N = p->fftLength = 1 << p->radix2Exp;
    p->slideLength = (slideLength && *slideLength > 0) ? *slideLength : N / 4;
    p->isContinue = isContinue ? *isContinue : 0;
    p->lagLength = 2 * N;
    p->ldsBytes = afx_pitch_lag_lds_bytes(p->radix2Exp);
    p->minIndex = (int)roundf(p->samplate / p->highFre);
    p->maxIndex = (int)roundf(p->samplate / p->lowFre);
    p->window = afx_window_fft((WindowType)p->windowType, N);
    if (!p->window) return AFX_ERR_NOMEM;

    /* where the reference overruns its own buffers (the headers' deviations) */
    const int last = mode == AFX_PITCH_LAG_NCF ? N - 1 : 2 * N - 1;
    if (p->maxIndex > last) {
        afxdev_set_error("%s_new: samplate %d / lowFre %g give maxIndex %d beyond the last %s %d of fftLength %d", lag_name[mode],
                         p->samplate, p->lowFre, p->maxIndex, mode == AFX_PITCH_LAG_NCF ? "lag" : "quefrency", last, N);
        return AFX_ERR_ARG;
    }
    if (mode == AFX_PITCH_LAG_NCF && p->minIndex < 1) {
        afxdev_set_error("%s_new: samplate %d / highFre %g give minIndex %d", lag_name[mode], p->samplate, p->highFre, p->minIndex);
        return AFX_ERR_ARG;
    }
    return 0;
}

static void lag_free(struct OpaquePitchLag *o) {
    if (!o) return;
    afx_pitch_head_sync(&o->head);
    afxdev_free(o->dWindow);
    afxdev_free(o->dTwiddle);
    afx_pitch_head_release(&o->head);
    free(o);
}

static int lag_new(int mode, void **handle, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,
                   WindowType *windowType, int *isContinue) {
    *handle = NULL;
    AfxPitchLagPlan p;
    int st = lag_plan(mode, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, isContinue, &p);
    if (st == 0) st = afxdev_ensure();
    if (st != AFX_OK) {
        lag_plan_free(&p);
        return st;
    }
    struct OpaquePitchLag *o = (struct OpaquePitchLag *)calloc(1, sizeof(*o));
    if (!o) {
        lag_plan_free(&p);
        return AFX_ERR_NOMEM;
    }
    o->mode = mode;
    o->minIndex = p.minIndex;
    o->maxIndex = p.maxIndex;
    o->lowFre = p.lowFre;
    o->highFre = p.highFre;
    o->windowType = (WindowType)p.windowType;
    st = afx_pitch_head_init(&o->head, p.radix2Exp, p.slideLength, p.samplate, p.isContinue);
    const size_t N = (size_t)p.fftLength;
    float *tw = NULL;
    if (st == AFX_OK) {
        tw = afx_twiddle_table(2 * p.fftLength);
        if (!tw) st = AFX_ERR_NOMEM;
    }
    /* the rectangular window is no multiply in the reference (_pitch_ncf.c:445, _pitch_cep.c:436): no table */
    if (o->windowType != Window_Rect) st = afx_pitch_table(st, &o->dWindow, p.window, sizeof(float) * N, o->head.stream);
    st = afx_pitch_table(st, &o->dTwiddle, tw, sizeof(float) * 2 * N, o->head.stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->head.stream);
    free(tw);
    lag_plan_free(&p);
    if (st != AFX_OK) {
        lag_free(o);
        return st;
    }
    *handle = o;
    return 0;
}

/* one launch over `batch` clips */
static int lag_run(void *ctx, const float *dData, int batch, int dataLength, long long clipStride, int T, float *dFre, float *dValue,
                   long long outStride, float *dCurve, void *stream) {
    const struct OpaquePitchLag *o = (const struct OpaquePitchLag *)ctx;
    AfxPitchLagArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dData;
    a.clipStride = clipStride;
    a.batch = batch;
    a.dataLength = dataLength;
    a.timeLength = T;
    a.radix2Exp = o->head.radix2Exp;
    a.hop = o->head.slideLength;
    a.mode = o->mode;
    a.samplate = o->head.samplate;
    a.minIndex = o->minIndex;
    a.maxIndex = o->maxIndex;
    a.window = o->dWindow;
    a.twiddle = o->dTwiddle;
    a.fre = dFre;
    a.value = dValue;
    a.outStride = outStride;
    a.curve = dCurve;
    return afxk_pitch_lag(&a, stream);
}

static int lag_pitch_batch(struct OpaquePitchLag *o, int mode, const float *dData, int batch, int dataLength, long long clipStride,
                           float *dFre, float *dValue, long long outStride, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), lag_name[mode], dData, batch, dataLength, clipStride, dFre, hipStream, &T);
    if (go <= 0) return go;
    if (outStride < T) return AFX_ERR_ARG;
    return lag_run(o, dData, batch, dataLength, clipStride, T, dFre, dValue, outStride, NULL, hipStream);
}

static int lag_curve_batch(struct OpaquePitchLag *o, int mode, const float *dData, int batch, int dataLength, long long clipStride,
                           float *dCurve, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), lag_name[mode], dData, batch, dataLength, clipStride, dCurve, hipStream, &T);
    if (go <= 0) return go;
    return lag_run(o, dData, batch, dataLength, clipStride, T, NULL, NULL, 0, dCurve, hipStream);
}

static void lag_debug(struct OpaquePitchLag *o, int isDebug) {
    if (!o) return;
    o->head.isDebug = isDebug;
    if (isDebug)
        printf("%s params is: samplate=%d, fftLength=%d, slideLength=%d, lowFre=%g, highFre=%g, minIndex=%d, maxIndex=%d, "
               "windowType=%d\n", lag_name[o->mode], o->head.samplate, o->head.fftLength, o->head.slideLength, o->lowFre, o->highFre,
               o->minIndex, o->maxIndex, (int)o->windowType);
}

/* a handle is its OpaquePitchLag: the first member of both wrappers */
#define LAG(o) ((struct OpaquePitchLag *)(o))

/* ---- normalised autocorrelation ------------------------------------------------------------------------------------------ */
int afx_pitch_ncf_plan_host(int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength, WindowType *windowType,
                            int *isContinue, AfxPitchLagPlan *plan) {
    return lag_plan(AFX_PITCH_LAG_NCF, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, isContinue, plan);
}
void afx_pitch_ncf_plan_free(AfxPitchLagPlan *plan) { lag_plan_free(plan); }

int pitchNCFObj_new(PitchNCFObj *pitchNCFObj, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,
                    WindowType *windowType, int *isContinue) {
    if (!pitchNCFObj) return -1;
    void *h = NULL;
    const int st = lag_new(AFX_PITCH_LAG_NCF, &h, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, isContinue);
    *pitchNCFObj = (PitchNCFObj)h;
    return st;
}
int pitchNCFObj_calTimeLength(PitchNCFObj o, int dataLength) { return afx_pitch_frames(AFX_PITCH_HEAD(LAG(o)), dataLength); }
void pitchNCFObj_pitch(PitchNCFObj o, float *dataArr, int dataLength, float *freArr) {
    afx_pitch_call(AFX_PITCH_HEAD(LAG(o)), dataArr, dataLength, freArr, lag_run, o, "pitchNCFObj_pitch");
}
int pitchNCFObj_pitchBatchDevice(PitchNCFObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dFre,
                                 float *dValue, long long outStride, void *hipStream) {
    return lag_pitch_batch(LAG(o), AFX_PITCH_LAG_NCF, dData, batch, dataLength, clipStride, dFre, dValue, outStride, hipStream);
}
int pitchNCFObj_curveBatchDevice(PitchNCFObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dCurve,
                                 void *hipStream) {
    return lag_curve_batch(LAG(o), AFX_PITCH_LAG_NCF, dData, batch, dataLength, clipStride, dCurve, hipStream);
}
void pitchNCFObj_enableDebug(PitchNCFObj o, int isDebug) { lag_debug(LAG(o), isDebug); }
void pitchNCFObj_free(PitchNCFObj o) { lag_free(LAG(o)); }
int pitchNCFObj_minIndex(PitchNCFObj o) { return o ? LAG(o)->minIndex : 0; }
int pitchNCFObj_maxIndex(PitchNCFObj o) { return o ? LAG(o)->maxIndex : 0; }

/* ---- cepstrum ------------------------------------------------------------------------------------------------------------ */
int afx_pitch_cep_plan_host(int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength, WindowType *windowType,
                            int *isContinue, AfxPitchLagPlan *plan) {
    return lag_plan(AFX_PITCH_LAG_CEP, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, isContinue, plan);
}
void afx_pitch_cep_plan_free(AfxPitchLagPlan *plan) { lag_plan_free(plan); }

int pitchCEPObj_new(PitchCEPObj *pitchCEPObj, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,
                    WindowType *windowType, int *isContinue) {
    if (!pitchCEPObj) return -1;
    void *h = NULL;
    const int st = lag_new(AFX_PITCH_LAG_CEP, &h, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, isContinue);
    *pitchCEPObj = (PitchCEPObj)h;
    return st;
}
int pitchCEPObj_calTimeLength(PitchCEPObj o, int dataLength) { return afx_pitch_frames(AFX_PITCH_HEAD(LAG(o)), dataLength); }
void pitchCEPObj_pitch(PitchCEPObj o, float *dataArr, int dataLength, float *freArr) {
    afx_pitch_call(AFX_PITCH_HEAD(LAG(o)), dataArr, dataLength, freArr, lag_run, o, "pitchCEPObj_pitch");
}
int pitchCEPObj_pitchBatchDevice(PitchCEPObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dFre,
                                 float *dValue, long long outStride, void *hipStream) {
    return lag_pitch_batch(LAG(o), AFX_PITCH_LAG_CEP, dData, batch, dataLength, clipStride, dFre, dValue, outStride, hipStream);
}
int pitchCEPObj_curveBatchDevice(PitchCEPObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dCurve,
                                 void *hipStream) {
    return lag_curve_batch(LAG(o), AFX_PITCH_LAG_CEP, dData, batch, dataLength, clipStride, dCurve, hipStream);
}
void pitchCEPObj_enableDebug(PitchCEPObj o, int isDebug) { lag_debug(LAG(o), isDebug); }
void pitchCEPObj_free(PitchCEPObj o) { lag_free(LAG(o)); }
int pitchCEPObj_minIndex(PitchCEPObj o) { return o ? LAG(o)->minIndex : 0; }
int pitchCEPObj_maxIndex(PitchCEPObj o) { return o ? LAG(o)->maxIndex : 0; }
