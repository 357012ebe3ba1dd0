/* afx_harmonic_ratio.c -- the harmonic ratio object (C host side) behind include/mir/harmonicRatio_algorithm.h.
 *
 * Mirrors the parameter semantics of the reference object (src/mir/harmonicRatio_algorithm.c:52-170): defaults, fallbacks,
 * the exponent that counts the TRANSFORM when it is defaulted and the window when it is given, the window type nobody reads,
 * maxLength in float32.  Execution: afxk_harmonic_ratio (afx_harmonic_ratio.hip), three stream-ordered launches from the
 * samples to the value per frame.  The host-pointer call is the batch of one through the staging buffers of afx_pitchkit.h;
 * there is no isContinue, so the head's tail never keeps a sample.  Device memory: the window and the twiddles, uploaded
 * once, the staged samples / values of the host-pointer call and two ints per frame of scratch.  There is no CPU compute
 * path.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/harmonicRatio_algorithm.h"

void afx_harmonic_ratio_plan_free(AfxHarmonicRatioPlan *p) {
    if (!p) return;
    free(p->window);
    p->window = NULL;
}

/* defaults, fallbacks, the window and the refusal of the constructor: needs no device */
int afx_harmonic_ratio_plan_host(int *samplate, float *lowFre, int *radix2Exp, WindowType *windowType, int *slideLength,
                                 AfxHarmonicRatioPlan *p) {
    (void)windowType; /* harmonicRatio_algorithm.c:60,119: the argument is never read */
    if (!p) return AFX_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->samplate = 32000;
    p->lowFre = 25.f;
    p->radix2Exp = 11; /* :59,103-104: the default 12 is the transform's exponent */
    if (samplate && *samplate > 0 && *samplate <= 196000) p->samplate = *samplate;
    if (lowFre && *lowFre > 0 && *lowFre < p->samplate / 2) p->lowFre = *lowFre;
    if (radix2Exp) {
        if (*radix2Exp < AFX_PITCH_LAG_MIN_EXP || *radix2Exp > AFX_PITCH_LAG_MAX_EXP) return -100;
        p->radix2Exp = *radix2Exp;
    }
    const int N = p->windowLength = 1 << p->radix2Exp;
    p->fftLength = 2 * N;
    p->slideLength = (slideLength && *slideLength > 0) ? *slideLength : N / 4;
    p->maxLength = (int)floorf(p->samplate / p->lowFre);
    if (p->maxLength > N - 1) p->maxLength = N - 1;
    p->ldsBytes = afx_pitch_lag_lds_bytes(p->radix2Exp);
    p->window = afx_window_fft(Window_Hamm, N);
    return p->window ? 0 : AFX_ERR_NOMEM;
}

int harmonicRatioObj_new(HarmonicRatioObj *harmonicRatioObj, int *samplate, float *lowFre, int *radix2Exp, WindowType *windowType,
                         int *slideLength) {
    if (!harmonicRatioObj) return -1;
    *harmonicRatioObj = NULL;
    AfxHarmonicRatioPlan p;
    int st = afx_harmonic_ratio_plan_host(samplate, lowFre, radix2Exp, windowType, slideLength, &p);
    if (st == 0) st = afxdev_ensure();
    if (st != AFX_OK) {
        afx_harmonic_ratio_plan_free(&p);
        return st;
    }
    struct OpaqueHarmonicRatio *o = (struct OpaqueHarmonicRatio *)calloc(1, sizeof(*o));
    if (!o) {
        afx_harmonic_ratio_plan_free(&p);
        return AFX_ERR_NOMEM;
    }
    o->maxLength = p.maxLength;
    o->lowFre = p.lowFre;
    st = afx_pitch_head_init(&o->head, p.radix2Exp, p.slideLength, p.samplate, 0);
    const size_t N = (size_t)p.windowLength;
    float *tw = NULL;
    if (st == AFX_OK) {
        tw = afx_twiddle_table(p.fftLength);
        if (!tw) st = AFX_ERR_NOMEM;
    }
    st = afx_pitch_table(st, &o->dWindow, p.window, sizeof(float) * N, o->head.stream);
    st = afx_pitch_table(st, &o->dTwiddle, tw, sizeof(float) * 2 * N, o->head.stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->head.stream);
    free(tw);
    afx_harmonic_ratio_plan_free(&p);
    if (st != AFX_OK) {
        harmonicRatioObj_free(o);
        return st;
    }
    *harmonicRatioObj = o;
    return 0;
}

void harmonicRatioObj_free(HarmonicRatioObj o) {
    if (!o) return;
    afx_pitch_head_sync(&o->head);
    afx_scratch_drain(&o->scratchStream);
    afxdev_free(o->dWindow);
    afxdev_free(o->dTwiddle);
    afxdev_free(o->dScratch);
    afx_pitch_head_release(&o->head);
    free(o);
}

int harmonicRatioObj_calTimeLength(HarmonicRatioObj o, int dataLength) { return afx_pitch_frames(AFX_PITCH_HEAD(o), dataLength); }
int harmonicRatioObj_maxLength(HarmonicRatioObj o) { return o ? o->maxLength : 0; }
int harmonicRatioObj_windowLength(HarmonicRatioObj o) { return o ? o->head.fftLength : 0; }

/* the three launches over `batch` clips; the scratch is reserved here */
static int hr_launch(struct OpaqueHarmonicRatio *o, const float *dData, int batch, int dataLength, long long clipStride, int T,
                     float *dValue, int *dLag, int *dFirst, long long outStride, float *dCurve, void *stream) {
    AfxHarmonicRatioArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dData;
    a.clipStride = clipStride;
    a.batch = batch;
    a.dataLength = dataLength;
    a.timeLength = T;
    a.radix2Exp = o->head.radix2Exp;
    a.hop = o->head.slideLength;
    a.maxLength = o->maxLength;
    a.window = o->dWindow;
    a.twiddle = o->dTwiddle;
    a.value = dValue;
    a.lag = dLag;
    a.first = dFirst;
    a.outStride = outStride;
    a.curve = dCurve;
    int st = afx_scratch_enter(&o->scratchStream, stream);
    if (st == AFX_OK)
        st = afxdev_reserve((void **)&o->dScratch, &o->capScratch,
                            sizeof(int) * (size_t)afx_harmonic_ratio_scratch_ints((long long)batch * T));
    if (st != AFX_OK) return st;
    a.scratch = o->dScratch;
    return afxk_harmonic_ratio(&a, stream);
}

/* AfxPitchRun of the host-pointer call: the row of results is the values */
static int hr_run(void *ctx, const float *dData, int batch, int dataLength, long long clipStride, int T, float *dValue, float *unused,
                  long long outStride, float *dCurve, void *stream) {
    (void)unused;
    return hr_launch((struct OpaqueHarmonicRatio *)ctx, dData, batch, dataLength, clipStride, T, dValue, NULL, NULL, outStride, dCurve,
                     stream);
}

void harmonicRatioObj_harmonicRatio(HarmonicRatioObj o, float *dataArr, int dataLength, float *valueArr) {
    afx_pitch_call(AFX_PITCH_HEAD(o), dataArr, dataLength, valueArr, hr_run, o, "harmonicRatioObj_harmonicRatio");
}

int harmonicRatioObj_harmonicRatioBatchDevice(HarmonicRatioObj o, const float *dData, int batch, int dataLength, long long clipStride,
                                              float *dValue, int *dLag, int *dFirst, long long outStride, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "harmonicRatioObj", dData, batch, dataLength, clipStride, dValue, hipStream, &T);
    if (go <= 0) return go;
    if (outStride < T) return AFX_ERR_ARG;
    return hr_launch(o, dData, batch, dataLength, clipStride, T, dValue, dLag, dFirst, outStride, NULL, hipStream);
}

int harmonicRatioObj_curveBatchDevice(HarmonicRatioObj o, const float *dData, int batch, int dataLength, long long clipStride,
                                      float *dCurve, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "harmonicRatioObj", dData, batch, dataLength, clipStride, dCurve, hipStream, &T);
    if (go <= 0) return go;
    return hr_launch(o, dData, batch, dataLength, clipStride, T, NULL, NULL, NULL, 0, dCurve, hipStream);
}
