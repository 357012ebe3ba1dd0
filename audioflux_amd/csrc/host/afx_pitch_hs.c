/* afx_pitch_hs.c -- the harmonic-product-spectrum and log-harmonic-sum pitch tracker objects (C host side) behind
 * include/mir/_pitch_hps.h and include/mir/_pitch_lhs.h: one implementation, two thin sets of exported names; `kind`
 * selects the combining operator and the few places where the reference's two constructors differ.
 *
 * Mirrors the parameter semantics of the reference objects (src/mir/_pitch_hps.c:81-269, src/mir/_pitch_lhs.c:81-266).
 * Execution: ONE kernel launch per call (k_pitch_hs, afx_pitch_hs.hip) from the samples to the frequency per frame.  The
 * host-pointer call is the batch of one through staging buffers and carries the isContinue tail (afx_frametail.h).  There
 * is no CPU compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "afx_frametail.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/_pitch_hps.h"
#include "mir/_pitch_lhs.h"

#define HS_MIN_EXP 6
#define HS_MAX_EXP 13

/* util_roundPowerTwo (flux_util.c:74-100): the nearer power of two, ties up; 1 below 1 */
static int round_pow2(int value) {
    if (value < 1) return 1;
    int lo = 1;
    while (lo <= value / 2) lo *= 2;
    if (lo == value) return value;
    const long long hi = 2LL * lo;
    return value - lo < hi - value ? lo : (int)hi;
}

/* defaults, clamps and refusals of the two constructors that need no device */
static int hs_plan(int kind, const int *samplate, const float *lowFre, const float *highFre, const int *radix2Exp,
                   const int *slideLength, const WindowType *windowType, const int *harmonicCount, const int *isContinue,
                   AfxPitchHsPlan *p) {
    memset(p, 0, sizeof(*p));
    p->samplate = 32000;
    p->lowFre = 32.f;
    p->highFre = 2000.f;
    p->radix2Exp = 12;
    p->harmonicCount = 5;
    p->windowType = (int)Window_Hamm;
    if (samplate && *samplate > 0 && *samplate <= 196000) p->samplate = *samplate;
    if (lowFre && *lowFre >= 27) p->lowFre = *lowFre;
    if (highFre) {
        /* (samplate / 2 is an integer division there, too) */
        if (*highFre > p->lowFre && *highFre < p->samplate / 2) {
            p->highFre = *highFre;
        } else {
            p->lowFre = 32.f;
            p->highFre = 2000.f;
        }
    }
    if (radix2Exp) {
        if (*radix2Exp < HS_MIN_EXP || *radix2Exp > HS_MAX_EXP) return -100;
        p->radix2Exp = *radix2Exp;
    }
    if (harmonicCount && *harmonicCount > 0) p->harmonicCount = *harmonicCount;
    if (windowType) {
        /* _pitch_hps.c:142-146 keeps Hamm for a type above it; _pitch_lhs.c:142-144 takes whatever it is given */
        if (kind == AFX_PITCH_LHS || (int)*windowType <= (int)Window_Hamm) p->windowType = (int)*windowType;
    }
    p->fftLength = 1 << p->radix2Exp;
    p->slideLength = (slideLength && *slideLength > 0) ? *slideLength : p->fftLength / 4;
    p->isContinue = isContinue ? *isContinue : 0;
    p->interpLength = round_pow2(p->samplate);
    p->minIndex = (int)ceilf(p->lowFre);
    p->maxIndex = (int)floorf(p->highFre);
    if (kind == AFX_PITCH_LHS) {
        /* _pitch_lhs.c:244-257.  _pitch_hps.c:246-252 computes the same clamp and drops it: HPS runs the count as given */
        const int k = p->samplate / (p->maxIndex + 1);
        if (p->harmonicCount > k) p->harmonicCount = k ? k : 1;
    }
    const long long last = (long long)p->maxIndex * p->harmonicCount;
    p->lastBin = last > 0x7fffffffLL ? 0x7fffffff : (int)last;
    if (p->fftLength > p->interpLength) {
        afxdev_set_error("pitch%sObj_new: fftLength %d above the interpolated length %d of samplate %d",
                         kind == AFX_PITCH_LHS ? "LHS" : "HPS", p->fftLength, p->interpLength, p->samplate);
        return AFX_ERR_ARG;
    }
    if (last >= p->interpLength) {
        afxdev_set_error("pitch%sObj_new: bin maxIndex %d * harmonicCount %d lies beyond the %d-point spectrum",
                         kind == AFX_PITCH_LHS ? "LHS" : "HPS", p->maxIndex, p->harmonicCount, p->interpLength);
        return AFX_ERR_ARG;
    }
    const int D = p->interpLength / p->fftLength;
    p->transforms = D / 2 + 1;
    p->sliceFloats = afx_pitch_hs_slice_floats(p->lastBin);
    const long long fixed = afx_pitch_hs_lds_fixed(p->radix2Exp);
    p->sliceInLds = fixed + 4 * p->sliceFloats <= AFX_PITCH_HS_LDS_BUDGET;
    p->ldsBytes = fixed + (p->sliceInLds ? 4 * p->sliceFloats : 0);
    return 0;
}

int afx_pitch_hs_plan_host(int kind, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,
                           WindowType *windowType, int *harmonicCount, int *isContinue, AfxPitchHsPlan *plan) {
    if (!plan || (kind != AFX_PITCH_HPS && kind != AFX_PITCH_LHS)) return AFX_ERR_ARG;
    return hs_plan(kind, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, harmonicCount, isContinue, plan);
}

static void hs_free(struct OpaquePitchHS *o) {
    if (!o) return;
    afx_pitch_head_sync(&o->head);
    afx_scratch_drain(&o->scratchStream);
    afxdev_free(o->dWindow);
    afxdev_free(o->dTwiddle);
    afxdev_free(o->dRoots);
    afxdev_free(o->dSlice);
    afx_pitch_head_release(&o->head);
    free(o);
}

static int hs_new(int kind, struct OpaquePitchHS **out, const int *samplate, const float *lowFre, const float *highFre,
                  const int *radix2Exp, const int *slideLength, const WindowType *windowType, const int *harmonicCount,
                  const int *isContinue) {
    if (!out) return -1;
    *out = NULL;
    AfxPitchHsPlan p;
    int st = hs_plan(kind, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, harmonicCount, isContinue, &p);
    if (st != 0) return st;
    st = afxdev_ensure();
    if (st != AFX_OK) return st;
    struct OpaquePitchHS *o = (struct OpaquePitchHS *)calloc(1, sizeof(*o));
    if (!o) return AFX_ERR_NOMEM;
    o->kind = kind;
    o->interpLength = p.interpLength;
    o->interpExp = afx_log2_exact(p.interpLength);
    o->minIndex = p.minIndex;
    o->maxIndex = p.maxIndex;
    o->harmonicCount = p.harmonicCount;
    o->lastBin = p.lastBin;
    o->sliceInLds = p.sliceInLds;
    o->transforms = p.transforms;
    o->windowType = (WindowType)p.windowType;
    st = afx_pitch_head_init(&o->head, p.radix2Exp, p.slideLength, p.samplate, p.isContinue);
    const size_t M = (size_t)p.interpLength, N = (size_t)p.fftLength;
    float *win = NULL, *tw = NULL, *roots = NULL;
    if (st == AFX_OK) {
        win = afx_window_fft(o->windowType, p.fftLength);
        tw = afx_twiddle_table(p.fftLength);
        roots = (float *)malloc(sizeof(float) * 2 * M);
        if (!win || !tw || !roots) st = AFX_ERR_NOMEM;
    }
    if (st == AFX_OK) {
        /* the M-th roots of unity, each evaluated in double: the modulator of residue q reads entry (n q) mod M */
        for (size_t m = 0; m < M; ++m) {
            const double ph = 2.0 * M_PI * (double)m / (double)M;
            roots[2 * m] = (float)cos(ph);
            roots[2 * m + 1] = (float)-sin(ph);
        }
    }
    st = afx_pitch_table(st, &o->dWindow, win, sizeof(float) * N, o->head.stream);
    st = afx_pitch_table(st, &o->dTwiddle, tw, sizeof(float) * N, o->head.stream);
    st = afx_pitch_table(st, &o->dRoots, roots, sizeof(float) * 2 * M, o->head.stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->head.stream);
    free(win);
    free(tw);
    free(roots);
    if (st != AFX_OK) {
        hs_free(o);
        return st;
    }
    *out = o;
    return 0;
}

/* one launch over `batch` clips: the slice scratch of the plans that need it is reserved here */
static int hs_run(void *ctx, const float *dData, int batch, int dataLength, long long clipStride, int T, float *dFre, float *dValue,
                  long long outStride, float *dCurve, void *stream) {
    struct OpaquePitchHS *o = (struct OpaquePitchHS *)ctx;
    AfxPitchHsArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dData;
    a.clipStride = clipStride;
    a.batch = batch;
    a.dataLength = dataLength;
    a.timeLength = T;
    a.kind = o->kind;
    a.radix2Exp = o->head.radix2Exp;
    a.hop = o->head.slideLength;
    a.interpExp = o->interpExp;
    a.minIndex = o->minIndex;
    a.maxIndex = o->maxIndex;
    a.harmonicCount = o->harmonicCount;
    a.freStep = 1.0 * o->head.samplate / o->interpLength;
    a.window = o->dWindow;
    a.twiddle = o->dTwiddle;
    a.roots = o->dRoots;
    a.fre = dFre;
    a.value = dValue;
    a.outStride = outStride;
    a.curve = dCurve;
    if (!o->sliceInLds) {
        const long long rows = (long long)batch * T;
        a.groups = rows < AFX_PITCH_HS_SCRATCH_GROUPS ? (int)rows : AFX_PITCH_HS_SCRATCH_GROUPS;
        int st = afx_scratch_enter(&o->scratchStream, stream);
        if (st == AFX_OK)
            st = afxdev_reserve((void **)&o->dSlice, &o->capSlice,
                                sizeof(float) * (size_t)a.groups * (size_t)afx_pitch_hs_slice_floats(o->lastBin));
        if (st != AFX_OK) return st;
        a.slice = o->dSlice;
    }
    return afxk_pitch_hs(&a, stream);
}

static int hs_pitch_batch(struct OpaquePitchHS *o, const char *name, const float *dData, int batch, int dataLength, long long clipStride,
                          float *dFre, float *dValue, long long outStride, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), name, dData, batch, dataLength, clipStride, dFre, hipStream, &T);
    if (go <= 0) return go;
    if (outStride < T) return AFX_ERR_ARG;
    return hs_run(o, dData, batch, dataLength, clipStride, T, dFre, dValue, outStride, NULL, hipStream);
}

static int hs_curve_batch(struct OpaquePitchHS *o, const char *name, const float *dData, int batch, int dataLength, long long clipStride,
                          float *dCurve, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), name, dData, batch, dataLength, clipStride, dCurve, hipStream, &T);
    if (go <= 0) return go;
    return hs_run(o, dData, batch, dataLength, clipStride, T, NULL, NULL, 0, dCurve, hipStream);
}

static void hs_debug(struct OpaquePitchHS *o, int isDebug) {
    if (!o) return;
    o->head.isDebug = isDebug;
    if (isDebug)
        printf("pitch%s params is: samplate=%d, fftLength=%d, slideLength=%d, interpFFTLength=%d, minIndex=%d, maxIndex=%d, "
               "harmonicCount=%d, windowType=%d\n",
               o->kind == AFX_PITCH_LHS ? "LHS" : "HPS", o->head.samplate, o->head.fftLength, o->head.slideLength, o->interpLength,
               o->minIndex, o->maxIndex, o->harmonicCount, (int)o->windowType);
}

/* ---- the exported names ------------------------------------------------------------------------------------------------ */
#define HS_EXPORTS(NAME, TYPE, KIND)                                                                                              \
    int pitch##NAME##Obj_new(TYPE *obj, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,           \
                             WindowType *windowType, int *harmonicCount, int *isContinue) {                                       \
        return hs_new(KIND, obj, samplate, lowFre, highFre, radix2Exp, slideLength, windowType, harmonicCount, isContinue);       \
    }                                                                                                                             \
    int pitch##NAME##Obj_calTimeLength(TYPE o, int dataLength) { return afx_pitch_frames(AFX_PITCH_HEAD(o), dataLength); }        \
    void pitch##NAME##Obj_pitch(TYPE o, float *dataArr, int dataLength, float *freArr) {                                          \
        afx_pitch_call(AFX_PITCH_HEAD(o), dataArr, dataLength, freArr, hs_run, o, "pitch" #NAME "Obj_pitch");                     \
    }                                                                                                                             \
    void pitch##NAME##Obj_enableDebug(TYPE o, int isDebug) { hs_debug(o, isDebug); }                                              \
    void pitch##NAME##Obj_free(TYPE o) { hs_free(o); }                                                                            \
    int pitch##NAME##Obj_pitchBatchDevice(TYPE o, const float *dData, int batch, int dataLength, long long clipStride,            \
                                          float *dFre, float *dValue, long long outStride, void *hipStream) {                     \
        return hs_pitch_batch(o, "pitch" #NAME "Obj", dData, batch, dataLength, clipStride, dFre, dValue, outStride, hipStream);  \
    }                                                                                                                             \
    int pitch##NAME##Obj_curveBatchDevice(TYPE o, const float *dData, int batch, int dataLength, long long clipStride,            \
                                          float *dCurve, void *hipStream) {                                                       \
        return hs_curve_batch(o, "pitch" #NAME "Obj", dData, batch, dataLength, clipStride, dCurve, hipStream);                   \
    }                                                                                                                             \
    int pitch##NAME##Obj_minIndex(TYPE o) { return o ? o->minIndex : 0; }                                                         \
    int pitch##NAME##Obj_maxIndex(TYPE o) { return o ? o->maxIndex : 0; }                                                         \
    int pitch##NAME##Obj_harmonicCount(TYPE o) { return o ? o->harmonicCount : 0; }                                               \
    int pitch##NAME##Obj_interpLength(TYPE o) { return o ? o->interpLength : 0; }

HS_EXPORTS(HPS, PitchHPSObj, AFX_PITCH_HPS)
HS_EXPORTS(LHS, PitchLHSObj, AFX_PITCH_LHS)
