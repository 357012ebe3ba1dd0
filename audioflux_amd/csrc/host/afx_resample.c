/* afx_resample.c -- the resampler object (C host side) behind include/dsp/resample_algorithm.h.
 *
 * Mirrors the parameter semantics of the reference object (src/dsp/resample_algorithm.c:59-341, 523-634): defaults and
 * fallbacks, the windowed-sinc table in the reference's float32 operation order (windows from afx_window.c), the ratio
 * state machine that divides and multiplies the table in place, the two length rules.  Execution: ONE kernel launch per
 * call (k_resample, afx_resample.hip).  The host-pointer call is the batch of one through grow-only staging buffers on the
 * object's stream.  Device memory: the table, uploaded by the constructor and by every setter that rescales it, and the
 * staged samples / outputs of the host-pointer call.  There is no CPU compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "dsp/resample_algorithm.h"

/* ---- the plan: everything that needs no device ---------------------------------------------------------------------------- */

/* what a launch over 4 or more clips would look like at the plan's ratio */
static void plan_launch(AfxResamplePlan *p) {
    AfxResampleLaunch l;
    memset(&l, 0, sizeof(l));
    p->step = p->ratio > 0 ? afx_resample_step(p->ratio, p->bitLength) : 0;
    const int ok = afx_resample_launch_plan(AFX_RESAMPLE_GROUP, p->ratio, p->bitLength, p->interpLength, &l) == AFX_OK;
    p->taps = ok ? l.taps : 0;
    p->tableInLds = ok ? l.tableInLds : 0;
    p->group = ok ? l.group : 0;
    p->ldsBytes = ok ? l.ldsBytes : 0;
}

/* the symmetric window of `length` points (_resampleObj_calInterpArr, :582-626) */
static float *plan_window(WindowType type, float value, int length) {
    if (type == Window_Kaiser) return afx_window_kaiser(length, value);
    if (type == Window_Gauss) return afx_window_gauss(length, value);
    if (type == Window_Tukey) return afx_window_tukey(length, value);
    return afx_window_create(type, length, 0);
}

/* table[k] *= ratio / table[k] /= ratio, entry by entry; the entry behind the last one repeats it */
static void table_mul(AfxResamplePlan *p, float r) {
    for (int i = 0; i < p->interpLength; i++) p->table[i] *= r;
}
static void table_div(AfxResamplePlan *p, float r) {
    for (int i = 0; i < p->interpLength; i++) p->table[i] /= r;
}

/* :281-295, :314-328: 1 when the table changed */
static int plan_ratio(AfxResamplePlan *p, float ratio) {
    int changed = 0;
    if (ratio != p->ratio && (p->ratio < 1 || ratio < 1)) {
        if (p->ratio < 1) table_div(p, p->ratio);
        if (ratio < 1) table_mul(p, ratio);
        p->table[p->interpLength] = p->table[p->interpLength - 1];
        changed = 1;
    }
    p->ratio = ratio;
    plan_launch(p);
    return changed;
}

static int gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

/* 0 / 1 / 2: ignored, accepted, accepted and the table changed */
static int plan_rate(AfxResamplePlan *p, int sourceRate, int targetRate, float ratio) {
    if (sourceRate == 0 && targetRate == 0) { /* resampleObj_setSamplateRatio */
        if (ratio < 0) return 0;
        const int changed = plan_ratio(p, ratio);
        p->p = p->q = 0;
        return 1 + changed;
    }
    if (sourceRate == targetRate || sourceRate <= 0 || targetRate <= 0) return 0;
    const int g = gcd(sourceRate, targetRate);
    const int changed = plan_ratio(p, targetRate / (float)sourceRate);
    p->sourceRate = sourceRate;
    p->targetRate = targetRate;
    p->p = targetRate / g;
    p->q = sourceRate / g;
    return 1 + changed;
}

/* :219-251: outputs of a call with dataLength samples, *source = the samples it consumes; -1: beyond an int */
static long long plan_length(const AfxResamplePlan *p, int dataLength, int *source) {
    *source = 0;
    if (dataLength <= 0) return 0;
    if (!p->isContinue) {
        const float f = floorf(dataLength * p->ratio);
        *source = dataLength;
        if (!(f < 2147483648.f)) return -1;
        return f > 0 ? (long long)f : 0;
    }
    if (p->q <= 1) return 0;
    *source = dataLength - dataLength % p->q;
    return (long long)*source * p->p / p->q;
}

static int plan_build(const ResampleQualityType *qualType, const int *zeroNum, const int *nbit, const WindowType *winType,
                      const float *value, const float *rollOff, const int *isScale, const int *isContinue, AfxResamplePlan *p) {
    if (!p) return AFX_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->zeroNum = 64;
    p->nbit = 9;
    p->winType = (int)Window_Hann;
    p->rollOff = 0.945f;
    if (qualType) { /* resampleObj_new, :59-97 */
        p->winType = (int)Window_Kaiser;
        p->value = 14.7696565f;
        p->rollOff = 0.9475937f;
        if (*qualType == ResampleQuality_Mid) {
            p->zeroNum = 32;
            p->value = 11.6625806f;
            p->rollOff = 0.8987969f;
        } else if (*qualType == ResampleQuality_Fast) {
            p->zeroNum = 16;
            p->value = 8.5555046f;
            p->rollOff = 0.85f;
        }
    } else { /* :130-175 */
        if (zeroNum && *zeroNum > 0) p->zeroNum = *zeroNum;
        if (nbit && *nbit > 0 && *nbit < 30) p->nbit = *nbit;
        if (winType && *winType > Window_Rect && *winType <= Window_Tukey) p->winType = (int)*winType; /* (beyond the enum: Hann too) */
        if (value) {
            if (*value >= 0) p->value = *value;
            if (p->value == 0) {
                if (p->winType == (int)Window_Kaiser) p->value = 5;
                else if (p->winType == (int)Window_Gauss) p->value = 2.5;
            }
        }
        if (rollOff && *rollOff > 0 && *rollOff <= 1) p->rollOff = *rollOff;
    }
    p->isScale = isScale ? *isScale : 0;
    p->isContinue = isContinue ? *isContinue : 0;
    p->bitLength = 1 << p->nbit;
    const long long entries = (long long)p->zeroNum * p->bitLength;
    if (entries > AFX_RESAMPLE_MAX_TABLE) {
        afxdev_set_error("resampleObj_new: a table of %d zero crossings x 2^%d entries is above the cap of 2^24 entries", p->zeroNum,
                         p->nbit);
        return AFX_ERR_UNSUPPORTED;
    }
    const int L = p->interpLength = (int)entries + 1;

    /* 1. the sinc: linspace(0, zeroNum, L) times rollOff, sin(pi x) / (pi x), times rollOff (:571-579, flux_vectorOp.c:378-400) */
    float *t = p->table = (float *)malloc(sizeof(float) * ((size_t)L + 1));
    float *w = plan_window((WindowType)p->winType, p->value, 2 * (L - 1) + 1);
    if (!t || !w) {
        free(w);
        free(t);
        p->table = NULL;
        return AFX_ERR_NOMEM;
    }
    const float step = ((float)p->zeroNum - 0.f) / (L - 1 > 0 ? L - 1 : 1);
    for (int i = 0; i < L; i++) {
        float v = 0.f + i * step;
        v *= p->rollOff;
        const float a = (float)(v * M_PI);
        v = fabsf(a) < 1e-9 ? 1.f : sinf(a) / a;
        v *= p->rollOff;
        /* 2. times the right half of the window (:629) */
        t[i] = v * w[L - 1 + i];
    }
    t[L] = t[L - 1];
    free(w);

    /* 3. born at 32000 -> 16000: the table times 0.5 (:194-208, :536-540) */
    p->ratio = 1.f; /* (not a state of the reference: the first plan_ratio multiplies only) */
    plan_ratio(p, 0.5f);
    p->p = 1;
    p->q = 2;
    p->sourceRate = 32000;
    p->targetRate = 16000;
    return AFX_OK;
}

int afx_resample_plan_host(ResampleQualityType *qualType, int *zeroNum, int *nbit, WindowType *winType, float *value, float *rollOff,
                           int *isScale, int *isContinue, AfxResamplePlan *plan) {
    return plan_build(qualType, zeroNum, nbit, winType, value, rollOff, isScale, isContinue, plan);
}
int afx_resample_plan_rate(AfxResamplePlan *plan, int sourceRate, int targetRate, float ratio) {
    if (!plan || !plan->table) return AFX_ERR_ARG;
    plan_rate(plan, sourceRate, targetRate, ratio);
    return AFX_OK;
}
int afx_resample_plan_length(const AfxResamplePlan *plan, int dataLength) {
    int source;
    const long long n = plan ? plan_length(plan, dataLength, &source) : 0;
    return n > 0 ? (int)n : 0;
}
void afx_resample_plan_free(AfxResamplePlan *plan) {
    if (!plan) return;
    free(plan->table);
    plan->table = NULL;
}

/* ---- the object ----------------------------------------------------------------------------------------------------------- */

static int table_upload(struct OpaqueResample *o) {
    int st = afxdev_h2d(o->dTable, o->plan.table, sizeof(float) * ((size_t)o->plan.interpLength + 1), o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream); /* the host table may change again right after */
    return st;
}

void resampleObj_free(ResampleObj o) {
    if (!o) return;
    if (o->stream) afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->batchStream);
    afxdev_free(o->dTable);
    afxdev_free(o->dX);
    afxdev_free(o->dOut);
    if (o->stream) afxdev_stream_destroy(o->stream);
    afx_resample_plan_free(&o->plan);
    free(o);
}

static int resample_new(ResampleObj *handle, ResampleQualityType *qualType, int *zeroNum, int *nbit, WindowType *winType, float *value,
                        float *rollOff, int *isScale, int *isContinue) {
    if (!handle) return AFX_ERR_ARG;
    *handle = NULL;
    AfxResamplePlan p;
    int st = plan_build(qualType, zeroNum, nbit, winType, value, rollOff, isScale, isContinue, &p);
    if (st == AFX_OK) st = afxdev_ensure();
    struct OpaqueResample *o = st == AFX_OK ? (struct OpaqueResample *)calloc(1, sizeof(*o)) : NULL;
    if (!o) {
        afx_resample_plan_free(&p);
        return st != AFX_OK ? st : AFX_ERR_NOMEM;
    }
    o->plan = p;
    st = afxdev_stream_create(&o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dTable, sizeof(float) * ((size_t)p.interpLength + 1));
    if (st == AFX_OK) st = table_upload(o);
    if (st != AFX_OK) {
        resampleObj_free(o);
        return st;
    }
    *handle = o;
    return 0;
}

int resampleObj_new(ResampleObj *resampleObj, ResampleQualityType *qualType, int *isScale, int *isContinue) {
    ResampleQualityType best = ResampleQuality_Best;
    return resample_new(resampleObj, qualType ? qualType : &best, NULL, NULL, NULL, NULL, NULL, isScale, isContinue);
}

int resampleObj_newWithWindow(ResampleObj *resampleObj, int *zeroNum, int *nbit, WindowType *winType, float *value, float *rollOff,
                              int *isScale, int *isContinue) {
    return resample_new(resampleObj, NULL, zeroNum, nbit, winType, value, rollOff, isScale, isContinue);
}

int resampleObj_calDataLength(ResampleObj o, int dataLength) { return o ? afx_resample_plan_length(&o->plan, dataLength) : 0; }

/* a setter: the kernels that read the table are waited for before it changes, then it is uploaded again */
static void resample_rate(ResampleObj o, int sourceRate, int targetRate, float ratio, const char *who) {
    if (!o) return;
    AFX_ENTER(o);
    int st = afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->batchStream);
    if (st == AFX_OK && plan_rate(&o->plan, sourceRate, targetRate, ratio) == 2) st = table_upload(o);
    if (st != AFX_OK) AFX_FAIL(o, st, who);
}
void resampleObj_setSamplate(ResampleObj o, int sourceRate, int targetRate) {
    if (sourceRate == targetRate || sourceRate <= 0 || targetRate <= 0) return;
    resample_rate(o, sourceRate, targetRate, 0.f, "resampleObj_setSamplate");
}
void resampleObj_setSamplateRatio(ResampleObj o, float ratio) { resample_rate(o, 0, 0, ratio, "resampleObj_setSamplateRatio"); }

void resampleObj_enableContinue(ResampleObj o, int flag) {
    if (o) o->plan.isContinue = flag;
}

/* one launch over `batch` clips */
static int resample_run(const struct OpaqueResample *o, const float *dData, int batch, int source, long long clipStride, int target,
                        float *dOut, long long outStride, void *stream) {
    const AfxResamplePlan *p = &o->plan;
    AfxResampleArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dData;
    a.clipStride = clipStride;
    a.batch = batch;
    a.sourceLength = source;
    a.targetLength = target;
    a.ratio = p->ratio;
    a.bitLength = p->bitLength;
    a.interpLength = p->interpLength;
    a.table = o->dTable;
    a.outScale = p->isScale ? sqrtf(p->ratio) : 1.f;
    a.out = dOut;
    a.outStride = outStride;
    return afxk_resample(&a, stream);
}

/* the lengths of a call, or the refusal of a ratio the kernel cannot index with */
static int resample_lengths(const struct OpaqueResample *o, int dataLength, int *source, const char *who) {
    const AfxResamplePlan *p = &o->plan;
    const long long target = plan_length(p, dataLength, source);
    if (target < 0 || (target > 0 && p->step < 1)) {
        afxdev_set_error("%s: ratio %g with 2^%d table entries per zero crossing and %d samples", who, (double)p->ratio, p->nbit, dataLength);
        return AFX_ERR_ARG;
    }
    return (int)target;
}

int resampleObj_resample(ResampleObj o, float *dataArr1, int dataLength1, float *dataArr2) {
    static const char who[] = "resampleObj_resample";
    if (!o) {
        afxdev_set_error("%s: NULL object", who);
        afxdev_report_failure(who, AFX_ERR_ARG);
        return AFX_ERR_ARG;
    }
    AFX_ENTER(o);
    int source = 0;
    int st = dataArr1 && dataArr2 && dataLength1 > 0 ? AFX_OK : AFX_ERR_ARG;
    const int target = st == AFX_OK ? resample_lengths(o, dataLength1, &source, who) : st;
    if (target < 0) st = target;
    if (st == AFX_OK && target == 0) return 0;
    const size_t inB = sizeof(float) * (size_t)source, outB = sizeof(float) * (size_t)(target > 0 ? target : 0);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dX, &o->capX, inB);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dOut, &o->capOut, outB);
    if (st == AFX_OK) st = afxdev_h2d(o->dX, dataArr1, inB, o->stream);
    if (st == AFX_OK) st = resample_run(o, o->dX, 1, source, source, target, o->dOut, target, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(dataArr2, o->dOut, outB, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) {
        AFX_FAIL(o, st, who);
        return st;
    }
    return target;
}

int resampleObj_resampleBatchDevice(ResampleObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dOut,
                                    long long outStride, void *hipStream) {
    static const char who[] = "resampleObj_resampleBatchDevice";
    if (!o || !dData || !dOut || batch <= 0 || dataLength <= 0 || clipStride < dataLength) return AFX_ERR_ARG;
    if (o->plan.isContinue) {
        afxdev_set_error("%s: a batched call on an object that belongs to one signal (isContinue = 1)", who);
        return AFX_ERR_UNSUPPORTED;
    }
    int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    int source = 0;
    const int target = resample_lengths(o, dataLength, &source, who);
    if (target <= 0) return target;
    if (outStride < target) return AFX_ERR_ARG;
    st = afx_scratch_enter(&o->batchStream, hipStream); /* (no scratch: the table's readers, for the setters) */
    if (st == AFX_OK) st = resample_run(o, dData, batch, source, clipStride, target, dOut, outStride, hipStream);
    return st == AFX_OK ? target : st;
}

void resampleObj_debug(ResampleObj o) {
    if (!o) return;
    const AfxResamplePlan *p = &o->plan;
    printf("resampleObj params is: zeroNum=%d, nbit=%d, interpLength=%d, winType=%d, value=%g, rollOff=%g, isScale=%d, isContinue=%d, "
           "ratio=%g, p=%d, q=%d, sourceRate=%d, targetRate=%d\n", p->zeroNum, p->nbit, p->interpLength, p->winType, (double)p->value,
           (double)p->rollOff, p->isScale, p->isContinue, (double)p->ratio, p->p, p->q, p->sourceRate, p->targetRate);
}
