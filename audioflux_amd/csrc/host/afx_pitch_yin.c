/* afx_pitch_yin.c -- the YIN pitch tracker object (C host side) behind include/mir/_pitch_yin.h and the device-pointer
 * calls of include/afx_batch.h.
 *
 * Mirrors the parameter semantics of the reference object (src/mir/_pitch_yin.c:87-196): defaults, clamps and the lag
 * range evaluated in float32.  Execution: ONE kernel launch per call (k_pitch_yin, afx_pitch_yin.hip) from the samples to
 * frequency / trough / min per frame, plus the candidate lists for the host-pointer call.  The host-pointer call is the
 * batch of one through staging buffers; it carries the isContinue tail (afx_frametail.h) and merges the result so that
 * frames without a trough keep the caller's freArr / valueArr1 entries.  There is no CPU compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_frametail.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/_pitch_yin.h"

#define YIN_MIN_EXP 6
#define YIN_MAX_EXP 13

typedef struct {
    int samplate, radix2Exp, fftLength, slideLength, autoLength, isContinue;
    float lowFre, highFre;
    int minIndex, maxIndex, diffLength, yinLength;
} YinPlan;

/* defaults, clamps and refusals of pitchYINObj_new that need no device (_pitch_yin.c:87-196) */
static int yin_plan(const int *samplate, const float *lowFre, const float *highFre, const int *radix2Exp, const int *slideLength,
                    const int *autoLength, const int *isContinue, YinPlan *p) {
    memset(p, 0, sizeof(*p));
    p->samplate = 32000;
    p->lowFre = 27.f;
    p->highFre = 2094.f;
    p->radix2Exp = 12;
    if (samplate && *samplate > 0 && *samplate <= 196000) p->samplate = *samplate;
    if (lowFre && *lowFre >= 27) p->lowFre = *lowFre;
    if (highFre) {
        /* (samplate / 2 is an integer division there, too) */
        if (*highFre > p->lowFre && *highFre < p->samplate / 2) {
            p->highFre = *highFre;
        } else {
            p->lowFre = 27.f;
            p->highFre = 2093.f;
        }
    }
    if (radix2Exp) {
        if (*radix2Exp < YIN_MIN_EXP || *radix2Exp > YIN_MAX_EXP) return -100;
        p->radix2Exp = *radix2Exp;
    }
    p->fftLength = 1 << p->radix2Exp;
    p->slideLength = (slideLength && *slideLength > 0) ? *slideLength : p->fftLength / 4;
    p->autoLength = (autoLength && *autoLength >= 0 && *autoLength < p->fftLength) ? *autoLength : p->fftLength / 2;
    p->diffLength = p->fftLength - p->autoLength;
    p->isContinue = isContinue ? *isContinue : 0;
    p->minIndex = (int)floorf((float)p->samplate / p->highFre);
    p->maxIndex = (int)ceilf((float)p->samplate / p->lowFre);
    if (p->maxIndex > p->diffLength - 1) p->maxIndex = p->diffLength - 1;
    p->yinLength = p->maxIndex - p->minIndex + 1;
    if (p->minIndex < 1) {
        afxdev_set_error("pitchYINObj_new: samplate %d / highFre %g puts the first lag at 0", p->samplate, (double)p->highFre);
        return AFX_ERR_ARG;
    }
    if (p->yinLength < 3) {
        afxdev_set_error("pitchYINObj_new: lags %d ... %d (autoLength %d of %d): fewer than 3", p->minIndex, p->maxIndex, p->autoLength,
                         p->fftLength);
        return AFX_ERR_ARG;
    }
    return 0;
}

int pitchYINObj_new(PitchYINObj *pitchYINObj, int *samplate, float *lowFre, float *highFre, int *radix2Exp, int *slideLength,
                    int *autoLength, int *isContinue) {
    if (!pitchYINObj) return -1;
    *pitchYINObj = NULL;
    YinPlan p;
    int st = yin_plan(samplate, lowFre, highFre, radix2Exp, slideLength, autoLength, isContinue, &p);
    if (st != 0) return st;
    st = afxdev_ensure();
    if (st != AFX_OK) return st;
    PitchYINObj o = (PitchYINObj)calloc(1, sizeof(struct OpaquePitchYIN));
    if (!o) return AFX_ERR_NOMEM;
    o->autoLength = p.autoLength;
    o->minIndex = p.minIndex;
    o->maxIndex = p.maxIndex;
    o->diffLength = p.diffLength;
    o->yinLength = p.yinLength;
    o->thresh = 0.1f;
    st = afx_pitch_head_init(&o->head, p.radix2Exp, p.slideLength, p.samplate, p.isContinue);
    float *tw = NULL;
    if (st == AFX_OK) {
        tw = afx_twiddle_table(p.fftLength);
        if (!tw) st = AFX_ERR_NOMEM;
    }
    st = afx_pitch_table(st, &o->dTwiddle, tw, sizeof(float) * (size_t)p.fftLength, o->head.stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->head.stream);
    free(tw);
    if (st != AFX_OK) {
        pitchYINObj_free(o);
        return st;
    }
    *pitchYINObj = o;
    return 0;
}

void pitchYINObj_setThresh(PitchYINObj o, float thresh) {
    if (o && thresh > 0) o->thresh = thresh;
}

int pitchYINObj_calTimeLength(PitchYINObj o, int dataLength) { return afx_pitch_frames(AFX_PITCH_HEAD(o), dataLength); }

int pitchYINObj_yinLength(PitchYINObj o) { return o ? o->yinLength : 0; }
int pitchYINObj_minIndex(PitchYINObj o) { return o ? o->minIndex : 0; }

static void fill_args(const struct OpaquePitchYIN *o, const float *dData, int batch, int dataLength, long long clipStride, int T,
                      AfxPitchYinArgs *a) {
    memset(a, 0, sizeof(*a));
    a->x = dData;
    a->clipStride = clipStride;
    a->batch = batch;
    a->dataLength = dataLength;
    a->timeLength = T;
    a->radix2Exp = o->head.radix2Exp;
    a->hop = o->head.slideLength;
    a->autoLength = o->autoLength;
    a->minIndex = o->minIndex;
    a->maxIndex = o->maxIndex;
    a->samplate = o->head.samplate;
    a->thresh = o->thresh;
    a->twiddle = o->dTwiddle;
}

int pitchYINObj_pitchBatchDevice(PitchYINObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dFre,
                                 float *dTrough, float *dMin, long long outStride, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "pitchYINObj", dData, batch, dataLength, clipStride, dFre, hipStream, &T);
    if (go <= 0) return go;
    if (outStride < T) return AFX_ERR_ARG;
    AfxPitchYinArgs a;
    fill_args(o, dData, batch, dataLength, clipStride, T, &a);
    a.fre = dFre;
    a.trough = dTrough;
    a.minv = dMin;
    a.outStride = outStride;
    return afxk_pitch_yin(&a, hipStream);
}

int pitchYINObj_troughsBatchDevice(PitchYINObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dFre,
                                   float *dVal, int *dLen, int troughPitch, void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "pitchYINObj", dData, batch, dataLength, clipStride, dLen, hipStream, &T);
    if (go <= 0) return go;
    if (troughPitch < 0 || (troughPitch > 0 && (!dFre || !dVal))) return AFX_ERR_ARG;
    AfxPitchYinArgs a;
    fill_args(o, dData, batch, dataLength, clipStride, T, &a);
    a.candFre = troughPitch > 0 ? dFre : NULL;
    a.candVal = troughPitch > 0 ? dVal : NULL;
    a.candLen = dLen;
    a.candPitch = troughPitch;
    return afxk_pitch_yin(&a, hipStream);
}

int pitchYINObj_curveBatchDevice(PitchYINObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dYin,
                                 void *hipStream) {
    int T = 0;
    const int go = afx_pitch_batch_enter(AFX_PITCH_HEAD(o), "pitchYINObj", dData, batch, dataLength, clipStride, dYin, hipStream, &T);
    if (go <= 0) return go;
    AfxPitchYinArgs a;
    fill_args(o, dData, batch, dataLength, clipStride, T, &a);
    a.curve = dYin;
    return afxk_pitch_yin(&a, hipStream);
}

/* host arrays of T frames: staging [3][T], candidate lists [T, mLen], lengths [T] */
static int reserve_host(PitchYINObj o, int T) {
    if ((size_t)T <= o->capHost) return AFX_OK;
    const size_t mLen = (size_t)o->yinLength / 2 + 1;
    float *h = (float *)malloc(sizeof(float) * 3 * (size_t)T);
    float *f = (float *)calloc((size_t)T * mLen, sizeof(float));
    float *v = (float *)calloc((size_t)T * mLen, sizeof(float));
    int *l = (int *)calloc((size_t)T, sizeof(int));
    if (!h || !f || !v || !l) {
        free(h);
        free(f);
        free(v);
        free(l);
        return AFX_ERR_NOMEM;
    }
    free(o->hOut);
    free(o->mFreArr);
    free(o->mTroughArr);
    free(o->lenArr);
    o->hOut = h;
    o->mFreArr = f;
    o->mTroughArr = v;
    o->lenArr = l;
    o->capHost = (size_t)T;
    return AFX_OK;
}

void pitchYINObj_pitch(PitchYINObj o, float *dataArr, int dataLength, float *freArr, float *valueArr1, float *valueArr2) {
    static const char *who = "pitchYINObj_pitch";
    if (!o) {
        afxdev_set_error("%s: NULL object", who);
        return;
    }
    AfxPitchHead *h = &o->head;
    AFX_ENTER(h);
    AfxFrameTake t;
    const int T = afx_pitch_call_begin(h, dataArr, dataLength, &t, who);
    if (T <= 0) return;
    const int n = t.total;
    int st = freArr ? AFX_OK : AFX_ERR_ARG;
    const int mLen = o->yinLength / 2 + 1;
    const size_t rowB = sizeof(float) * (size_t)T, candF = (size_t)T * (size_t)mLen;
    if (st == AFX_OK) st = reserve_host(o, T);
    if (st == AFX_OK) st = afx_frametail_upload(&h->tail, &t, dataArr, &h->dX, &h->capX, h->stream);
    if (st == AFX_OK) st = afxdev_reserve((void **)&h->dOut, &h->capOut, 3 * rowB);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dCand, &o->capCand, sizeof(float) * 2 * candF + sizeof(int) * (size_t)T);
    if (st == AFX_OK) {
        AfxPitchYinArgs a;
        fill_args(o, h->dX, 1, n, n, T, &a);
        a.fre = h->dOut;
        a.trough = h->dOut + T;
        a.minv = h->dOut + 2 * (size_t)T;
        a.outStride = T;
        a.candFre = o->dCand;
        a.candVal = o->dCand + candF;
        a.candLen = (int *)(o->dCand + 2 * candF);
        a.candPitch = mLen;
        st = afxk_pitch_yin(&a, h->stream);
    }
    if (st == AFX_OK) st = afxdev_d2h(o->hOut, h->dOut, 3 * rowB, h->stream);
    if (st == AFX_OK) st = afxdev_d2h(o->lenArr, o->dCand + 2 * candF, sizeof(int) * (size_t)T, h->stream);
    /* the kernel writes min(len, mLen) entries per frame; rows are fetched whole and the rest of a row is zeroed below */
    if (st == AFX_OK) st = afxdev_d2h(o->mFreArr, o->dCand, sizeof(float) * candF, h->stream);
    if (st == AFX_OK) st = afxdev_d2h(o->mTroughArr, o->dCand + candF, sizeof(float) * candF, h->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(h->stream);
    if (afx_pitch_call_end(h, dataArr, dataLength, st, who) != AFX_OK) return;
    for (int i = 0; i < T; ++i) {
        const float *h = o->hOut;
        if (h[i] != 0.f) { /* a found frequency is never 0: 0 marks "no trough", the caller's entries stay (_pitch_yin.c:548-551) */
            freArr[i] = h[i];
            if (valueArr1) valueArr1[i] = h[T + i];
        }
        if (valueArr2) valueArr2[i] = h[2 * (size_t)T + i];
        /* entries behind a frame's count: zero, not stale device memory */
        int stored = o->lenArr[i];
        if (stored < 0) stored = 0;
        for (int j = stored; j < mLen; ++j) o->mFreArr[(size_t)i * mLen + j] = o->mTroughArr[(size_t)i * mLen + j] = 0.f;
    }
}

int pitchYINObj_getTroughData(PitchYINObj o, float **mFreArr, float **mTroughArr, int **lenArr) {
    if (!o) return 0;
    if (mFreArr) *mFreArr = o->mFreArr;
    if (mTroughArr) *mTroughArr = o->mTroughArr;
    if (lenArr) *lenArr = o->lenArr;
    return o->yinLength / 2 + 1;
}

void pitchYINObj_enableDebug(PitchYINObj o, int isDebug) {
    if (!o) return;
    o->head.isDebug = isDebug;
    if (isDebug)
        printf("pitchYIN params is: samplate=%d, fftLength=%d, slideLength=%d, autoLength=%d, minIndex=%d, maxIndex=%d, thresh=%g\n",
               o->head.samplate, o->head.fftLength, o->head.slideLength, o->autoLength, o->minIndex, o->maxIndex, (double)o->thresh);
}

void pitchYINObj_free(PitchYINObj o) {
    if (!o) return;
    afx_pitch_head_sync(&o->head);
    afxdev_free(o->dTwiddle);
    afxdev_free(o->dCand);
    afx_pitch_head_release(&o->head);
    free(o->hOut);
    free(o->mFreArr);
    free(o->mTroughArr);
    free(o->lenArr);
    free(o);
}

/* ---- test hooks (host logic only, no device): tests/test_pitch_cpu.py ------------------------------------------------ */
/* what pitchYINObj_new would decide: out = {status, samplate, fftLength, slideLength, autoLength, minIndex, maxIndex, diffLength,
 * yinLength, isContinue}, lowHigh = {lowFre, highFre} */
int afx_test_pitch_yin_plan(const int *samplate, const float *lowFre, const float *highFre, const int *radix2Exp,
                            const int *slideLength, const int *autoLength, const int *isContinue, int *out, float *lowHigh) {
    YinPlan p;
    const int st = yin_plan(samplate, lowFre, highFre, radix2Exp, slideLength, autoLength, isContinue, &p);
    out[0] = st;
    out[1] = p.samplate;
    out[2] = p.fftLength;
    out[3] = p.slideLength;
    out[4] = p.autoLength;
    out[5] = p.minIndex;
    out[6] = p.maxIndex;
    out[7] = p.diffLength;
    out[8] = p.yinLength;
    out[9] = p.isContinue;
    lowHigh[0] = p.lowFre;
    lowHigh[1] = p.highFre;
    return st;
}

/* the framing state machine over a sequence of calls on data[0 ...]: per call the frames, the tail afterwards, the length of
 * the framed signal and a checksum of it (sum of sample * (index + 1) in double); returns 0 or a status */
int afx_test_frametail(int frameLength, int hop, int isContinue, const float *data, const int *callLengths, int calls, int *frames,
                       int *tails, int *curLengths, double *sums) {
    AfxFrameTail f;
    int st = afx_frametail_init(&f, frameLength, hop, isContinue);
    long long at = 0;
    for (int c = 0; st == AFX_OK && c < calls; ++c) {
        const float *piece = data + at;
        AfxFrameTake t;
        const int T = afx_frametail_take(&f, callLengths[c], &t);
        if (T < 0) st = T;
        frames[c] = T;
        curLengths[c] = t.total;
        double s = 0.0; /* over [tail head | piece past the skip], as the object uploads it */
        for (int i = 0; i < t.total; ++i) s += (double)(i < t.head ? f.tail[i] : piece[t.skip + i - t.head]) * (double)(i + 1);
        sums[c] = s;
        if (T >= 0) afx_frametail_keep(&f, piece, callLengths[c]);
        tails[c] = f.tailLength;
        at += callLengths[c];
    }
    afx_frametail_free(&f);
    return st;
}
