/* afx_timestretch.c -- the time-stretch object (C host side) behind include/mir/timeStretch_algorithm.h.
 *
 * Mirrors the parameter semantics of the reference object (src/mir/timeStretch_algorithm.c:34-164): radix2Exp 12, hop
 * fftLength / 4 and Hann by default, T1 = (n - N) / hop + 1 frames in, T2 = ceilf(T1 / rate) frames out, the weighted
 * overlap-add inverse, roundf(n / rate) returned.  Execution, per chunk of whole clips: the owned STFT object's forward kernel
 * stores the half spectrum, the phase vocoder (afx_phasevocoder.hip) turns it into polar form in place and writes the full
 * output spectrum, the STFT object's inverse adds the frames onto a zeroed scratch row, and a row copy cuts or zero-tails
 * that row to the length the call writes.  Everything is enqueued on one stream; the scratch of a chunk is bounded by the
 * object's limit and reused.  There is no CPU compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/timeStretch_algorithm.h"
#include "stft_algorithm.h"

#define TS_MAX_EXP 14
#define TS_MAX_CHUNK 65535 /* clips of one vocoder launch */

static size_t align4(size_t floats) { return (floats + 3) & ~(size_t)3; }

/* ---- the plan: everything that needs no device ---------------------------------------------------------------------------- */

/* defaults and refusals of the constructor (timeStretch_algorithm.c:47-59) */
static int plan_sizes(const int *radix2Exp, const int *slideLength, int *exp, int *hop) {
    *exp = radix2Exp && *radix2Exp >= 1 && *radix2Exp <= 30 ? *radix2Exp : 12;
    if (*exp > TS_MAX_EXP) {
        afxdev_set_error("timeStretchObj_new: fftLength 2^%d exceeds the on-chip FFT limit 2^%d", *exp, TS_MAX_EXP);
        return AFX_ERR_UNSUPPORTED;
    }
    const int N = 1 << *exp;
    *hop = slideLength && *slideLength > 0 ? *slideLength : N / 4;
    if (*hop < 1) *hop = 1; /* (fftLength 2: the reference's default of 0 divides by zero in its frame count) */
    if (*hop > N) {
        afxdev_set_error("timeStretchObj_new: slideLength %d above fftLength %d leaves samples no frame covers", *hop, N);
        return AFX_ERR_UNSUPPORTED;
    }
    return AFX_OK;
}

/* floats of one clip's scratch: every plane and row starts on a 16-byte boundary whatever the chunk holds */
static size_t clip_floats(const AfxTimeStretchPlan *p) {
    const size_t N = (size_t)p->fftLength, F = N / 2 + 1;
    return 2 * align4((size_t)p->T2 * N) + 2 * align4((size_t)p->T1 * F) + align4((size_t)p->istftLength);
}

static int plan_call(int exp, int hop, float rate, int dataLength, int batch, long long limit, AfxTimeStretchPlan *p) {
    memset(p, 0, sizeof(*p));
    const int N = p->fftLength = 1 << exp;
    p->slideLength = hop;
    if (!(rate > 0.f) || !(rate <= 3.0e38f)) {
        afxdev_set_error("time stretch: rate %g is not a positive finite number", (double)rate);
        return AFX_ERR_ARG;
    }
    p->T1 = afx_frames(dataLength, N, hop);
    if (p->T1 <= 0) {
        afxdev_set_error("time stretch: %d samples hold no frame of %d", dataLength, N);
        return AFX_ERR_ARG;
    }
    p->T2 = afx_pv_frames(p->T1, rate);
    const float q = (float)dataLength / rate; /* timeStretch_algorithm.c:79, :148 */
    const long long L2 = ((long long)p->T2 - 1) * hop + N;
    if (p->T2 <= 0 || L2 > 0x7fffffff || !(ceilf(q) + (float)N < 2147483648.f)) {
        afxdev_set_error("time stretch: rate %g stretches %d samples beyond the sizes a call takes", (double)rate, dataLength);
        return AFX_ERR_ARG;
    }
    p->istftLength = (int)L2;
    p->returnLength = (int)roundf(q);
    p->capacity = (int)(ceilf(q) + (float)N);
    const size_t floats = clip_floats(p);
    p->scratchBytes = (long long)(sizeof(float) * floats);
    if (limit <= 0) limit = AFX_TIMESTRETCH_SCRATCH_BYTES;
    long long chunk = limit / p->scratchBytes;
    if (chunk < 1) chunk = 1;
    if (chunk > TS_MAX_CHUNK) chunk = TS_MAX_CHUNK;
    if (batch > 0 && chunk > batch) chunk = batch;
    /* (a launch of the transforms takes at most 2^31 - 1 frames) */
    while (chunk > 1 && chunk * (p->T2 > p->T1 ? p->T2 : p->T1) > 0x7fffffffLL) chunk /= 2;
    p->clipsPerChunk = (int)chunk;
    return AFX_OK;
}

int afx_timestretch_plan(int radix2Exp, int slideLength, float rate, int dataLength, int batch, long long scratchLimit,
                         AfxTimeStretchPlan *plan, int *kArr, float *alphaArr) {
    if (!plan) return AFX_ERR_ARG;
    memset(plan, 0, sizeof(*plan));
    int exp, hop;
    int st = plan_sizes(&radix2Exp, &slideLength, &exp, &hop);
    if (st != AFX_OK) return st;
    st = plan_call(exp, hop, rate, dataLength, batch, scratchLimit, plan);
    if (st != AFX_OK) return st;
    for (int i = 0; i < plan->T2 && (kArr || alphaArr); i++) {
        float alpha;
        const int k = afx_pv_time(i, rate, &alpha);
        if (kArr) kArr[i] = k;
        if (alphaArr) alphaArr[i] = alpha;
    }
    return AFX_OK;
}

/* ---- the object ----------------------------------------------------------------------------------------------------------- */

int timeStretchObj_new(TimeStretchObj *timeStretchObj, int *radix2Exp, int *slideLength, WindowType *windowType) {
    if (!timeStretchObj) return AFX_ERR_ARG;
    *timeStretchObj = NULL;
    int exp, hop;
    int st = plan_sizes(radix2Exp, slideLength, &exp, &hop);
    if (st != AFX_OK) return st;
    TimeStretchObj o = (TimeStretchObj)calloc(1, sizeof(struct OpaqueTimeStretch));
    if (!o) return AFX_ERR_NOMEM;
    o->radix2Exp = exp;
    o->fftLength = 1 << exp;
    o->slideLength = hop;
    o->scratchLimit = AFX_TIMESTRETCH_SCRATCH_BYTES;
    WindowType wt = windowType ? *windowType : Window_Hann;
    st = stftObj_new(&o->stft, exp, &wt, &hop, NULL);
    if (st == 0) {
        o->stream = o->stft->stream;
        /* the window never changes: uploaded here, so that no compute call has to */
        st = afxdev_h2d(o->stft->dWindow, o->stft->windowDataArr, sizeof(float) * (size_t)o->fftLength, o->stream);
        if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
        if (st == AFX_OK) o->stft->windowDirty = 0;
    }
    if (st != 0) {
        timeStretchObj_free(o);
        return st;
    }
    *timeStretchObj = o;
    return 0;
}

void timeStretchObj_setScratchLimit(TimeStretchObj o, long long bytes) {
    if (o) o->scratchLimit = bytes > 0 ? bytes : AFX_TIMESTRETCH_SCRATCH_BYTES;
}

int timeStretchObj_calDataCapacity(TimeStretchObj o, float rate, int dataLength) {
    if (!o || !(rate > 0.f) || !(rate <= 3.0e38f)) return 0;
    const float v = ceilf((float)dataLength / rate) + (float)o->fftLength;
    return v < 2147483648.f && v > -2147483648.f ? (int)v : 0;
}

/* chunks of whole clips: forward half spectrum -> vocoder -> inverse onto zeros -> the first outLength words of every row
 * (the inverse's samples, zeros behind them) */
static int run(TimeStretchObj o, const AfxTimeStretchPlan *p, float rate, const float *dData, int batch, int dataLength,
               long long clipStride, float *dOut, long long outStride, int outLength, void *stream) {
    const int N = o->fftLength, F = N / 2 + 1, hop = o->slideLength, T1 = p->T1, T2 = p->T2;
    int st = afx_scratch_enter(&o->scratchStream, stream); /* dScratch */
    if (st != AFX_OK) return st;
    const int chunk = p->clipsPerChunk < batch ? p->clipsPerChunk : batch;
    st = afxdev_reserve((void **)&o->dScratch, &o->capScratch, sizeof(float) * clip_floats(p) * (size_t)chunk);
    if (st != AFX_OK) return st;
    const size_t rowY = align4((size_t)p->istftLength);
    for (int c0 = 0; c0 < batch; c0 += chunk) {
        const int nc = batch - c0 < chunk ? batch - c0 : chunk;
        const size_t A = align4((size_t)nc * T2 * N), B = align4((size_t)nc * T1 * F);
        float *re2 = o->dScratch, *im2 = re2 + A, *sRe = im2 + A, *sIm = sRe + B, *y = sIm + B;
        AfxStftArgs s;
        afx_stft_args(&s, dData + (long long)c0 * clipStride, clipStride, nc, dataLength, T1, o->radix2Exp, hop, o->stft->dWindow,
                      o->stft->dTwiddle, AFX_SPEC_COMPLEX, 0, F, sRe, sIm);
        st = afxk_stft(&s, stream);
        if (st != AFX_OK) return st;
        AfxPhaseVocoderArgs v;
        memset(&v, 0, sizeof(v));
        v.re = v.mag = sRe; /* polar form in place */
        v.im = v.ang = sIm;
        v.inPitch = F;
        v.batch = nc;
        v.T1 = T1;
        v.T2 = T2;
        v.radix2Exp = o->radix2Exp;
        v.hop = hop;
        v.rate = rate;
        v.outRe = re2;
        v.outIm = im2;
        st = afxk_phase_vocoder(&v, stream);
        /* weighted overlap-add (type 0, timeStretch_algorithm.c:146) onto zeros */
        if (st == AFX_OK) st = afxdev_memset(y, 0, sizeof(float) * rowY * (size_t)nc, stream);
        if (st == AFX_OK) st = stftObj_istftBatchDevice(o->stft, re2, im2, nc, T2, 0, y, (long long)rowY, stream);
        if (st == AFX_OK)
            st = afxk_rows_fit(y, (long long)rowY, p->istftLength, dOut + (long long)c0 * outStride, outStride, outLength, nc, stream);
        if (st != AFX_OK) return st;
    }
    return AFX_OK;
}

int timeStretchObj_timeStretchBatchDevice(TimeStretchObj o, float rate, const float *dData, int batch, int dataLength,
                                          long long clipStride, float *dOut, long long outStride, void *hipStream) {
    if (!o || !dData || !dOut || batch <= 0 || dataLength <= 0 || clipStride < dataLength) return AFX_ERR_ARG;
    int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    AfxTimeStretchPlan p;
    st = plan_call(o->radix2Exp, o->slideLength, rate, dataLength, batch, o->scratchLimit, &p);
    if (st != AFX_OK) return st;
    if (p.returnLength <= 0) return 0;
    if (outStride < p.returnLength) return AFX_ERR_ARG;
    st = run(o, &p, rate, dData, batch, dataLength, clipStride, dOut, outStride, p.returnLength, hipStream);
    return st == AFX_OK ? p.returnLength : st;
}

int timeStretchObj_timeStretch(TimeStretchObj o, float rate, float *dataArr1, int dataLength, float *dataArr2) {
    static const char who[] = "timeStretchObj_timeStretch";
    if (!o) {
        afxdev_set_error("%s: NULL object", who);
        afxdev_report_failure(who, AFX_ERR_ARG);
        return AFX_ERR_ARG;
    }
    AFX_ENTER(o);
    AfxTimeStretchPlan p;
    int st = AFX_OK;
    if (!dataArr1 || !dataArr2 || dataLength <= 0) {
        afxdev_set_error("%s: NULL array or no samples", who);
        st = AFX_ERR_ARG;
    }
    if (st == AFX_OK) st = plan_call(o->radix2Exp, o->slideLength, rate, dataLength, 1, o->scratchLimit, &p);
    const size_t inB = sizeof(float) * (size_t)(st == AFX_OK ? dataLength : 0), outB = sizeof(float) * (size_t)(st == AFX_OK ? p.istftLength : 0);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dX, &o->capX, inB);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dOut, &o->capOut, outB);
    if (st == AFX_OK) st = afxdev_h2d(o->dX, dataArr1, inB, o->stream);
    if (st == AFX_OK) st = run(o, &p, rate, o->dX, 1, dataLength, dataLength, o->dOut, p.istftLength, p.istftLength, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(dataArr2, o->dOut, outB, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) {
        AFX_FAIL(o, st, who);
        return st;
    }
    return p.returnLength;
}

int afx_phase_vocoder_device(const float *dRe, const float *dIm, int batch, int T1, int radix2Exp, long long pitch, int hop, float rate,
                             float *dRe2, float *dIm2, void *hipStream) {
    if (!dRe || !dIm || !dRe2 || !dIm2 || batch <= 0 || T1 <= 0 || hop <= 0 || radix2Exp < 1 || radix2Exp > TS_MAX_EXP) return AFX_ERR_ARG;
    const int N = 1 << radix2Exp, F = N / 2 + 1, T2 = afx_pv_frames(T1, rate);
    if (pitch < F || T2 <= 0) return AFX_ERR_ARG;
    int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    const int chunk = batch < TS_MAX_CHUNK ? batch : TS_MAX_CHUNK;
    const size_t plane = (size_t)chunk * T1 * F;
    float *polar = NULL;
    st = afxdev_malloc((void **)&polar, sizeof(float) * 2 * plane);
    for (int c0 = 0; st == AFX_OK && c0 < batch; c0 += chunk) {
        AfxPhaseVocoderArgs v;
        memset(&v, 0, sizeof(v));
        v.re = dRe + (long long)c0 * T1 * pitch;
        v.im = dIm + (long long)c0 * T1 * pitch;
        v.inPitch = pitch;
        v.batch = batch - c0 < chunk ? batch - c0 : chunk;
        v.T1 = T1;
        v.T2 = T2;
        v.radix2Exp = radix2Exp;
        v.hop = hop;
        v.rate = rate;
        v.mag = polar;
        v.ang = polar + plane;
        v.outRe = dRe2 + (long long)c0 * T2 * N;
        v.outIm = dIm2 + (long long)c0 * T2 * N;
        st = afxk_phase_vocoder(&v, hipStream);
    }
    /* the kernels read the scratch: it is freed behind them */
    const int sync = afxdev_stream_sync(hipStream);
    afxdev_free(polar);
    return st != AFX_OK ? st : sync;
}

void timeStretchObj_free(TimeStretchObj o) {
    if (!o) return;
    if (o->stream) afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->scratchStream);
    afxdev_free(o->dScratch);
    afxdev_free(o->dX);
    afxdev_free(o->dOut);
    stftObj_free(o->stft); /* destroys the stream */
    free(o);
}
