/* afx_pitchshift.c -- the pitch-shift object (C host side) behind include/mir/pitchShift_algorithm.h.
 *
 * Mirrors the reference object (src/mir/pitchShift_algorithm.c:28-89): rate = powf(2, -nSemitone / 12), a time stretch by that
 * rate into a zero-tailed buffer of roundf(n / rate) samples, the Fast resampler with isScale at ratio `rate`.  Execution, per
 * chunk of whole clips: timeStretchObj_timeStretchBatchDevice into scratch rows (the inverse transform's samples, then
 * zeros), resampleObj_resampleBatchDevice into scratch rows, and a row copy of at most dataLength samples to the caller.
 * There is no CPU compute path.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "dsp/resample_algorithm.h"
#include "mir/pitchShift_algorithm.h"
#include "mir/timeStretch_algorithm.h"

static size_t align4(size_t floats) { return (floats + 3) & ~(size_t)3; }

int pitchShiftObj_new(PitchShiftObj *pitchShiftObj, int *radix2Exp, int *slideLength, WindowType *windowType) {
    if (!pitchShiftObj) return AFX_ERR_ARG;
    *pitchShiftObj = NULL;
    PitchShiftObj o = (PitchShiftObj)calloc(1, sizeof(struct OpaquePitchShift));
    if (!o) return AFX_ERR_NOMEM;
    o->scratchLimit = AFX_TIMESTRETCH_SCRATCH_BYTES;
    int scale = 1;
    ResampleQualityType qual = ResampleQuality_Fast;
    int st = timeStretchObj_new(&o->stretch, radix2Exp, slideLength, windowType);
    if (st == 0) st = resampleObj_new(&o->resample, &qual, &scale, NULL);
    if (st != 0) {
        pitchShiftObj__free(o);
        return st;
    }
    o->stream = o->stretch->stream;
    *pitchShiftObj = o;
    return 0;
}

void pitchShiftObj_setScratchLimit(PitchShiftObj o, long long bytes) {
    if (!o) return;
    o->scratchLimit = bytes > 0 ? bytes : AFX_TIMESTRETCH_SCRATCH_BYTES;
    timeStretchObj_setScratchLimit(o->stretch, bytes);
}

/* 0: nothing to do (|nSemitone| > 12, pitchShift_algorithm.c:59); else the samples written per clip, or a status */
static int run(PitchShiftObj o, int nSemitone, const float *dData, int batch, int dataLength, long long clipStride, float *dOut,
               long long outStride, void *stream) {
    if (nSemitone > 12 || nSemitone < -12) return 0;
    const float rate = powf(2, (float)(-nSemitone * 1.0 / 12));
    AfxTimeStretchPlan p;
    int st = afx_timestretch_plan(o->stretch->radix2Exp, o->stretch->slideLength, rate, dataLength, batch, 0, &p, NULL, NULL);
    if (st != AFX_OK) return st;
    const int stretched = p.returnLength;
    /* the setter waits for the table's readers and uploads when the table changed: only when the rate is a new one */
    if (!o->rateSet || o->lastRate != rate) {
        const int errors = afxdev_error_count();
        o->rateSet = 0;
        resampleObj_setSamplateRatio(o->resample, rate);
        if (afxdev_error_count() != errors) return o->resample->status;
        o->lastRate = rate;
        o->rateSet = 1;
    }
    const int target = resampleObj_calDataLength(o->resample, stretched);
    const int written = target < dataLength ? target : dataLength;
    if (stretched <= 0 || written <= 0) return 0;
    if (outStride < written) return AFX_ERR_ARG;
    st = afx_scratch_enter(&o->scratchStream, stream); /* dScratch */
    if (st != AFX_OK) return st;
    const size_t rowS = align4((size_t)stretched), rowT = align4((size_t)target);
    long long chunk = o->scratchLimit / (long long)(sizeof(float) * (rowS + rowT));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    st = afxdev_reserve((void **)&o->dScratch, &o->capScratch, sizeof(float) * (rowS + rowT) * (size_t)chunk);
    if (st != AFX_OK) return st;
    for (int c0 = 0; c0 < batch; c0 += (int)chunk) {
        const int nc = batch - c0 < (int)chunk ? batch - c0 : (int)chunk;
        float *s = o->dScratch, *t = s + rowS * (size_t)nc;
        st = timeStretchObj_timeStretchBatchDevice(o->stretch, rate, dData + (long long)c0 * clipStride, nc, dataLength, clipStride, s,
                                                   (long long)rowS, stream);
        if (st != stretched) return st < 0 ? st : AFX_ERR_ARG;
        st = resampleObj_resampleBatchDevice(o->resample, s, nc, stretched, (long long)rowS, t, (long long)rowT, stream);
        if (st != target) return st < 0 ? st : AFX_ERR_ARG;
        st = afxk_rows_fit(t, (long long)rowT, target, dOut + (long long)c0 * outStride, outStride, written, nc, stream);
        if (st != AFX_OK) return st;
    }
    return written;
}

int pitchShiftObj_pitchShiftBatchDevice(PitchShiftObj o, int nSemitone, const float *dData, int batch, int dataLength,
                                        long long clipStride, float *dOut, long long outStride, void *hipStream) {
    if (!o || !dData || !dOut || batch <= 0 || dataLength <= 0 || clipStride < dataLength) return AFX_ERR_ARG;
    const int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    return run(o, nSemitone, dData, batch, dataLength, clipStride, dOut, outStride, hipStream);
}

void pitchShiftObj_pitchShift(PitchShiftObj o, int samplate, int nSemitone, float *dataArr1, int dataLength1, float *dataArr2) {
    static const char who[] = "pitchShiftObj_pitchShift";
    (void)samplate; /* pitchShift_algorithm.c:64: computed, never used */
    if (!o) {
        afxdev_set_error("%s: NULL object", who);
        afxdev_report_failure(who, AFX_ERR_ARG);
        return;
    }
    AFX_ENTER(o);
    if (nSemitone > 12 || nSemitone < -12) return;
    int st = AFX_OK;
    if (!dataArr1 || !dataArr2 || dataLength1 <= 0) {
        afxdev_set_error("%s: NULL array or no samples", who);
        st = AFX_ERR_ARG;
    }
    const size_t bytes = sizeof(float) * (size_t)(st == AFX_OK ? dataLength1 : 0);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dX, &o->capX, bytes);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dOut, &o->capOut, bytes);
    if (st == AFX_OK) st = afxdev_h2d(o->dX, dataArr1, bytes, o->stream);
    if (st == AFX_OK) st = run(o, nSemitone, o->dX, 1, dataLength1, dataLength1, o->dOut, dataLength1, o->stream);
    if (st > 0) st = afxdev_d2h(dataArr2, o->dOut, sizeof(float) * (size_t)st, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) AFX_FAIL(o, st, who);
}

void pitchShiftObj__free(PitchShiftObj o) {
    if (!o) return;
    if (o->stream) afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->scratchStream);
    afxdev_free(o->dScratch);
    afxdev_free(o->dX);
    afxdev_free(o->dOut);
    resampleObj_free(o->resample);
    timeStretchObj_free(o->stretch); /* destroys the stream */
    free(o);
}
