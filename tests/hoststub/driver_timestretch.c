/* driver_timestretch.c -- the time-stretch and pitch-shift host objects under AddressSanitizer / UBSan, as a program of its
 * own: timeStretchObj_new / calDataCapacity / timeStretch / timeStretchBatchDevice / setScratchLimit / free,
 * pitchShiftObj_new / pitchShift / pitchShiftBatchDevice / setScratchLimit / _free, afx_phase_vocoder_device and
 * afx_timestretch_plan against the generated stand-in of the device layer (gen_stub.py --omit=afxk_phase_vocoder
 * --omit=afxk_rows_fit --omit=afxk_resample).  The three launchers are supplied HERE: each reads every word its kernel reads
 * and writes every word it writes, so a scratch plane, a staging buffer or an output row that is too small is a sanitizer
 * report ("device" buffers are exactly sized); the stand-in's forward and inverse transforms do the same for theirs. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "dsp/resample_algorithm.h"
#include "mir/pitchShift_algorithm.h"
#include "mir/timeStretch_algorithm.h"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            exit(1);                                               \
        }                                                          \
    } while (0)

static int vocoders, fits, resamples, lastBatch;
static volatile float sink;

int afxk_phase_vocoder(const AfxPhaseVocoderArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->re || !a->im || !a->mag || !a->ang || !a->outRe || !a->outIm) return AFX_ERR_ARG;
    if (a->radix2Exp < 1 || a->radix2Exp > 14 || a->hop <= 0 || a->batch <= 0 || a->batch > 65535 || a->T1 <= 0) return AFX_ERR_ARG;
    const int N = 1 << a->radix2Exp, F = N / 2 + 1;
    if (a->T2 <= 0 || a->T2 != afx_pv_frames(a->T1, a->rate) || a->inPitch < F) return AFX_ERR_ARG;
    vocoders++;
    lastBatch = a->batch;
    for (long long row = 0; row < (long long)a->batch * a->T1; row++) /* polar (in place when mag == re) */
        for (int j = 0; j < F; j++) {
            const float re = a->re[row * a->inPitch + j], im = a->im[row * a->inPitch + j];
            a->mag[row * F + j] = re + im;
            a->ang[row * F + j] = re - im;
        }
    for (int b = 0; b < a->batch; b++)
        for (int i = 0; i < a->T2; i++) {
            float alpha;
            const int k = afx_pv_time(i, a->rate, &alpha);
            CHECK(k >= 0 && k <= a->T1 && alpha >= 0.f && alpha < 1.f);
            float *re = a->outRe + ((long long)b * a->T2 + i) * N, *im = a->outIm + ((long long)b * a->T2 + i) * N;
            for (int j = 0; j < F; j++) {
                float v = 0;
                if (k < a->T1) v += a->mag[((long long)b * a->T1 + k) * F + j] + a->ang[((long long)b * a->T1 + k) * F + j];
                if (k + 1 < a->T1) v += a->mag[((long long)b * a->T1 + k + 1) * F + j] + a->ang[((long long)b * a->T1 + k + 1) * F + j];
                re[j] = v;
                im[j] = alpha;
                if (j > 0 && j < N - j) {
                    re[N - j] = v;
                    im[N - j] = -alpha;
                }
            }
        }
    return AFX_OK;
}

int afxk_rows_fit(const float *src, long long srcStride, int srcLength, float *dst, long long dstStride, int length, int batch,
                  void *stream) {
    (void)stream;
    if (!src || !dst || srcLength < 0 || length <= 0 || batch <= 0) return AFX_ERR_ARG;
    fits++;
    for (int b = 0; b < batch; b++)
        for (int i = 0; i < length; i++) dst[b * dstStride + i] = i < srcLength ? src[b * srcStride + i] : 0.f;
    return AFX_OK;
}

int afxk_resample(const AfxResampleArgs *a, void *stream) {
    (void)stream;
    if (!a || !a->x || !a->out || !a->table || a->batch <= 0 || a->sourceLength <= 0 || a->targetLength <= 0) return AFX_ERR_ARG;
    resamples++;
    float s = 0;
    for (int k = 0; k <= a->interpLength; k++) s += a->table[k];
    for (int b = 0; b < a->batch; b++) {
        for (int i = 0; i < a->sourceLength; i++) s += a->x[b * a->clipStride + i];
        for (int i = 0; i < a->targetLength; i++) a->out[b * a->outStride + i] = 0.5f;
    }
    sink = s;
    return AFX_OK;
}

static float *signal(int n) {
    float *x = (float *)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
    CHECK(x);
    unsigned v = 12345u;
    for (int i = 0; i < n; i++) {
        v = v * 1664525u + 1013904223u;
        x[i] = (float)(v >> 8) / 16777216.f - 0.5f;
    }
    return x;
}

/* the host-pointer call into an exactly sized destination (the inverse transform's samples, a guard behind them) */
static void stretch(TimeStretchObj o, float *x, int n, int exp, int hop, float rate) {
    AfxTimeStretchPlan p;
    CHECK(afx_timestretch_plan(exp, hop, rate, n, 1, 0, &p, NULL, NULL) == 0);
    CHECK(timeStretchObj_calDataCapacity(o, rate, n) == p.capacity && p.istftLength <= p.capacity);
    float *y = (float *)malloc(sizeof(float) * ((size_t)p.istftLength + 1));
    CHECK(y);
    for (int i = 0; i <= p.istftLength; i++) y[i] = 9.f;
    CHECK(timeStretchObj_timeStretch(o, rate, x, n, y) == p.returnLength);
    CHECK(y[p.istftLength] == 9.f && y[0] != 9.f && y[p.istftLength - 1] != 9.f);
    free(y);
    printf("stretch 2^%d / %d, %d samples at %g: %d -> %d frames, %d samples, %lld scratch bytes\n", exp, hop, n, (double)rate, p.T1, p.T2,
           p.istftLength, p.scratchBytes);
}

int main(void) {
    float *x = signal(400000);
    const int errors0 = afxdev_error_count();

    /* construction and free: defaults, every argument, refusals */
    TimeStretchObj ts = NULL;
    PitchShiftObj ps = NULL;
    int exp = 15, hop = 257, small = 8;
    WindowType hamm = Window_Hamm;
    CHECK(timeStretchObj_new(NULL, NULL, NULL, NULL) == AFX_ERR_ARG && pitchShiftObj_new(NULL, NULL, NULL, NULL) == AFX_ERR_ARG);
    CHECK(timeStretchObj_new(&ts, &exp, NULL, NULL) == AFX_ERR_UNSUPPORTED && ts == NULL);
    CHECK(timeStretchObj_new(&ts, &small, &hop, NULL) == AFX_ERR_UNSUPPORTED && ts == NULL);
    CHECK(pitchShiftObj_new(&ps, &exp, NULL, NULL) == AFX_ERR_UNSUPPORTED && ps == NULL);
    CHECK(pitchShiftObj_new(&ps, &small, &hop, &hamm) == AFX_ERR_UNSUPPORTED && ps == NULL);
    CHECK(timeStretchObj_new(&ts, NULL, NULL, NULL) == 0 && ts); /* 2^12, hop 1024, Hann */
    stretch(ts, x, 20000, 12, 1024, 0.7f);
    timeStretchObj_free(ts);
    exp = 31; /* outside 1 ... 30: the default again */
    hop = -3;
    CHECK(timeStretchObj_new(&ts, &exp, &hop, &hamm) == 0 && ts);
    stretch(ts, x, 20000, 12, 1024, 1.5f);
    timeStretchObj_free(ts);
    timeStretchObj_free(NULL);
    pitchShiftObj__free(NULL);
    printf("timestretch construction: defaults, refusals\n");

    /* the scratch sizes of long and short calls on one object (grow-only, never trusted), odd sizes */
    exp = 8;
    hop = 100;
    CHECK(timeStretchObj_new(&ts, &exp, &hop, NULL) == 0 && ts);
    stretch(ts, x, 3000, 8, 100, 0.8f);
    stretch(ts, x, 300001, 8, 100, 0.5f);
    stretch(ts, x, 256, 8, 100, 2.f); /* one frame in, one out */
    stretch(ts, x, 3001, 8, 100, 1.7f);
    stretch(ts, x, 400000, 8, 100, 1.99f);
    hop = 256; /* no overlap */
    TimeStretchObj flat = NULL;
    CHECK(timeStretchObj_new(&flat, &exp, &hop, &hamm) == 0 && flat);
    stretch(flat, x, 3000, 8, 256, 1.3f);
    timeStretchObj_free(flat);

    /* a strided batch in chunks under a small scratch limit: exactly the returned length is written per row */
    {
        const int n = 3000, clips = 7, stride = n + 13;
        AfxTimeStretchPlan p;
        CHECK(afx_timestretch_plan(8, 100, 0.8f, n, clips, 0, &p, NULL, NULL) == 0 && p.clipsPerChunk == clips);
        const int m = p.returnLength, pitch = m + 5;
        float *in = (float *)malloc(sizeof(float) * ((size_t)(clips - 1) * stride + n)); /* the last clip ends the buffer */
        float *out = (float *)malloc(sizeof(float) * ((size_t)(clips - 1) * pitch + m));
        CHECK(in && out);
        for (int b = 0; b < clips; b++) memcpy(in + (size_t)b * stride, x + 100 * b, sizeof(float) * n);
        vocoders = fits = 0;
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, stride, out, pitch, NULL) == m);
        CHECK(vocoders == 1 && fits == 1 && lastBatch == clips);
        timeStretchObj_setScratchLimit(ts, 3 * p.scratchBytes + 17);
        CHECK(afx_timestretch_plan(8, 100, 0.8f, n, clips, 3 * p.scratchBytes + 17, &p, NULL, NULL) == 0 && p.clipsPerChunk == 3);
        vocoders = fits = 0;
        for (size_t i = 0; i < (size_t)(clips - 1) * pitch + m; i++) out[i] = 9.f;
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, stride, out, pitch, NULL) == m);
        CHECK(vocoders == 3 && fits == 3 && lastBatch == 1); /* 3 + 3 + 1 clips */
        for (int b = 0; b < clips - 1; b++)
            for (int i = m; i < pitch; i++) CHECK(out[(size_t)b * pitch + i] == 9.f);
        timeStretchObj_setScratchLimit(ts, 1); /* below one clip: one clip per chunk */
        vocoders = 0;
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, stride, out, pitch, NULL) == m && vocoders == clips);
        timeStretchObj_setScratchLimit(ts, 0); /* the default again */
        vocoders = 0;
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, stride, out, pitch, NULL) == m && vocoders == 1);
        /* refusals of the device call: nothing is launched */
        vocoders = fits = 0;
        CHECK(timeStretchObj_timeStretchBatchDevice(NULL, 0.8f, in, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, NULL, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, stride, NULL, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, 0, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, 0, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, n - 1, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, n, stride, out, m - 1, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.f, in, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, -1.f, in, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, NAN, in, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, INFINITY, in, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 1e-6f, in, clips, n, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretchBatchDevice(ts, 0.8f, in, clips, 255, stride, out, pitch, NULL) == AFX_ERR_ARG);
        CHECK(vocoders == 0 && fits == 0);
        free(in);
        free(out);
        printf("timestretch batch: %d strided clips in chunks of 7, 3 and 1, refusals\n", clips);
    }

    /* refusals of the host-pointer call: recorded, nothing written */
    {
        float y[4] = {9.f, 9.f, 9.f, 9.f};
        int before = afxdev_error_count();
        CHECK(timeStretchObj_timeStretch(NULL, 0.8f, x, 3000, y) == AFX_ERR_ARG && afxdev_error_count() > before);
        const float rates[] = {0.f, -2.f, NAN, INFINITY};
        for (int i = 0; i < 4; i++) {
            before = afxdev_error_count();
            CHECK(timeStretchObj_timeStretch(ts, rates[i], x, 3000, y) == AFX_ERR_ARG && afxdev_error_count() > before);
            CHECK(timeStretchObj_calDataCapacity(ts, rates[i], 3000) == 0);
        }
        before = afxdev_error_count();
        CHECK(timeStretchObj_timeStretch(ts, 0.8f, NULL, 3000, y) == AFX_ERR_ARG && timeStretchObj_timeStretch(ts, 0.8f, x, 3000, NULL) == AFX_ERR_ARG);
        CHECK(timeStretchObj_timeStretch(ts, 0.8f, x, 255, y) == AFX_ERR_ARG && timeStretchObj_timeStretch(ts, 0.8f, x, 0, y) == AFX_ERR_ARG);
        CHECK(afxdev_error_count() >= before + 4 && y[0] == 9.f && y[3] == 9.f);
        CHECK(timeStretchObj_calDataCapacity(NULL, 0.8f, 3000) == 0);
        printf("timestretch refusals: recorded, nothing written\n");
    }
    timeStretchObj_free(ts);

    /* the vocoder alone: half spectra and full spectra, its own scratch, refusals */
    {
        const int T1 = 9, N = 64, F = 33, T2 = afx_pv_frames(T1, 0.7f);
        float *re = signal(3 * T1 * N), *out = (float *)malloc(sizeof(float) * 2 * 3 * (size_t)T2 * N);
        CHECK(out && T2 == 13);
        vocoders = 0;
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 6, F, 16, 0.7f, out, out + 3 * T2 * N, NULL) == 0);
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 6, N, 16, 0.7f, out, out + 3 * T2 * N, NULL) == 0 && vocoders == 2);
        CHECK(afx_phase_vocoder_device(NULL, re, 3, T1, 6, F, 16, 0.7f, out, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 6, F, 16, 0.7f, NULL, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 0, T1, 6, F, 16, 0.7f, out, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 3, 0, 6, F, 16, 0.7f, out, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 15, F, 16, 0.7f, out, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 6, F - 1, 16, 0.7f, out, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 6, F, 0, 0.7f, out, out, NULL) == AFX_ERR_ARG);
        CHECK(afx_phase_vocoder_device(re, re, 3, T1, 6, F, 16, 0.f, out, out, NULL) == AFX_ERR_ARG && vocoders == 2);
        free(re);
        free(out);
        printf("timestretch vocoder alone: pitches %d and %d, refusals\n", F, N);
    }

    /* pitch shift: the length rule, chunks of its own scratch, refusals */
    exp = 8;
    hop = 64;
    CHECK(pitchShiftObj_new(&ps, &exp, &hop, NULL) == 0 && ps);
    {
        const int semis[] = {-12, -5, 0, 3, 12};
        for (int n = 3000; n <= 3001; n++)
            for (int s = 0; s < 5; s++) {
                float *y = (float *)malloc(sizeof(float) * (size_t)n); /* exactly the input's length: one more sample is a report */
                CHECK(y);
                for (int i = 0; i < n; i++) y[i] = 9.f;
                const int before = afxdev_error_count();
                pitchShiftObj_pitchShift(ps, 32000, semis[s], x, n, y);
                CHECK(afxdev_error_count() == before && y[0] == 0.5f);
                int written = 0;
                while (written < n && y[written] == 0.5f) written++;
                const float rate = powf(2, (float)(-semis[s] * 1.0 / 12));
                const float target = floorf(roundf((float)n / rate) * rate);
                CHECK(written == (target < (float)n ? (int)target : n));
                for (int i = written; i < n; i++) CHECK(y[i] == 9.f);
                printf("pitchshift %d samples, %+d semitones: %d written (resampled length %d)\n", n, semis[s], written, (int)target);
                free(y);
            }
        CHECK((int)floorf(roundf(3001.f / 2.f) * 2.f) == 3002 && (int)floorf(roundf(3000.f / powf(2, (float)(5.0 / 12))) * powf(2, (float)(5.0 / 12))) == 2999);
    }
    {
        const int n = 3000, clips = 5, stride = n + 3;
        float *in = (float *)malloc(sizeof(float) * ((size_t)(clips - 1) * stride + n)), *out = (float *)malloc(sizeof(float) * ((size_t)(clips - 1) * stride + n));
        CHECK(in && out);
        for (int b = 0; b < clips; b++) memcpy(in + (size_t)b * stride, x + 50 * b, sizeof(float) * n);
        vocoders = resamples = 0;
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, clips, n, stride, out, stride, NULL) == n && vocoders == 1 && resamples == 1);
        AfxTimeStretchPlan p;
        CHECK(afx_timestretch_plan(8, 64, powf(2, (float)(-3 * 1.0 / 12)), n, clips, 0, &p, NULL, NULL) == 0 && p.returnLength == 3568);
        /* two clips of this object's rows (3568 stretched + 3000 resampled samples); the time stretch takes one clip a chunk */
        pitchShiftObj_setScratchLimit(ps, 2 * 4 * (3568 + 3000) + 64);
        vocoders = resamples = 0;
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, clips, n, stride, out, stride, NULL) == n && vocoders == 5 && resamples == 3);
        pitchShiftObj_setScratchLimit(ps, 0);
        vocoders = resamples = 0;
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, -5, in, clips, n, stride, out, stride, NULL) == n - 1 && vocoders == 1);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 13, in, clips, n, stride, out, stride, NULL) == 0);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, -13, in, clips, n, stride, out, stride, NULL) == 0);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(NULL, 3, in, clips, n, stride, out, stride, NULL) == AFX_ERR_ARG);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, NULL, clips, n, stride, out, stride, NULL) == AFX_ERR_ARG);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, clips, n, stride, NULL, stride, NULL) == AFX_ERR_ARG);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, 0, n, stride, out, stride, NULL) == AFX_ERR_ARG);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, clips, n, n - 1, out, stride, NULL) == AFX_ERR_ARG);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, clips, n, stride, out, n - 1, NULL) == AFX_ERR_ARG);
        CHECK(pitchShiftObj_pitchShiftBatchDevice(ps, 3, in, clips, 255, stride, out, stride, NULL) == AFX_ERR_ARG);
        CHECK(vocoders == 1);
        float y[2] = {9.f, 9.f};
        int before = afxdev_error_count();
        pitchShiftObj_pitchShift(ps, 32000, 13, x, n, y);
        pitchShiftObj_pitchShift(ps, 32000, -13, x, n, y);
        CHECK(afxdev_error_count() == before);
        pitchShiftObj_pitchShift(NULL, 32000, 3, x, n, y);
        pitchShiftObj_pitchShift(ps, 32000, 3, NULL, n, y);
        pitchShiftObj_pitchShift(ps, 32000, 3, x, n, NULL);
        pitchShiftObj_pitchShift(ps, 32000, 3, x, 255, y);
        pitchShiftObj_pitchShift(ps, 32000, 3, x, 0, y);
        CHECK(afxdev_error_count() >= before + 5 && y[0] == 9.f && y[1] == 9.f);
        free(in);
        free(out);
        printf("pitchshift batch: %d strided clips in chunks, refusals\n", clips);
    }
    pitchShiftObj__free(ps);

    /* the plan function */
    {
        AfxTimeStretchPlan p;
        int k[64];
        float al[64];
        CHECK(afx_timestretch_plan(8, 64, 0.8f, 3000, 1, 0, NULL, NULL, NULL) == AFX_ERR_ARG);
        CHECK(afx_timestretch_plan(15, 64, 0.8f, 3000, 1, 0, &p, NULL, NULL) == AFX_ERR_UNSUPPORTED);
        CHECK(afx_timestretch_plan(8, 64, 0.8f, 3000, 1, 0, &p, k, al) == 0 && p.T1 == 43 && p.T2 == 54 && p.istftLength == 53 * 64 + 256);
        CHECK(k[0] == 0 && al[0] == 0.f && k[53] == 42 && p.returnLength == 3750 && p.capacity == 3750 + 256);
        CHECK(afx_timestretch_plan(8, 64, 0.8f, 3000, 1, 0, &p, k, NULL) == 0 && afx_timestretch_plan(8, 64, 0.8f, 3000, 1, 0, &p, NULL, al) == 0);
        CHECK(afx_timestretch_plan(8, 64, 0.8f, 255, 1, 0, &p, k, al) == AFX_ERR_ARG && p.T1 == 0);
    }
    CHECK(afxdev_error_count() > errors0);
    free(x);
    printf("OK\n");
    return 0;
}
