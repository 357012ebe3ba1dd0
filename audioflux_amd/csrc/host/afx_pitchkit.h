/* afx_pitchkit.h -- what the pitch tracker objects share on the host (afx_pitch_yin.c, afx_pitch_hs.c, afx_pitch_pef.c), each
 * rule written once (library-internal, next to afx_objkit.h and afx_frametail.h): the head of the object, its init and
 * release, the guard of the batched device calls and the frame of the host-pointer call around a tracker's own launch.
 * A tracker supplies its plan, its tables, the fill of its Afx*Args and its kernel. */
#ifndef AFX_PITCHKIT_H
#define AFX_PITCHKIT_H

#include <stddef.h>

#include "afx_device.h"
#include "afx_frametail.h"
#include "afx_objkit.h"

/* the head every pitch object embeds as `head`; AFX_ENTER and AFX_FAIL apply to it */
typedef struct {
    int radix2Exp, fftLength, slideLength, samplate;
    int isDebug;
    AfxFrameTail tail; /* isContinue and the samples carried between host-pointer calls */
    int timeLength;    /* frames of the last host-pointer call */
    void *stream;
    float *dX, *dOut; /* grow-only device buffers of the host-pointer call: the samples, the result rows */
    size_t capX, capOut;
    int status; /* last failure of a void entry point */
} AfxPitchHead;
/* of a handle that may be NULL */
#define AFX_PITCH_HEAD(o) ((o) ? &(o)->head : NULL)

/* of a calloc'ed object: the sizes, the tail, the stream */
static inline int afx_pitch_head_init(AfxPitchHead *h, int radix2Exp, int slideLength, int samplate, int isContinue) {
    h->radix2Exp = radix2Exp;
    h->fftLength = 1 << radix2Exp;
    h->slideLength = slideLength;
    h->samplate = samplate;
    int st = afx_frametail_init(&h->tail, h->fftLength, slideLength, isContinue);
    if (st == AFX_OK) st = afxdev_stream_create(&h->stream);
    return st;
}

/* *_calTimeLength: frames a host-pointer call with dataLength samples would yield */
static inline int afx_pitch_frames(const AfxPitchHead *h, int dataLength) { return h ? afx_frametail_frames(&h->tail, dataLength) : 0; }

/* release in two steps: the stream drained FIRST, then the tracker's own frees, then the head's buffers, stream and tail */
static inline void afx_pitch_head_sync(AfxPitchHead *h) {
    if (h->stream) afxdev_stream_sync(h->stream);
}
static inline void afx_pitch_head_release(AfxPitchHead *h) {
    afxdev_free(h->dX);
    afxdev_free(h->dOut);
    if (h->stream) afxdev_stream_destroy(h->stream);
    afx_frametail_free(&h->tail);
}

/* a table of the constructor: allocated, then uploaded on `stream`; `st` chains the calls */
static inline int afx_pitch_table(int st, float **dTable, const void *table, size_t bytes, void *stream) {
    if (st == AFX_OK) st = afxdev_malloc((void **)dTable, bytes);
    if (st == AFX_OK) st = afxdev_h2d(*dTable, table, bytes, stream);
    return st;
}

/* Guard of every *BatchDevice call of object `name`: 1 = run *T frames per clip, 0 = nothing to do, < 0 = refusal (an
 * isContinue object takes no batch: its tail belongs to one signal). */
static inline int afx_pitch_batch_enter(const AfxPitchHead *h, const char *name, const float *dData, int batch, int dataLength,
                                        long long clipStride, const void *out, void *hipStream, int *T) {
    if (!h || !dData || !out || batch <= 0 || dataLength <= 0 || clipStride < dataLength) return AFX_ERR_ARG;
    if (h->tail.isContinue) {
        afxdev_set_error("%s: a batched call on an object that carries one signal's tail (isContinue = 1)", name);
        return AFX_ERR_UNSUPPORTED;
    }
    const int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    *T = afx_frames(dataLength, h->fftLength, h->slideLength);
    return *T > 0;
}

/* The host-pointer call, opening half: frames the call has to compute, their signal in *t.  0: the call is over -- empty
 * input (as in the reference), no whole frame yet (the samples are kept) or a failure (reported). */
static inline int afx_pitch_call_begin(AfxPitchHead *h, const float *dataArr, int dataLength, AfxFrameTake *t, const char *who) {
    if (!dataArr || dataLength <= 0) return 0;
    const int T = afx_frametail_take(&h->tail, dataLength, t);
    h->timeLength = T > 0 ? T : 0;
    if (T < 0) {
        AFX_FAIL(h, T, who);
        return 0;
    }
    if (T == 0) afx_frametail_keep(&h->tail, dataArr, dataLength);
    return T;
}

/* closing half: the samples are taken in whatever became of the frames (`st`, which is returned) */
static inline int afx_pitch_call_end(AfxPitchHead *h, const float *dataArr, int dataLength, int st, const char *who) {
    afx_frametail_keep(&h->tail, dataArr, dataLength);
    if (st != AFX_OK) {
        h->timeLength = 0;
        AFX_FAIL(h, st, who);
    }
    return st;
}

/* one launch of tracker `ctx` over `batch` clips: fre / value rows every outStride and / or the curve */
typedef int (*AfxPitchRun)(void *ctx, const float *dData, int batch, int dataLength, long long clipStride, int T, float *dFre,
                           float *dValue, long long outStride, float *dCurve, void *stream);

/* the whole host-pointer call of a tracker that returns a frequency per frame: the batch of one through the head's staging
 * buffers */
static inline void afx_pitch_call(AfxPitchHead *h, const float *dataArr, int dataLength, float *freArr, AfxPitchRun run, void *ctx,
                                  const char *who) {
    if (!h) {
        afxdev_set_error("%s: NULL object", who);
        afxdev_report_failure(who, AFX_ERR_ARG);
        return;
    }
    AFX_ENTER(h);
    AfxFrameTake t;
    const int T = afx_pitch_call_begin(h, dataArr, dataLength, &t, who);
    if (T <= 0) return;
    const int n = t.total;
    const size_t rowB = sizeof(float) * (size_t)T;
    int st = freArr ? AFX_OK : AFX_ERR_ARG;
    if (st == AFX_OK) st = afx_frametail_upload(&h->tail, &t, dataArr, &h->dX, &h->capX, h->stream);
    if (st == AFX_OK) st = afxdev_reserve((void **)&h->dOut, &h->capOut, rowB);
    if (st == AFX_OK) st = run(ctx, h->dX, 1, n, n, T, h->dOut, NULL, T, NULL, h->stream);
    if (st == AFX_OK) st = afxdev_d2h(freArr, h->dOut, rowB, h->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(h->stream);
    afx_pitch_call_end(h, dataArr, dataLength, st, who);
}

#endif /* AFX_PITCHKIT_H */
