/* afx_objkit.h -- the call plumbing every host object shares, each rule written once (library-internal; the framing of
 * streamed signals is afx_frametail.h).  Plain C over the afxdev_* calls of afx_device.h. */
#ifndef AFX_OBJKIT_H
#define AFX_OBJKIT_H

#include <string.h>

#include "afx_device.h"

/* A void entry point of object `o` (any struct with a `status` field) ends in failure `st`. */
#define AFX_FAIL(o, st, who)                  \
    do {                                      \
        (o)->status = (st);                   \
        afxdev_report_failure((who), (st));   \
    } while (0)

/* Grow-only device scratch belongs to its object, not to a stream: a call that is about to use it on another stream than
 * the previous one drains that stream first. */
typedef struct {
    void *stream; /* of the previous call that used the scratch */
    int used;
} AfxScratchStream;

static inline int afx_scratch_wait(const AfxScratchStream *s, void *stream) {
    return s->used && s->stream != stream ? afxdev_stream_sync(s->stream) : AFX_OK;
}
static inline void afx_scratch_mark(AfxScratchStream *s, void *stream) {
    s->stream = stream;
    s->used = 1;
}
/* wait, then mark: the guard of an entry point that returns on failure */
static inline int afx_scratch_enter(AfxScratchStream *s, void *stream) {
    const int st = afx_scratch_wait(s, stream);
    if (st == AFX_OK) afx_scratch_mark(s, stream);
    return st;
}
/* before the scratch is freed or replaced: whichever stream used it last may still run our kernels */
static inline void afx_scratch_drain(const AfxScratchStream *s) {
    if (s->used && s->stream) afxdev_stream_sync(s->stream);
}

/* Arguments of the framed transform (afxk_stft / afxk_temporal), zeroed, then what every caller sets: `batch` clips of
 * dataLength valid samples every clipStride at x, timeLength frames each, bins binLo ... binLo + binCount - 1 stored as
 * `mode`.  Padding, band plan, fullSpectrum, normValue, outPitch and the temporal planes follow at the call site. */
static inline void afx_stft_args(AfxStftArgs *a, const float *x, long long clipStride, int batch, int dataLength, int timeLength,
                                 int radix2Exp, int hop, const float *window, const float *twiddle, int mode, int binLo,
                                 int binCount, float *outRe, float *outIm) {
    memset(a, 0, sizeof(*a));
    a->x = x;
    a->clipStride = clipStride;
    a->batch = batch;
    a->dataLength = dataLength;
    a->timeLength = timeLength;
    a->radix2Exp = radix2Exp;
    a->hop = hop;
    a->window = window;
    a->twiddle = twiddle;
    a->mode = mode;
    a->binLo = binLo;
    a->binCount = binCount;
    a->outRe = outRe;
    a->outIm = outIm;
}

#endif /* AFX_OBJKIT_H */
