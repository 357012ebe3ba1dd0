/* afx_frametail.c -- see afx_frametail.h */
#include "afx_frametail.h"

#include <stdlib.h>
#include <string.h>

#include "afx_device.h"

int afx_frametail_init(AfxFrameTail *f, int frameLength, int hop, int isContinue) {
    memset(f, 0, sizeof(*f));
    f->frameLength = frameLength;
    f->hop = hop;
    f->isContinue = isContinue != 0;
    f->tail = (float *)calloc((size_t)frameLength, sizeof(float));
    return f->tail ? AFX_OK : AFX_ERR_NOMEM;
}

void afx_frametail_free(AfxFrameTail *f) {
    free(f->tail);
    memset(f, 0, sizeof(*f));
}

int afx_frametail_frames(const AfxFrameTail *f, int dataLength) {
    return afx_frames((long long)dataLength + (f->isContinue ? f->tailLength : 0), f->frameLength, f->hop);
}

int afx_frametail_take(const AfxFrameTail *f, int dataLength, AfxFrameTake *t) {
    const int carried = f->isContinue ? f->tailLength : 0;
    const long long total = (long long)carried + dataLength;
    memset(t, 0, sizeof(*t));
    if (total < f->frameLength) return 0; /* no frame: the call extends the tail or works off the skip */
    if (total > 0x7fffffffLL) return AFX_ERR_ARG; /* (frames <= total) */
    t->frames = afx_frames(total, f->frameLength, f->hop);
    if (carried < 0) t->skip = -carried;
    else t->head = carried;
    t->total = (int)total;
    return t->frames;
}

void afx_frametail_keep(AfxFrameTail *f, const float *data, int dataLength) {
    const int N = f->frameLength, hop = f->hop, old = f->tailLength;
    if (!f->isContinue) {
        f->tailLength = 0;
        return;
    }
    const long long total = (long long)old + dataLength;
    /* without a frame everything stays; else what the last frame's hop leaves: < N, negative when the next frame starts
     * beyond this call */
    const long long left = total < N ? total : (total - N) % hop + (N - hop);
    if (left > 0) { /* the last `left` samples of [tail | data] */
        if (left <= dataLength) {
            memcpy(f->tail, data + (dataLength - left), sizeof(float) * (size_t)left);
        } else {
            const size_t fromOld = (size_t)(left - dataLength); /* <= old */
            memmove(f->tail, f->tail + ((size_t)old - fromOld), sizeof(float) * fromOld);
            memcpy(f->tail + fromOld, data, sizeof(float) * (size_t)dataLength);
        }
    }
    f->tailLength = (int)left;
}

int afx_frametail_upload(const AfxFrameTail *f, const AfxFrameTake *t, const float *data, float **dX, size_t *capX,
                         void *stream) {
    const size_t head = (size_t)t->head, fresh = (size_t)t->total - head;
    int st = afxdev_reserve((void **)dX, capX, sizeof(float) * (size_t)t->total);
    if (st == AFX_OK && head > 0) st = afxdev_h2d(*dX, f->tail, sizeof(float) * head, stream);
    if (st == AFX_OK && fresh > 0) st = afxdev_h2d(*dX + head, data + t->skip, sizeof(float) * fresh, stream);
    return st;
}
