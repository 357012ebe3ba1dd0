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
    free(f->cur);
    memset(f, 0, sizeof(*f));
}

int afx_frametail_frames(const AfxFrameTail *f, int dataLength) {
    long long total = dataLength;
    if (f->isContinue) total += f->tailLength;
    if (total < f->frameLength) return 0;
    return (int)((total - f->frameLength) / f->hop + 1);
}

int afx_frametail_push(AfxFrameTail *f, const float *data, int dataLength, int *curLength) {
    const int N = f->frameLength, hop = f->hop;
    const int carried = f->isContinue ? f->tailLength : 0;
    const long long total = (long long)carried + dataLength;
    *curLength = 0;
    if (total < N) { /* no frame: the call extends the tail or works off the skip */
        if (!f->isContinue) {
            f->tailLength = 0;
            return 0;
        }
        if (total > 0) {
            if (carried >= 0) memcpy(f->tail + carried, data, sizeof(float) * (size_t)dataLength);
            else memcpy(f->tail, data - carried, sizeof(float) * (size_t)total);
        }
        f->tailLength = (int)total;
        return 0;
    }
    const long long frames = (total - N) / hop + 1;
    const long long left = (total - N) % hop + (N - hop); /* < N; negative when the next frame starts beyond this call */
    if (frames > 0x7fffffffLL || total > 0x7fffffffLL) return AFX_ERR_ARG;
    if ((size_t)total > f->curCap) {
        float *p = (float *)malloc(sizeof(float) * (size_t)total);
        if (!p) return AFX_ERR_NOMEM;
        free(f->cur);
        f->cur = p;
        f->curCap = (size_t)total;
    }
    if (carried < 0) {
        memcpy(f->cur, data - carried, sizeof(float) * (size_t)total);
    } else {
        if (carried > 0) memcpy(f->cur, f->tail, sizeof(float) * (size_t)carried);
        memcpy(f->cur + carried, data, sizeof(float) * (size_t)dataLength);
    }
    f->tailLength = 0;
    if (f->isContinue) {
        if (left > 0) memcpy(f->tail, f->cur + (total - left), sizeof(float) * (size_t)left);
        f->tailLength = (int)left;
    }
    *curLength = (int)total;
    return (int)frames;
}
