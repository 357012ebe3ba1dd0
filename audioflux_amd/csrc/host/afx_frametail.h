/* afx_frametail.h -- framing of a signal that arrives in pieces: frames of frameLength samples every hop samples, the
 * samples a call leaves unused kept for the next one.  With hop > frameLength the "tail" is negative: that many samples of
 * the next call are skipped.  Host bookkeeping only; the semantics are the reference's (src/mir/_pitch_yin.c:791-938). */
#ifndef AFX_FRAMETAIL_H
#define AFX_FRAMETAIL_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int frameLength, hop, isContinue;
    float *tail;    /* frameLength floats */
    int tailLength; /* < frameLength; negative: samples still to skip */
    float *cur;     /* grow-only: the signal the frames of the last call were cut from */
    size_t curCap;
} AfxFrameTail;

int afx_frametail_init(AfxFrameTail *f, int frameLength, int hop, int isContinue);
void afx_frametail_free(AfxFrameTail *f);
/* frames a call with dataLength samples would yield (the tail counts when continuing) */
int afx_frametail_frames(const AfxFrameTail *f, int dataLength);
/* one call: returns the frames (0: the call only changed the tail), < 0 on allocation failure.  With frames, f->cur holds
 * the *curLength samples they are cut from: frame i starts at i * hop. */
int afx_frametail_push(AfxFrameTail *f, const float *data, int dataLength, int *curLength);

#ifdef __cplusplus
}
#endif
#endif
