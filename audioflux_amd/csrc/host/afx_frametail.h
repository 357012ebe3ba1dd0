/* afx_frametail.h -- framing of a signal that arrives in pieces: frames of frameLength samples every hop samples over
 * [kept tail | new data], the samples a call leaves unused kept for the next one.  With hop > frameLength the "tail" is
 * negative: that many samples of the next call are skipped.  Host bookkeeping only, and the only implementation: the
 * STFT, spectrogram, CQT and YIN objects carry one.  The rule is the same in every streaming object of the reference
 * (src/stft_algorithm.c:548-557, 826-850; src/cqt_algorithm.c:309-327, 345-456; src/mir/_pitch_yin.c:791-938; the
 * spectrogram object through the STFT object it owns).  The STFT object's PADDED framing is another rule and stays in
 * afx_stft.c. */
#ifndef AFX_FRAMETAIL_H
#define AFX_FRAMETAIL_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* whole frames in n samples */
static inline int afx_frames(long long n, int frameLength, int hop) {
    return n < frameLength ? 0 : (int)((n - frameLength) / hop + 1);
}

typedef struct {
    int frameLength, hop, isContinue;
    float *tail;    /* frameLength floats */
    int tailLength; /* < frameLength; negative: samples still to skip */
} AfxFrameTail;

/* what one call frames: the signal [tail[0 .. head) | data[skip .. dataLength)] of `total` samples, frame i at i * hop */
typedef struct {
    int frames, head, skip, total;
} AfxFrameTake;

int afx_frametail_init(AfxFrameTail *f, int frameLength, int hop, int isContinue);
void afx_frametail_free(AfxFrameTail *f);
/* frames a call with dataLength samples would yield (the tail counts when continuing) */
int afx_frametail_frames(const AfxFrameTail *f, int dataLength);
/* (library-internal: not part of the exported symbols) */
#define AFX_INTERNAL __attribute__((visibility("hidden")))
/* computes only: the frames of a call with dataLength samples (0: the call only changes the tail) and, with frames, where
 * their signal comes from; AFX_ERR_ARG when it would exceed 2^31 - 1 samples */
AFX_INTERNAL int afx_frametail_take(const AfxFrameTail *f, int dataLength, AfxFrameTake *t);
/* ends the call: the samples of [tail | data] behind its last frame (all of them when it had none) become the tail; an
 * object that does not continue keeps nothing */
AFX_INTERNAL void afx_frametail_keep(AfxFrameTail *f, const float *data, int dataLength);
/* the signal of a take on the device: *dX (grow-only, afxdev_reserve) receives its two pieces on `stream`.  Before keep. */
AFX_INTERNAL int afx_frametail_upload(const AfxFrameTail *f, const AfxFrameTake *t, const float *data, float **dX,
                                      size_t *capX, void *stream);

#ifdef __cplusplus
}
#endif
#endif
