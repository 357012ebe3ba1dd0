/* afx_hpss.c -- the harmonic / percussive separation object (C host side) behind include/mir/hpss_algorithm.h and
 * the device-pointer calls of include/afx_batch.h.
 *
 * Mirrors the parameter semantics of the reference object (src/mir/hpss_algorithm.c:40-358): Hamm by default, the hop
 * fixed at fftLength/4 whatever slideLength says, odd orders with the defaults 21 / 31, outputs accumulated onto the
 * caller's arrays.  Execution: the owned STFT object's forward kernel stores the half spectrum of a chunk of whole
 * clips, k_hpss_tile (afx_hpss.hip) turns it into the two masked full spectra in one launch, the STFT object's inverse
 * adds each requested output onto the caller's buffer.  Everything is enqueued on one stream; the scratch of a chunk is
 * bounded by a constant and reused.  There is no CPU compute path.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/hpss_algorithm.h"
#include "stft_algorithm.h"

#define HPSS_MIN_EXP 2 /* hop = fftLength/4 >= 1 */
#define HPSS_MAX_EXP 14

/* scratch of one chunk of clips.  AFX_HPSS_CHUNK_MB overrides (tools/bench_hpss.py --chunk-mb, the chunked == unchunked tests) */
static size_t chunk_bytes(void) {
    const char *s = getenv("AFX_HPSS_CHUNK_MB");
    size_t mb = 1024;
    if (s && atoi(s) > 0) mb = (size_t)atoi(s);
    return mb << 20;
}

/* defaults and refusals of hpssObj_new that need no device (hpss_algorithm.c:48-81) */
static int hpss_params(int radix2Exp, const WindowType *windowType, const int *hOrder, const int *pOrder, WindowType *wt,
                       int *h, int *p) {
    *wt = windowType ? *windowType : Window_Hamm;
    *h = (hOrder && *hOrder > 0 && (*hOrder & 1)) ? *hOrder : 21;
    *p = (pOrder && *pOrder > 0 && (*pOrder & 1)) ? *pOrder : 31;
    if (radix2Exp < HPSS_MIN_EXP || radix2Exp > HPSS_MAX_EXP) return -100;
    const int fast = AFX_MEDIAN_FAST_ORDER;
    if (*h > fast || *p > fast) {
        afxdev_set_error("hpssObj_new: orders %d / %d: the separation kernel covers odd orders up to %d", *h, *p, fast);
        return AFX_ERR_UNSUPPORTED;
    }
    return 0;
}

int hpssObj_new(HPSSObj *hpssObj, int radix2Exp, WindowType *windowType, int *slideLength, int *hOrder, int *pOrder) {
    (void)slideLength; /* hpss_algorithm.c:81 overwrites it with fftLength/4 */
    if (!hpssObj) return -1;
    *hpssObj = NULL;
    WindowType wt;
    int h, p;
    int st = hpss_params(radix2Exp, windowType, hOrder, pOrder, &wt, &h, &p);
    if (st != 0) return st;
    HPSSObj o = (HPSSObj)calloc(1, sizeof(struct OpaqueHPSS));
    if (!o) return AFX_ERR_NOMEM;
    o->radix2Exp = radix2Exp;
    o->fftLength = 1 << radix2Exp;
    o->slideLength = o->fftLength / 4;
    o->hOrder = h;
    o->pOrder = p;
    int hop = o->slideLength;
    st = stftObj_new(&o->stft, radix2Exp, &wt, &hop, NULL);
    if (st == 0) {
        o->stream = o->stft->stream;
        /* the window never changes: uploaded here, so that no compute call has to */
        st = afxdev_h2d(o->stft->dWindow, o->stft->windowDataArr, sizeof(float) * (size_t)o->fftLength, o->stream);
        if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
        if (st == AFX_OK) o->stft->windowDirty = 0;
    }
    if (st != 0) {
        hpssObj_free(o);
        return st;
    }
    *hpssObj = o;
    return 0;
}

int hpssObj_calDataLength(HPSSObj o, int dataLength) {
    if (!o) return 0;
    return (afx_frames(dataLength, o->fftLength, o->slideLength) - 1) * o->slideLength + o->fftLength;
}

/* chunks of whole clips: forward half spectrum -> masked spectra (or magnitudes) -> one inverse per requested output */
static int run(HPSSObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dH, float *dP,
               long long outStride, float *dHMag, float *dPMag, void *stream) {
    const int N = o->fftLength, F = N / 2 + 1, hop = o->slideLength;
    const int T = afx_frames(dataLength, N, hop);
    if (T <= 0) return AFX_OK;
    const int nOut = (dH != NULL) + (dP != NULL);
    int st = afx_scratch_enter(&o->scratchStream, stream); /* dSpec */
    if (st != AFX_OK) return st;
    const size_t clipFloats = (size_t)T * (2 * (size_t)F + 2 * (size_t)nOut * N);
    size_t chunk = chunk_bytes() / (sizeof(float) * clipFloats);
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)batch) chunk = (size_t)batch;
    /* (a launch of the transforms takes at most 2^31 - 1 frames) */
    while (chunk > 1 && chunk * (size_t)T > 0x7fffffffu) chunk /= 2;
    st = afxdev_reserve((void **)&o->dSpec, &o->capSpec, sizeof(float) * clipFloats * chunk);
    if (st != AFX_OK) return st;
    for (int c0 = 0; c0 < batch; c0 += (int)chunk) {
        const int nc = batch - c0 < (int)chunk ? batch - c0 : (int)chunk;
        const size_t rows = (size_t)nc * T;
        /* [full spectra of the outputs | half spectrum re | im]: the planes the inverse reads start on 16-byte boundaries */
        float *full = o->dSpec;
        float *sRe = full + 2 * (size_t)nOut * rows * N, *sIm = sRe + rows * F;
        AfxStftArgs s;
        afx_stft_args(&s, dData + (long long)c0 * clipStride, clipStride, nc, dataLength, T, o->radix2Exp, hop, o->stft->dWindow,
                      o->stft->dTwiddle, AFX_SPEC_COMPLEX, 0, F, sRe, sIm);
        st = afxk_stft(&s, stream);
        if (st != AFX_OK) return st;
        AfxHpssArgs a;
        memset(&a, 0, sizeof(a));
        a.re = sRe;
        a.im = sIm;
        a.rows = (long long)rows;
        a.framesPerClip = T;
        a.cols = a.pitch = F;
        a.hOrder = o->hOrder;
        a.pOrder = o->pOrder;
        a.fftLength = N;
        float *next = full;
        if (dH) {
            a.hRe = next;
            a.hIm = next + rows * N;
            next += 2 * rows * N;
        }
        if (dP) {
            a.pRe = next;
            a.pIm = next + rows * N;
        }
        if (dHMag) a.hMag = dHMag + (size_t)c0 * T * F;
        if (dPMag) a.pMag = dPMag + (size_t)c0 * T * F;
        st = afxk_hpss_mask(&a, stream);
        if (st != AFX_OK) return st;
        /* weighted overlap-add (type 0, hpss_algorithm.c:272 / :298), adding onto the caller's samples */
        if (dH) st = stftObj_istftBatchDevice(o->stft, a.hRe, a.hIm, nc, T, 0, dH + (long long)c0 * outStride, outStride, stream);
        if (st == AFX_OK && dP)
            st = stftObj_istftBatchDevice(o->stft, a.pRe, a.pIm, nc, T, 0, dP + (long long)c0 * outStride, outStride, stream);
        if (st != AFX_OK) return st;
    }
    return AFX_OK;
}

int hpssObj_hpssBatchDevice(HPSSObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dH, float *dP,
                            long long outStride, void *hipStream) {
    AFX_ENTER(o);
    if (!o || !dData || (!dH && !dP) || batch <= 0 || dataLength <= 0) return AFX_ERR_ARG;
    if (afx_frames(dataLength, o->fftLength, o->slideLength) > 0 && outStride < hpssObj_calDataLength(o, dataLength)) return AFX_ERR_ARG;
    return run(o, dData, batch, dataLength, clipStride, dH, dP, outStride, NULL, NULL, hipStream);
}

int hpssObj_spectraBatchDevice(HPSSObj o, const float *dData, int batch, int dataLength, long long clipStride, float *dHMag,
                               float *dPMag, void *hipStream) {
    AFX_ENTER(o);
    if (!o || !dData || (!dHMag && !dPMag) || batch <= 0 || dataLength <= 0) return AFX_ERR_ARG;
    return run(o, dData, batch, dataLength, clipStride, NULL, NULL, 0, dHMag, dPMag, hipStream);
}

int afx_medianFilterDevice(const float *dIn, long long rows, int cols, int framesPerClip, int axis, int order, float *dOut,
                           void *hipStream) {
    if (!dIn || !dOut || dIn == dOut || rows <= 0 || cols <= 0 || framesPerClip < 0 || (axis != 0 && axis != 1)) return AFX_ERR_ARG;
    if (order < 1 || !(order & 1) || order > AFX_MEDIAN_MAX_ORDER) {
        afxdev_set_error("afx_medianFilterDevice: order %d is not an odd number in 1 ... %d", order, AFX_MEDIAN_MAX_ORDER);
        return AFX_ERR_UNSUPPORTED;
    }
    int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    return afxk_median_filter(dIn, rows, cols, framesPerClip, axis, order, dOut, hipStream);
}

void hpssObj_hpss(HPSSObj o, float *dataArr, int dataLength, float *hArr, float *pArr) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("hpssObj_hpss: NULL object");
        return;
    }
    if ((!hArr && !pArr) || !dataArr || dataLength <= 0) return; /* hpss_algorithm.c:141-143 */
    if (afx_frames(dataLength, o->fftLength, o->slideLength) <= 0) return;
    const int outLength = hpssObj_calDataLength(o, dataLength);
    const size_t inB = sizeof(float) * (size_t)dataLength, outB = sizeof(float) * (size_t)outLength;
    int st = afxdev_reserve((void **)&o->dX, &o->capX, inB);
    if (st == AFX_OK && hArr) st = afxdev_reserve((void **)&o->dH, &o->capH, outB);
    if (st == AFX_OK && pArr) st = afxdev_reserve((void **)&o->dP, &o->capP, outB);
    if (st == AFX_OK) st = afxdev_h2d(o->dX, dataArr, inB, o->stream);
    /* the reference adds the frames ONTO hArr / pArr (stft_algorithm.c:382); carry the caller's content along */
    if (st == AFX_OK && hArr) st = afxdev_h2d(o->dH, hArr, outB, o->stream);
    if (st == AFX_OK && pArr) st = afxdev_h2d(o->dP, pArr, outB, o->stream);
    if (st == AFX_OK)
        st = run(o, o->dX, 1, dataLength, dataLength, hArr ? o->dH : NULL, pArr ? o->dP : NULL, outLength, NULL, NULL, o->stream);
    if (st == AFX_OK && hArr) st = afxdev_d2h(hArr, o->dH, outB, o->stream);
    if (st == AFX_OK && pArr) st = afxdev_d2h(pArr, o->dP, outB, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) AFX_FAIL(o, st, "hpssObj_hpss");
}

void hpssObj_debug(HPSSObj o) {
    if (!o) return;
    printf("hpss params is: fftLength=%d, slideLength=%d, hOrder=%d, pOrder=%d\n", o->fftLength, o->slideLength, o->hOrder,
           o->pOrder);
}

void hpssObj_free(HPSSObj o) {
    if (!o) return;
    if (o->stream) afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->scratchStream);
    afxdev_free(o->dSpec);
    afxdev_free(o->dX);
    afxdev_free(o->dH);
    afxdev_free(o->dP);
    stftObj_free(o->stft); /* destroys the stream */
    free(o);
}

/* ---- test hook (host logic only, no device): tests/test_hpss_cpu.py ------------------------------------------------ */
/* what hpssObj_new would decide and what hpssObj_calDataLength would answer: out = {status, windowType, hop, hOrder, pOrder,
 * frames, calDataLength} */
int afx_test_hpss_plan(int radix2Exp, const int *windowType, const int *slideLength, const int *hOrder, const int *pOrder,
                       int dataLength, int *out) {
    (void)slideLength;
    WindowType wt, in = windowType ? (WindowType)*windowType : Window_Hamm;
    int h, p;
    const int st = hpss_params(radix2Exp, windowType ? &in : NULL, hOrder, pOrder, &wt, &h, &p);
    out[0] = st;
    out[1] = (int)wt;
    out[3] = h;
    out[4] = p;
    out[2] = out[5] = out[6] = 0;
    if (st != 0) return st;
    const int N = 1 << radix2Exp, hop = N / 4;
    out[2] = hop;
    out[5] = afx_frames(dataLength, N, hop);
    out[6] = (out[5] - 1) * hop + N;
    return 0;
}
