/* afx_descriptor.c -- the spectral-descriptor object (C host side) behind include/feature/spectral_algorithm.h, the
 * descriptor methods of the spectrogram object (include/spectrogram_algorithm.h) and spectralObj_computeDevice
 * (include/afx_batch.h).
 *
 * Parameter semantics follow src/feature/spectral_algorithm.c:57-1160 and src/flux_spectral.c:21-833.  The reference
 * loops over the rows once per intermediate (sum, centroid, spread, ...) and caches them between calls; here every call
 * is one pass of csrc/hip/afx_descriptors.hip over the rows it is handed, and nothing is cached: the reference's caches
 * survive a change of the data under an unchanged object (they are reset in setTimeLength / setEdge only), this object
 * cannot return a stale value.  The per-edge constants of slope / mean / var (mean frequency and its squared
 * deviations) are summed here in float32 in the reference's order.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "feature/spectral_algorithm.h"

/* AfxSpectralKind (public, include/afx_batch.h) and AFX_DESC_* (device layer, afx_device.h) are one numbering: requests go
 * to the launcher as they come, and the frame-difference / phase kinds are recognised by their ranges */
#define AFX_SAME_KIND(name) \
    typedef char afx_kind_check_##name[(int)AFX_SD_##name == (int)AFX_DESC_##name ? 1 : -1]
AFX_SAME_KIND(FLATNESS);
AFX_SAME_KIND(FLUX);
AFX_SAME_KIND(HFC);
AFX_SAME_KIND(SD);
AFX_SAME_KIND(MKL);
AFX_SAME_KIND(PD);
AFX_SAME_KIND(RCD);
AFX_SAME_KIND(BROADBAND);
AFX_SAME_KIND(NOVELTY);
AFX_SAME_KIND(EEF);
AFX_SAME_KIND(MAX);
AFX_SAME_KIND(VAR);
AFX_SAME_KIND(COUNT);

static int kind_slots(int kind) {
    return kind == AFX_SD_MAX || kind == AFX_SD_MEAN || kind == AFX_SD_VAR ? 2 : 1;
}
static int kind_needs_phase(int kind) { return kind >= AFX_SD_PD && kind <= AFX_SD_RCD; }

int afx_spectralSlots(const AfxSpectralRequest *requests, int count) {
    if (!requests || count <= 0) return AFX_ERR_ARG;
    int slots = 0;
    for (int i = 0; i < count; i++) {
        if (requests[i].kind < 0 || requests[i].kind >= AFX_SD_COUNT) return AFX_ERR_ARG;
        slots += kind_slots(requests[i].kind);
    }
    return slots;
}

/* the constants of the current edge (spectral_algorithm.c:1120-1128, flux_spectral.c:346-355, spectral_algorithm.c:1004-1019) */
static void edge_constants(SpectralObj o) {
    const int n = o->indexLength;
    float mean = 0, den = 0;
    for (int j = 0; j < n; j++) mean += o->freBandArr[o->indexArr[j]];
    mean = mean / n;
    for (int j = 0; j < n; j++) {
        const float v = o->freBandArr[o->indexArr[j]] - mean;
        den += v * v;
    }
    o->meanFre = mean;
    o->slopeDen = den;
    float var = 0;
    for (int j = 0; j < n; j++) {
        const float v = mean - o->freBandArr[o->indexArr[j]];
        var += v * v;
    }
    o->varFre = n > 1 ? var / (n - 1) : 0;
}

static int *range_indices(int start, int end) {
    int *idx = (int *)calloc((size_t)(end - start + 1), sizeof(int));
    if (idx)
        for (int i = start; i <= end; i++) idx[i - start] = i;
    return idx;
}

int spectralObj_new(SpectralObj *spectralObj, int num, float *freBandArr) {
    if (!spectralObj) return -1;
    *spectralObj = NULL;
    if (num < 2) { /* spectral_algorithm.c:66-69 */
        printf("num is error!!!\n");
        return -1;
    }
    if (!freBandArr) return -1;
    int st = afxdev_ensure();
    if (st != AFX_OK) return st;
    SpectralObj o = (SpectralObj)calloc(1, sizeof(struct OpaqueSpectral));
    if (!o) return AFX_ERR_NOMEM;
    o->num = num;
    o->freBandArr = (float *)malloc(sizeof(float) * (size_t)num);
    o->indexArr = range_indices(0, num - 1);
    if (!o->freBandArr || !o->indexArr) st = AFX_ERR_NOMEM;
    if (st == AFX_OK) {
        memcpy(o->freBandArr, freBandArr, sizeof(float) * (size_t)num);
        o->indexLength = num;
        o->start = 0;
        o->end = num - 1;
        o->isRange = 1;
        edge_constants(o);
        st = afxdev_stream_create(&o->stream);
    }
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dFre, sizeof(float) * (size_t)num);
    if (st == AFX_OK) st = afxdev_h2d(o->dFre, o->freBandArr, sizeof(float) * (size_t)num, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) {
        spectralObj_free(o);
        return st;
    }
    *spectralObj = o;
    return 0;
}

void spectralObj_setTimeLength(SpectralObj o, int timeLength) {
    if (o) o->timeLength = timeLength;
}

void spectralObj_setEdge(SpectralObj o, int start, int end) {
    if (!o) return;
    if (!(start >= 0 && end <= o->num - 1 && end > start)) return; /* spectral_algorithm.c:164 */
    int *idx = range_indices(start, end);
    if (!idx) {
        afxdev_report_failure("spectralObj_setEdge", AFX_ERR_NOMEM);
        return;
    }
    free(o->indexArr);
    o->indexArr = idx;
    o->indexLength = end - start + 1;
    o->start = start;
    o->end = end;
    o->isRange = 1;
    edge_constants(o);
}

void spectralObj_setEdgeArr(SpectralObj o, int *indexArr, int indexLength) {
    if (!o || !indexArr) return;
    AFX_ENTER(o);
    if (indexLength < 1) { /* (the reference would read indexArr[-1]) */
        free(indexArr);
        return;
    }
    for (int i = 0; i < indexLength; i++)
        if (indexArr[i] < 0 || indexArr[i] > o->num - 1) { /* spectral_algorithm.c:193-199 */
            free(indexArr);
            return;
        }
    /* the device table first: the edge changes only when the kernels can have it */
    if (o->stream) afxdev_stream_sync(o->stream);
    int st = afxdev_reserve((void **)&o->dIndex, &o->capIndex, sizeof(int) * (size_t)indexLength);
    if (st == AFX_OK) st = afxdev_h2d(o->dIndex, indexArr, sizeof(int) * (size_t)indexLength, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) {
        free(indexArr);
        AFX_FAIL(o, st, "spectralObj_setEdgeArr");
        return;
    }
    free(o->indexArr);
    o->indexArr = indexArr;
    o->indexLength = indexLength;
    o->start = indexArr[0];
    o->end = indexArr[indexLength - 1];
    o->isRange = 0;
    edge_constants(o);
}

/* one launch pair per pass: a pass takes the first request of every kind not served yet */
int spectralObj_computeDevice(SpectralObj o, const float *dSpec, const float *dPhase, long long rows, int framesPerClip,
                              const AfxSpectralRequest *requests, int count, float *dOut, long long outStride,
                              void *hipStream) {
    AFX_ENTER(o);
    const int slots = afx_spectralSlots(requests, count);
    if (slots < 0 || count > 4096) {
        afxdev_set_error("spectralObj_computeDevice: count %d, or a kind outside AfxSpectralKind", count);
        return AFX_ERR_ARG;
    }
    for (int i = 0; i < count; i++)
        if (kind_needs_phase(requests[i].kind) && !dPhase) {
            afxdev_set_error("spectralObj_computeDevice: request %d (kind %d) needs dPhase", i, requests[i].kind);
            return AFX_ERR_ARG;
        }
    if (!o || !dSpec || !dOut || rows < 0 || framesPerClip < 0 || outStride < rows) {
        afxdev_set_error("spectralObj_computeDevice: bad argument");
        return AFX_ERR_ARG;
    }
    if (rows == 0) return AFX_OK;
    AfxDescArgs a;
    memset(&a, 0, sizeof(a));
    a.spec = dSpec;
    a.phase = dPhase;
    a.out = dOut;
    a.rows = rows;
    a.outStride = outStride;
    a.framesPerClip = framesPerClip;
    a.num = o->num;
    a.start = o->isRange ? o->start : 0;
    a.len = o->indexLength;
    a.idx = o->isRange ? NULL : o->dIndex;
    a.idx0 = o->indexArr[0];
    a.fre = o->dFre;
    a.meanFre = o->meanFre;
    a.slopeDen = o->slopeDen;
    a.varFre = o->varFre;
    a.isPower = o->isPower;

    AfxDescReq pass[AFX_SD_COUNT];
    char *done = (char *)calloc((size_t)count, 1);
    if (!done) return AFX_ERR_NOMEM;
    int left = count, st = AFX_OK;
    while (left > 0 && st == AFX_OK) {
        char taken[AFX_SD_COUNT] = {0};
        int n = 0, slot = 0;
        for (int i = 0; i < count; i++) {
            const int kind = requests[i].kind;
            if (!done[i] && !taken[kind]) {
                taken[kind] = 1;
                done[i] = 1;
                left--;
                pass[n].kind = kind;
                memcpy(pass[n].iarg, requests[i].iarg, sizeof(pass[n].iarg));
                memcpy(pass[n].farg, requests[i].farg, sizeof(pass[n].farg));
                pass[n].slot = slot;
                n++;
            }
            slot += kind_slots(kind);
        }
        a.req = pass;
        a.count = n;
        st = afxk_descriptors(&a, hipStream);
    }
    free(done);
    return st;
}

/* the legacy protocol: upload timeLength x num floats (and the phase), one request on the object's stream, download */
static void run_host(SpectralObj o, const char *who, int timeLength, const float *mSpec, const float *mPhase,
                     const AfxSpectralRequest *req, float *out0, float *out1) {
    if (!o) {
        afxdev_set_error("%s: NULL object", who);
        return;
    }
    AFX_ENTER(o);
    const int two = kind_slots(req->kind) == 2;
    if (timeLength <= 0 || !mSpec || !out0 || (two && !out1) || (kind_needs_phase(req->kind) && !mPhase)) return;
    if (req->kind == AFX_SD_VAR && o->indexLength < 2) return; /* spectral_algorithm.c:929-931 */
    const size_t T = (size_t)timeLength, inBytes = sizeof(float) * T * o->num;
    int st = afxdev_reserve((void **)&o->dIn, &o->capIn, inBytes);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dOut, &o->capOut, sizeof(float) * T * 2);
    if (st == AFX_OK) st = afxdev_h2d(o->dIn, mSpec, inBytes, o->stream);
    if (st == AFX_OK && mPhase && kind_needs_phase(req->kind)) {
        st = afxdev_reserve((void **)&o->dPhase, &o->capPhase, inBytes);
        if (st == AFX_OK) st = afxdev_h2d(o->dPhase, mPhase, inBytes, o->stream);
    }
    if (st == AFX_OK)
        st = spectralObj_computeDevice(o, o->dIn, kind_needs_phase(req->kind) ? o->dPhase : NULL, (long long)T, 0, req, 1,
                                       o->dOut, (long long)T, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(out0, o->dOut, sizeof(float) * T, o->stream);
    if (st == AFX_OK && two) st = afxdev_d2h(out1, o->dOut + T, sizeof(float) * T, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) AFX_FAIL(o, st, who);
}

static AfxSpectralRequest request(int kind, int i0, int i1, int i2, int i3, float f0) {
    AfxSpectralRequest r;
    memset(&r, 0, sizeof(r));
    r.kind = kind;
    r.iarg[0] = i0;
    r.iarg[1] = i1;
    r.iarg[2] = i2;
    r.iarg[3] = i3;
    r.farg[0] = f0;
    return r;
}

/* Every descriptor twice: on the descriptor object (timeLength from spectralObj_setTimeLength) and on the spectrogram
 * object (its own descriptor state, timeLength of its last spectrogram call), one macro per prototype shape. */
#define D_PLAIN(name, KIND)                                                                                       \
    void spectralObj_##name(SpectralObj o, float *m, float *d) {                                                  \
        const AfxSpectralRequest r = request(KIND, 0, 0, 0, 0, 0);                                                \
        run_host(o, "spectralObj_" #name, o ? o->timeLength : 0, m, NULL, &r, d, NULL);                          \
    }                                                                                                             \
    void spectrogramObj_##name(SpectrogramObj s, float *m, float *d) {                                            \
        int T = 0;                                                                                                \
        SpectralObj o = afx_spectrogram_descriptor(s, "spectrogramObj_" #name, &T);                              \
        const AfxSpectralRequest r = request(KIND, 0, 0, 0, 0, 0);                                                \
        if (o) run_host(o, "spectrogramObj_" #name, T, m, NULL, &r, d, NULL);                                    \
    }
#define D_PHASE(name, KIND)                                                                                       \
    void spectralObj_##name(SpectralObj o, float *m, float *ph, float *d) {                                       \
        const AfxSpectralRequest r = request(KIND, 0, 0, 0, 0, 0);                                                \
        run_host(o, "spectralObj_" #name, o ? o->timeLength : 0, m, ph, &r, d, NULL);                            \
    }                                                                                                             \
    void spectrogramObj_##name(SpectrogramObj s, float *m, float *ph, float *d) {                                 \
        int T = 0;                                                                                                \
        SpectralObj o = afx_spectrogram_descriptor(s, "spectrogramObj_" #name, &T);                              \
        const AfxSpectralRequest r = request(KIND, 0, 0, 0, 0, 0);                                                \
        if (o) run_host(o, "spectrogramObj_" #name, T, m, ph, &r, d, NULL);                                      \
    }
#define D_PAIR(name, KIND)                                                                                        \
    void spectralObj_##name(SpectralObj o, float *m, float *v, float *f) {                                        \
        const AfxSpectralRequest r = request(KIND, 0, 0, 0, 0, 0);                                                \
        run_host(o, "spectralObj_" #name, o ? o->timeLength : 0, m, NULL, &r, v, f);                             \
    }                                                                                                             \
    void spectrogramObj_##name(SpectrogramObj s, float *m, float *v, float *f) {                                  \
        int T = 0;                                                                                                \
        SpectralObj o = afx_spectrogram_descriptor(s, "spectrogramObj_" #name, &T);                              \
        const AfxSpectralRequest r = request(KIND, 0, 0, 0, 0, 0);                                                \
        if (o) run_host(o, "spectrogramObj_" #name, T, m, NULL, &r, v, f);                                       \
    }
/* descriptors with parameters: DECL as declared, REQ the request built from them */
#define D_PARAM(name, DECL, REQ)                                                                                  \
    void spectralObj_##name(SpectralObj o, float *m, DECL, float *d) {                                            \
        const AfxSpectralRequest r = REQ;                                                                         \
        run_host(o, "spectralObj_" #name, o ? o->timeLength : 0, m, NULL, &r, d, NULL);                          \
    }                                                                                                             \
    void spectrogramObj_##name(SpectrogramObj s, float *m, DECL, float *d) {                                      \
        int T = 0;                                                                                                \
        SpectralObj o = afx_spectrogram_descriptor(s, "spectrogramObj_" #name, &T);                              \
        const AfxSpectralRequest r = REQ;                                                                         \
        if (o) run_host(o, "spectrogramObj_" #name, T, m, NULL, &r, d, NULL);                                    \
    }
#define COMMA ,

D_PLAIN(flatness, AFX_SD_FLATNESS)
/* spectral_algorithm.c:250-280: isExp / type NULL -> 0 */
D_PARAM(flux, int step COMMA float p COMMA int isPostive COMMA int *isExp COMMA int *type,
        request(AFX_SD_FLUX, step, isPostive, isExp ? *isExp : 0, type ? *type : 0, p))
D_PARAM(rolloff, float threshold, request(AFX_SD_ROLLOFF, 0, 0, 0, 0, threshold))
D_PLAIN(centroid, AFX_SD_CENTROID)
D_PLAIN(spread, AFX_SD_SPREAD)
D_PLAIN(skewness, AFX_SD_SKEWNESS)
D_PLAIN(kurtosis, AFX_SD_KURTOSIS)
D_PARAM(entropy, int isNorm, request(AFX_SD_ENTROPY, isNorm, 0, 0, 0, 0))
D_PLAIN(crest, AFX_SD_CREST)
D_PLAIN(slope, AFX_SD_SLOPE)
D_PLAIN(decrease, AFX_SD_DECREASE)
D_PARAM(bandWidth, float p, request(AFX_SD_BANDWIDTH, 0, 0, 0, 0, p))
D_PLAIN(rms, AFX_SD_RMS)
D_PARAM(energy, int isLog COMMA float gamma, request(AFX_SD_ENERGY, isLog, 0, 0, 0, gamma))
D_PLAIN(hfc, AFX_SD_HFC)
D_PARAM(sd, int step COMMA int isPostive, request(AFX_SD_SD, step, isPostive, 0, 0, 0))
D_PARAM(sf, int step COMMA int isPostive, request(AFX_SD_SF, step, isPostive, 0, 0, 0))
D_PARAM(mkl, int type, request(AFX_SD_MKL, type, 0, 0, 0, 0))
D_PHASE(pd, AFX_SD_PD)
D_PHASE(wpd, AFX_SD_WPD)
D_PHASE(nwpd, AFX_SD_NWPD)
D_PHASE(cd, AFX_SD_CD)
D_PHASE(rcd, AFX_SD_RCD)
D_PARAM(broadband, float threshold, request(AFX_SD_BROADBAND, 0, 0, 0, 0, threshold))
/* spectral_algorithm.c:758-779, flux_spectral.c:789-799: NULL -> Sub / Value */
D_PARAM(novelty, int step COMMA float threshold COMMA SpectralNoveltyMethodType *methodType COMMA SpectralNoveltyDataType *dataType,
        request(AFX_SD_NOVELTY, step, methodType ? (int)*methodType : 0, dataType ? (int)*dataType : 0, 0, threshold))
D_PARAM(eef, int isNorm, request(AFX_SD_EEF, isNorm, 0, 0, 0, 0))
D_PARAM(eer, int isNorm COMMA float gamma, request(AFX_SD_EER, isNorm, 0, 0, 0, gamma))
D_PAIR(max, AFX_SD_MAX)
D_PAIR(mean, AFX_SD_MEAN)
D_PAIR(var, AFX_SD_VAR)

void spectrogramObj_setEdge(SpectrogramObj s, int start, int end) {
    SpectralObj o = afx_spectrogram_descriptor(s, "spectrogramObj_setEdge", NULL);
    if (o) spectralObj_setEdge(o, start, end);
}

void spectrogramObj_setEdgeArr(SpectrogramObj s, int *indexArr, int indexLength) {
    SpectralObj o = afx_spectrogram_descriptor(s, "spectrogramObj_setEdgeArr", NULL);
    if (o) spectralObj_setEdgeArr(o, indexArr, indexLength);
    else free(indexArr);
}

void spectralObj_free(SpectralObj o) {
    if (!o) return;
    if (o->stream) afxdev_stream_sync(o->stream);
    afxdev_free(o->dFre);
    afxdev_free(o->dIndex);
    afxdev_free(o->dIn);
    afxdev_free(o->dPhase);
    afxdev_free(o->dOut);
    afxdev_stream_destroy(o->stream);
    free(o->freBandArr);
    free(o->indexArr);
    free(o);
}
