/* afx_onset.c -- the onset detector (C host side) behind include/mir/onset_algorithm.h, and the device-pointer calls of
 * include/afx_batch.h that came with it: onsetObj_onsetBatchDevice, afx_maxFilterDevice, afx_peakPickDevice,
 * afx_powerToDbDevice, util_powerToDB, afx_onset_plan_host.
 *
 * Mirrors the parameter semantics of the reference object (src/mir/onset_algorithm.c:58-460).  Execution per chunk of whole
 * clips, all on one stream: k_max_filter over the rows when the object filters (order >= 2), the descriptor kernels
 * (afxk_descriptors with framesPerClip = nLength: the arithmetic of spectralObj_computeDevice) over the caller's rows or
 * the filtered copy into one float per frame of scratch, k_onset_pick -- one workgroup per clip -- for normalisation,
 * envelope and points.  The host-pointer call is the batch of one through staging buffers.  There is no CPU compute path.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objects.h"
#include "mir/onset_algorithm.h"

/* filtered copy of one chunk of clips.  AFX_ONSET_CHUNK_MB overrides (the chunked == unchunked tests) */
static size_t chunk_bytes(void) {
    const char *s = getenv("AFX_ONSET_CHUNK_MB");
    size_t mb = 1024;
    if (s && atoi(s) > 0) mb = (size_t)atoi(s);
    return mb << 20;
}

/* onset_algorithm.c:123-133: the products in double, then floorf */
int afx_onset_plan_host(int samplate, int slideLength, int out[5], float *delta) {
    if (!out) return AFX_ERR_ARG;
    if (samplate <= 0) samplate = 32000;
    if (slideLength < 1) slideLength = 512;
    out[0] = (int)floorf(0.03 * samplate / slideLength);
    out[1] = (int)floorf(0.0 * samplate / slideLength + 1);
    out[2] = (int)floorf(0.1 * samplate / slideLength);
    out[3] = (int)floorf(0.1 * samplate / slideLength + 1);
    out[4] = (int)floorf(0.03 * samplate / slideLength);
    if (delta) *delta = 0.07f;
    return 0;
}

int onsetObj_new(OnsetObj *onsetObj, int nLength, int mLength, int slideLength, int *samplate, int *filterOrder,
                 NoveltyType *type) {
    if (!onsetObj) return -1;
    *onsetObj = NULL;
    if (nLength < 1 || mLength < 1) {
        afxdev_set_error("onsetObj_new: nLength %d, mLength %d", nLength, mLength);
        return AFX_ERR_ARG;
    }
    int st = afxdev_ensure();
    if (st != AFX_OK) return st;
    OnsetObj o = (OnsetObj)calloc(1, sizeof(struct OpaqueOnset));
    if (!o) return AFX_ERR_NOMEM;
    o->noveltyType = type ? (int)*type : (int)Novelty_Flux;
    o->nLength = nLength;
    o->mLength = mLength;
    o->order = (filterOrder && *filterOrder > 0) ? *filterOrder : 1;
    o->step = 1;
    int pick[5];
    afx_onset_plan_host(samplate ? *samplate : 0, slideLength, pick, &o->delta);
    o->preMax = pick[0];
    o->postMax = pick[1];
    o->preAvg = pick[2];
    o->postAvg = pick[3];
    o->wait = pick[4];
    st = afxdev_stream_create(&o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dFre, sizeof(float) * (size_t)mLength);
    if (st == AFX_OK) st = afxdev_memset(o->dFre, 0, sizeof(float) * (size_t)mLength, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) {
        onsetObj_free(o);
        return st;
    }
    *onsetObj = o;
    return 0;
}

static int is_phase_kind(int type) { return type >= (int)Novelty_PD && type <= (int)Novelty_RCD; }

/* _onsetObj_initParam (onset_algorithm.c:135-179) and the dispatch of _onsetObj_dealFluxArr (:318-377) as one descriptor
 * request; *step: what the reference's memset (:316) takes */
static AfxDescReq novelty_request(int type, const NoveltyParam *param, int *step) {
    int st = 1, isPostive = 1, isExp = 0, sumType = 0;
    float p = 1, threshold = 0;
    if (param) {
        if (param->step > 0) st = param->step;
        if (param->p != 0) p = param->p;
        isPostive = param->isPostive;
        isExp = param->isExp;
        sumType = param->type;
        threshold = param->threshold;
    }
    *step = st;
    AfxDescReq r;
    memset(&r, 0, sizeof(r));
    switch (type) {
        case Novelty_HFC: r.kind = AFX_DESC_HFC; break;
        case Novelty_SD:
        case Novelty_SF:
            r.kind = type == Novelty_SD ? AFX_DESC_SD : AFX_DESC_SF;
            r.iarg[0] = st;
            r.iarg[1] = isPostive;
            break;
        case Novelty_MKL:
            r.kind = AFX_DESC_MKL;
            r.iarg[0] = sumType;
            break;
        case Novelty_PD: r.kind = AFX_DESC_PD; break;
        case Novelty_WPD: r.kind = AFX_DESC_WPD; break;
        case Novelty_NWPD: r.kind = AFX_DESC_NWPD; break;
        case Novelty_CD: r.kind = AFX_DESC_CD; break;
        case Novelty_RCD: r.kind = AFX_DESC_RCD; break;
        case Novelty_Broadband:
            r.kind = AFX_DESC_BROADBAND;
            r.farg[0] = threshold;
            break;
        default: /* flux, and every value that is no named kind (:372) */
            r.kind = AFX_DESC_FLUX;
            r.iarg[0] = st;
            r.iarg[1] = isPostive;
            r.iarg[2] = isExp;
            r.iarg[3] = sumType;
            r.farg[0] = p;
            break;
    }
    return r;
}

/* the refusals both calls share (mir/onset_algorithm.h) */
static int check_call(OnsetObj o, const char *who, int hasPhase, int step, const int *indexArr, int indexLength) {
    if (is_phase_kind(o->noveltyType) && !hasPhase) {
        afxdev_set_error("%s: novelty type %d needs the phase rows", who, o->noveltyType);
        return AFX_ERR_ARG;
    }
    if (step > o->nLength) {
        afxdev_set_error("%s: step %d beyond the %d frames", who, step, o->nLength);
        return AFX_ERR_ARG;
    }
    if (indexArr) {
        if (indexLength < 1) {
            afxdev_set_error("%s: indexLength %d", who, indexLength);
            return AFX_ERR_ARG;
        }
        for (int i = 0; i < indexLength; i++)
            if (indexArr[i] < 0 || indexArr[i] > o->mLength - 1) {
                afxdev_set_error("%s: index %d (entry %d) outside 0 ... %d", who, indexArr[i], i, o->mLength - 1);
                return AFX_ERR_ARG;
            }
    }
    return AFX_OK;
}

/* the index table on the device: uploaded when it differs from the one the object holds.  The previous launches that read
 * the old table precede the copy on `stream` (another stream was drained by afx_scratch_enter) */
static int index_table(OnsetObj o, const int *indexArr, int indexLength, void *stream) {
    const size_t bytes = sizeof(int) * (size_t)indexLength;
    if (o->hIndex && o->indexLength == indexLength && memcmp(o->hIndex, indexArr, bytes) == 0) return AFX_OK;
    int *h = (int *)realloc(o->hIndex, bytes);
    if (!h) return AFX_ERR_NOMEM;
    o->hIndex = h;
    o->indexLength = 0; /* until the device has it */
    memcpy(h, indexArr, bytes);
    int st = afxdev_reserve((void **)&o->dIndex, &o->capIndex, bytes);
    if (st == AFX_OK) st = afxdev_h2d(o->dIndex, h, bytes, stream);
    if (st == AFX_OK) o->indexLength = indexLength;
    return st;
}

/* chunks of whole clips: filter -> novelty -> normalise and pick */
static int run(OnsetObj o, const float *dSpec, const float *dPhase, int batch, const AfxDescReq *req, const int *indexArr,
               int indexLength, float *dEvn, int *dPoint, int *dCount, long long outStride, long long pointStride, void *stream) {
    const int n = o->nLength, m = o->mLength;
    int st = afx_scratch_enter(&o->scratchStream, stream);
    if (st != AFX_OK) return st;
    if (indexArr) {
        st = index_table(o, indexArr, indexLength, stream);
        if (st != AFX_OK) return st;
    }
    const size_t clipFloats = (size_t)n * (size_t)m;
    size_t chunk = (size_t)batch;
    if (o->order >= 2) {
        chunk = chunk_bytes() / (sizeof(float) * clipFloats);
        if (chunk < 1) chunk = 1;
        if (chunk > (size_t)batch) chunk = (size_t)batch;
    }
    if (o->order >= 2) {
        st = afxdev_reserve((void **)&o->dFilt, &o->capFilt, sizeof(float) * clipFloats * chunk);
        if (st != AFX_OK) return st;
    }
    st = afxdev_reserve((void **)&o->dRaw, &o->capRaw, sizeof(float) * (size_t)n * chunk);
    if (st != AFX_OK) return st;
    for (int c0 = 0; c0 < batch; c0 += (int)chunk) {
        const int nc = batch - c0 < (int)chunk ? batch - c0 : (int)chunk;
        const long long rows = (long long)nc * n;
        const float *spec = dSpec + (size_t)c0 * clipFloats;
        if (o->order >= 2) { /* mDataArr1 only, never the phase (:238-257) */
            st = afxk_max_filter(spec, rows, m, o->order, o->dFilt, stream);
            if (st != AFX_OK) return st;
            spec = o->dFilt;
        }
        AfxDescArgs a;
        memset(&a, 0, sizeof(a));
        a.spec = spec;
        a.phase = dPhase ? dPhase + (size_t)c0 * clipFloats : NULL;
        a.out = o->dRaw;
        a.rows = rows;
        a.outStride = rows;
        a.framesPerClip = n;
        a.num = m;
        a.start = 0;
        a.len = indexArr ? indexLength : m;
        a.idx = indexArr ? o->dIndex : NULL;
        a.idx0 = indexArr ? indexArr[0] : 0;
        a.fre = o->dFre;
        AfxDescReq r = *req;
        r.slot = 0;
        a.req = &r;
        a.count = 1;
        st = afxk_descriptors(&a, stream);
        if (st != AFX_OK) return st;
        AfxOnsetPickArgs k;
        memset(&k, 0, sizeof(k));
        k.src = o->dRaw;
        k.srcStride = n;
        k.batch = nc;
        k.length = n;
        k.normalise = 1;
        k.evn = dEvn + (long long)c0 * outStride;
        k.evnStride = outStride;
        k.preMax = o->preMax;
        k.postMax = o->postMax;
        k.preAvg = o->preAvg;
        k.postAvg = o->postAvg;
        k.wait = o->wait;
        k.delta = o->delta;
        k.point = dPoint ? dPoint + (long long)c0 * pointStride : NULL;
        k.count = dCount ? dCount + c0 : NULL;
        k.pointStride = pointStride;
        st = afxk_onset_pick(&k, stream);
        if (st != AFX_OK) return st;
    }
    return AFX_OK;
}

int onsetObj_onsetBatchDevice(OnsetObj o, const float *dSpec, const float *dPhase, int batch, const NoveltyParam *param,
                              const int *indexArr, int indexLength, float *dEvn, int *dPoint, int *dCount, long long outStride,
                              long long pointStride, void *hipStream) {
    static const char *who = "onsetObj_onsetBatchDevice";
    if (!o || !dSpec || !dEvn || batch <= 0 || outStride < o->nLength || (dPoint && pointStride < 0)) {
        afxdev_set_error("%s: bad argument", who);
        return AFX_ERR_ARG;
    }
    int step = 1;
    const AfxDescReq req = novelty_request(o->noveltyType, param, &step);
    int st = check_call(o, who, dPhase != NULL, step, indexArr, indexLength);
    if (st != AFX_OK) return st;
    st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    o->step = step;
    return run(o, dSpec, is_phase_kind(o->noveltyType) ? dPhase : NULL, batch, &req, indexArr, indexLength, dEvn, dPoint, dCount,
               outStride, pointStride, hipStream);
}

int onsetObj_onset(OnsetObj o, float *mDataArr1, float *mDataArr2, NoveltyParam *param, int *indexArr, int indexLength,
                   float *evnArr, int *pointArr) {
    static const char *who = "onsetObj_onset";
    if (!o || !mDataArr1 || !evnArr || !pointArr) {
        afxdev_set_error("%s: NULL object or array", who);
        return AFX_ERR_ARG;
    }
    AFX_ENTER(o);
    int step = 1;
    const AfxDescReq req = novelty_request(o->noveltyType, param, &step);
    int st = check_call(o, who, mDataArr2 != NULL, step, indexArr, indexLength);
    if (st != AFX_OK) return st;
    o->step = step;
    const int n = o->nLength, phase = is_phase_kind(o->noveltyType);
    const size_t inB = sizeof(float) * (size_t)n * (size_t)o->mLength;
    int count = 0;
    st = afxdev_reserve((void **)&o->dIn, &o->capIn, inB);
    if (st == AFX_OK && phase) st = afxdev_reserve((void **)&o->dPhase, &o->capPhase, inB);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dEvn, &o->capEvn, sizeof(float) * (size_t)n);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dPoint, &o->capPoint, sizeof(int) * ((size_t)n + 1));
    if (st == AFX_OK) st = afxdev_h2d(o->dIn, mDataArr1, inB, o->stream);
    if (st == AFX_OK && phase) st = afxdev_h2d(o->dPhase, mDataArr2, inB, o->stream);
    if (st == AFX_OK)
        st = run(o, o->dIn, phase ? o->dPhase : NULL, 1, &req, indexArr, indexLength, o->dEvn, o->dPoint, o->dPoint + n, n, n,
                 o->stream);
    if (st == AFX_OK) st = afxdev_d2h(evnArr, o->dEvn, sizeof(float) * (size_t)n, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(&count, o->dPoint + n, sizeof(int), o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st == AFX_OK && (count < 0 || count > n)) { /* (no picker writes such a count) */
        afxdev_set_error("%s: the device reported %d points of %d frames", who, count, n);
        st = AFX_ERR_HIP;
    }
    if (st == AFX_OK && count > 0) { /* the points themselves: as many as there are */
        st = afxdev_d2h(pointArr, o->dPoint, sizeof(int) * (size_t)count, o->stream);
        if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    }
    if (st != AFX_OK) {
        AFX_FAIL(o, st, who);
        return st;
    }
    return count;
}

void onsetObj_free(OnsetObj o) {
    if (!o) return;
    if (o->stream) afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->scratchStream);
    afxdev_free(o->dFre);
    afxdev_free(o->dIndex);
    afxdev_free(o->dFilt);
    afxdev_free(o->dRaw);
    afxdev_free(o->dIn);
    afxdev_free(o->dPhase);
    afxdev_free(o->dEvn);
    afxdev_free(o->dPoint);
    if (o->stream) afxdev_stream_destroy(o->stream);
    free(o->hIndex);
    free(o);
}

/* onset_algorithm.c:405-415, line for line: tests read the pick parameters of the reference from this text */
void onsetObj_debug(OnsetObj o) {
    if (!o) return;
    printf("onsetObj is :\n");
    printf("preMax=%d,postMax=%d, preAvg=%d,postAvg=%d, wait=%d,delta=%f\n", o->preMax, o->postMax, o->preAvg, o->postAvg, o->wait,
           o->delta);
    printf("timeLength=%d,freNum=%d, step=%d,order=%d\n", o->nLength, o->mLength, o->step, o->order);
    printf("\n");
}

int afx_maxFilterDevice(const float *dIn, long long rows, int cols, int order, float *dOut, void *hipStream) {
    if (!dIn || !dOut || dIn == dOut || rows <= 0 || cols <= 0 || order < 1) {
        afxdev_set_error("afx_maxFilterDevice: bad argument (rows %lld, cols %d, order %d, in place: %d)", rows, cols, order,
                         dIn && dIn == dOut);
        return AFX_ERR_ARG;
    }
    int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    return afxk_max_filter(dIn, rows, cols, order, dOut, hipStream);
}

int afx_peakPickDevice(const float *dEvn, int batch, int length, long long stride, int preMax, int postMax, int preAvg,
                       int postAvg, int wait, float delta, int *dPoint, int *dCount, long long pointStride, void *hipStream) {
    if (!dEvn || (!dPoint && !dCount) || batch <= 0 || length <= 0 || stride < length || (dPoint && pointStride < 0)) {
        afxdev_set_error("afx_peakPickDevice: bad argument");
        return AFX_ERR_ARG;
    }
    if (preMax < 0 || preAvg < 0 || wait < 0 || postMax < 1 || postAvg < 1) {
        afxdev_set_error("afx_peakPickDevice: preMax %d, postMax %d, preAvg %d, postAvg %d, wait %d: pre* and wait >= 0, post* >= 1",
                         preMax, postMax, preAvg, postAvg, wait);
        return AFX_ERR_ARG;
    }
    int st = afxdev_bind_stream(hipStream);
    if (st != AFX_OK) return st;
    AfxOnsetPickArgs k;
    memset(&k, 0, sizeof(k));
    k.src = dEvn;
    k.srcStride = stride;
    k.batch = batch;
    k.length = length;
    k.preMax = preMax;
    k.postMax = postMax;
    k.preAvg = preAvg;
    k.postAvg = postAvg;
    k.wait = wait;
    k.delta = delta;
    k.point = dPoint;
    k.count = dCount;
    k.pointStride = pointStride;
    return afxk_onset_pick(&k, hipStream);
}

int afx_powerToDbDevice(const float *dIn, int batch, long long length, long long stride, float min, float *dOut,
                        void *hipStream) {
    if (!dIn || !dOut || batch <= 0 || length <= 0 || stride < length) {
        afxdev_set_error("afx_powerToDbDevice: bad argument");
        return AFX_ERR_ARG;
    }
    if (min >= 0) min = -80; /* flux_util.c:560-562 */
    int st = afxdev_bind_stream(hipStream);
    /* (a launch takes at most 65535 clips) */
    for (int c0 = 0; st == AFX_OK && c0 < batch; c0 += 65535) {
        const int nc = batch - c0 < 65535 ? batch - c0 : 65535;
        st = afxk_power_to_db(dIn + (long long)c0 * stride, nc, length, stride, min, dOut + (long long)c0 * stride, hipStream);
    }
    return st;
}

void util_powerToDB(float *pArr, int length, float min, float *dArr) {
    static const char *who = "util_powerToDB";
    if (!pArr || length <= 0) return; /* (the reference's loops do nothing) */
    float *d = NULL;
    const size_t bytes = sizeof(float) * (size_t)length;
    int st = afxdev_ensure();
    if (st == AFX_OK) st = afxdev_malloc((void **)&d, bytes);
    if (st == AFX_OK) st = afxdev_h2d(d, pArr, bytes, NULL);
    if (st == AFX_OK) st = afx_powerToDbDevice(d, 1, length, length, min, d, NULL);
    if (st == AFX_OK) st = afxdev_d2h(dArr ? dArr : pArr, d, bytes, NULL);
    if (st == AFX_OK) st = afxdev_stream_sync(NULL);
    afxdev_free(d);
    if (st != AFX_OK) afxdev_report_failure(who, st);
}
