/* afx_nsgt.c -- the non-stationary Gabor transform object (C host side) behind include/nsgt_algorithm.h.
 *
 * Parameter handling follows nsgtObj_new (src/nsgt_algorithm.c:72-251), the bank nsgt_filterBank
 * (src/filterbank/nsgt_filterBank.c:48-365), the time map __nsgtObj_dealTime (:253-290) and the search of nsgtObj_nsgt
 * (:585-604), all in the reference's float32 arithmetic: band edges, lengths and the column map are decided by float32
 * comparisons.  The plan is built on the host, without a device (afx_nsgt_plan_host hands it out), then uploaded:
 * lengths, offsets, cell starts, windows, one twiddle table per distinct length, the column map and the launch order.
 * Execution: afxk_nsgt_spectrum + afxk_nsgt_bands (afx_nsgt.hip).
 *
 * Divergences from the reference, both deliberate:
 *   1. a plan with a band longer than 2^radix2Exp is refused (AFX_ERR_UNSUPPORTED) -- the reference writes such a band past
 *      its 2^radix2Exp-entry scratch;
 *   2. nsgtObj_setMinLength rebuilds the time map with the bank -- the reference keeps the arrays of the old lengths and
 *      reads past them.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "afx_batch.h"
#include "afx_device.h"
#include "afx_host.h"
#include "afx_objkit.h"
#include "nsgt_algorithm.h"

typedef struct {
    int num, radix2Exp, samplate, binPerOctave, minLength;
    float lowFre, highFre;
    NSGTFilterBankType bankType;
    SpectralFilterBankScaleType scale;
    SpectralFilterBankStyleType style;
    SpectralFilterBankNormalType normal;
} NsgtParams;

typedef struct {
    /* host */
    int num, maxLength, totalLength, nItems;
    int *len, *offset, *bin;
    float *fre, *window;
    int *colMap;      /* [num][maxLength] */
    float *cellRe, *cellIm; /* [totalLength]: nsgtObj_getCellData */
    /* device */
    AfxNsgtBand *dBands;
    int *dItems, *dColMap, *dCellCol;
    float *dWindow, *dTwiddle;
    float *dOut, *dCell; /* one chunk: [2][num][maxLength], [2][totalLength] */
} NsgtPlan;

struct OpaqueNSGT {
    NsgtParams prm;
    NsgtPlan plan;
    AfxCwtPlanDims dims;
    void *stream;
    float *dTw, *dX, *dA, *dXt;    /* forward twiddles, one chunk's samples / scratch / spectrum */
    float *dGA, *dGXt;             /* scratch of the batched calls: `pass` chunks at a time */
    size_t capGA, capGXt;
    AfxScratchStream scratchStream;
    int status;
};

/* ---- parameters (nsgt_algorithm.c:97-214) ---------------------------------------------------------------------------- */
static int resolve_params(int num, int radix2Exp, int *samplate, float *lowFre, float *highFre, int *binPerOctave,
                          int *minLength, NSGTFilterBankType *bankType, SpectralFilterBankScaleType *scaleType,
                          SpectralFilterBankStyleType *styleType, SpectralFilterBankNormalType *normalType, NsgtParams *p) {
    int sr = 32000, bpo = 12, minLen = 3;
    float low = 0, high = 0;
    NSGTFilterBankType bt = NSGTFilterBank_Efficient;
    SpectralFilterBankScaleType sc = SpectralFilterBankScale_Octave;
    SpectralFilterBankStyleType style = SpectralFilterBankStyle_Hann;
    SpectralFilterBankNormalType normal = SpectralFilterBankNormal_BandWidth;
    if (minLength && *minLength > 0) minLen = *minLength;
    if (radix2Exp && (radix2Exp < 1 || radix2Exp > 30)) {
        printf("radix2Exp is error!\n");
        return -100;
    }
    const long long N = 1LL << radix2Exp;
    if (samplate && *samplate > 0 && *samplate <= 196000) sr = *samplate;
    if (bankType) bt = *bankType;
    if (scaleType) {
        sc = *scaleType;
        if ((int)sc > (int)SpectralFilterBankScale_Log) {
            printf("scaleType is error!\n");
            return 1;
        }
    }
    if (styleType) {
        style = *styleType;
        if (style == SpectralFilterBankStyle_Gammatone) style = SpectralFilterBankStyle_Hann;
    }
    if (normalType) {
        normal = *normalType;
        if (normal == SpectralFilterBankNormal_Area) normal = SpectralFilterBankNormal_BandWidth;
    }
    high = (float)(sr / 2.0);
    if (lowFre && *lowFre >= 0 && *lowFre < sr / 2.0) low = *lowFre;
    const int logLike = (sc == SpectralFilterBankScale_Octave || sc == SpectralFilterBankScale_Log);
    if (low == 0 && logLike) {
        low = (float)(powf(2, (float)(-45 / 12.0)) * 440);
        high = (float)(powf(2, (float)(38 / 12.0)) * 440);
    }
    if (highFre && *highFre > 0 && *highFre <= sr / 2.0) high = *highFre;
    if (high < low) {
        low = 0;
        high = (float)(sr / 2.0);
        if (logLike) {
            low = (float)(powf(2, (float)(-45 / 12.0)) * 440);
            high = (float)(powf(2, (float)(38 / 12.0)) * 440);
        }
    }
    if (binPerOctave && *binPerOctave >= 4 && *binPerOctave <= 48) bpo = *binPerOctave;
    if (sc == SpectralFilterBankScale_Linear) {
        const float det = sr / (float)N;
        afx_auditory_revise_linear(num, low, high, det, 1, &low, &high);
        if (high > sr / 2.0) {
            printf("scale linear: lowFre and num is large, overflow error\n");
            return -1;
        }
    } else if (sc == SpectralFilterBankScale_Octave) {
        afx_auditory_revise_log(num, low, high, bpo, 1, &low, &high);
        if (high > sr / 2.0) {
            printf("scale log: lowFre and num is large, overflow error!\n");
            return -1;
        }
    }
    if (num < 2 || num > N / 2 + 1) {
        printf("num is error!\n");
        return -1;
    }
    p->num = num;
    p->radix2Exp = radix2Exp;
    p->samplate = sr;
    p->binPerOctave = bpo;
    p->minLength = minLen;
    p->lowFre = low;
    p->highFre = high;
    p->bankType = bt;
    p->scale = sc;
    p->style = style;
    p->normal = normal;
    return 0;
}

/* ---- the host plan ----------------------------------------------------------------------------------------------------- */
static void plan_free_host(NsgtPlan *pl) {
    free(pl->len);
    free(pl->offset);
    free(pl->bin);
    free(pl->fre);
    free(pl->window);
    free(pl->colMap);
    free(pl->cellRe);
    free(pl->cellIm);
    pl->len = pl->offset = pl->bin = pl->colMap = NULL;
    pl->fre = pl->window = pl->cellRe = pl->cellIm = NULL;
}

static float *band_window(SpectralFilterBankStyleType style, int len, int periodic) {
    WindowType wt;
    switch (style) { /* nsgt_filterBank.c:265-294, :325-354 */
        case SpectralFilterBankStyle_Slaney: wt = Window_Triang; break;
        case SpectralFilterBankStyle_ETSI: wt = Window_Bartlett; break;
        case SpectralFilterBankStyle_Hann: wt = Window_Hann; break;
        case SpectralFilterBankStyle_Hamm: wt = Window_Hamm; break;
        case SpectralFilterBankStyle_Blackman: wt = Window_Blackman; break;
        case SpectralFilterBankStyle_Bohman: wt = Window_Bohman; break;
        case SpectralFilterBankStyle_Kaiser: wt = Window_Kaiser; break;
        case SpectralFilterBankStyle_Gauss: wt = Window_Gauss; break;
        default: wt = Window_Rect; break;
    }
    return afx_window_create(wt, len, periodic);
}

/* lengths, offsets, bins, frequencies, windows (nsgt_filterBank.c:48-365) and the column map (nsgt_algorithm.c:253-290,
 * :585-604); 0, AFX_ERR_NOMEM or AFX_ERR_UNSUPPORTED (with a message) */
static int plan_build_host(const NsgtParams *p, NsgtPlan *pl) {
    const int num = p->num, sr = p->samplate;
    const long long N = 1LL << p->radix2Exp;
    memset(pl, 0, sizeof(*pl));
    if (p->radix2Exp > 24) {
        afxdev_set_error("nsgt: chunks of 2^%d samples are not supported (at most 2^24 here, 2^20 on the device)", p->radix2Exp);
        return AFX_ERR_UNSUPPORTED;
    }
    int count = 0;
    float *f = afx_auditory_edges(num, (int)N, sr, p->scale, p->lowFre, p->highFre, p->binPerOctave, 0, &count);
    int *b = (int *)calloc((size_t)num + 2, sizeof(int));
    pl->num = num;
    pl->len = (int *)calloc((size_t)num, sizeof(int));
    pl->offset = (int *)calloc((size_t)num, sizeof(int));
    pl->bin = (int *)calloc((size_t)num, sizeof(int));
    pl->fre = (float *)calloc((size_t)num, sizeof(float));
    int st = (f && b && pl->len && pl->offset && pl->bin && pl->fre && count == num + 2) ? AFX_OK : AFX_ERR_NOMEM;
    long long total = 0;
    int maxLen = 0;
    if (st == AFX_OK) {
        for (int i = 0; i < num + 2; i++) b[i] = (int)roundf(N * f[i] / sr);
        for (int i = 0; i < num && st == AFX_OK; i++) {
            const long long left = b[i], cur = b[i + 1], right = b[i + 2];
            long long len;
            if (p->bankType == NSGTFilterBank_Standard) {
                len = right - left + 1;
            } else if (right - left >= 1) {
                const long long v1 = cur - left, v2 = right - cur;
                len = 2 * (v2 >= v1 ? v2 : v1) + 1;
            } else {
                len = 0;
            }
            if (len < p->minLength) len = p->minLength;
            if (len > N) { /* divergence 1: the reference overruns its scratch here */
                afxdev_set_error("nsgt: band %d would be %lld bins long, more than the 2^%d of a chunk", i, len, p->radix2Exp);
                st = AFX_ERR_UNSUPPORTED;
                break;
            }
            pl->len[i] = (int)len;
            long long off = cur - len / 2;
            pl->offset[i] = off < 0 ? 0 : (int)off;
            pl->bin[i] = b[i + 1];
            pl->fre[i] = f[i + 1];
            total += len;
            if (len > maxLen) maxLen = (int)len;
        }
    }
    if (st == AFX_OK && (total > (1LL << 28) || (long long)num * maxLen > (1LL << 28))) {
        afxdev_set_error("nsgt: %lld cells / %lld matrix elements per chunk exceed the supported 2^28", total, (long long)num * maxLen);
        st = AFX_ERR_UNSUPPORTED;
    }
    free(f);
    free(b);
    if (st == AFX_OK) {
        pl->maxLength = maxLen;
        pl->totalLength = (int)total;
        pl->window = (float *)calloc((size_t)total, sizeof(float));
        pl->colMap = (int *)calloc((size_t)num * maxLen, sizeof(int));
        pl->cellRe = (float *)calloc((size_t)total, sizeof(float));
        pl->cellIm = (float *)calloc((size_t)total, sizeof(float));
        if (!pl->window || !pl->colMap || !pl->cellRe || !pl->cellIm) st = AFX_ERR_NOMEM;
    }
    /* windows: symmetric (efficient) or periodic (standard), over sqrtf(len) under BandWidth */
    size_t at = 0;
    for (int i = 0; i < num && st == AFX_OK; i++) {
        const int len = pl->len[i];
        float *w = band_window(p->style, len, p->bankType == NSGTFilterBank_Standard);
        if (!w) {
            st = AFX_ERR_NOMEM;
            break;
        }
        if (p->normal == SpectralFilterBankNormal_BandWidth) {
            const float d = sqrtf((float)len);
            for (int j = 0; j < len; j++) w[j] = w[j] / d;
        }
        memcpy(pl->window + at, w, sizeof(float) * (size_t)len);
        at += (size_t)len;
        free(w);
    }
    /* column j of row i holds cell k - 1, k the first index >= the row's running start with maxTime[j] < time_i[k] */
    if (st == AFX_OK) {
        const float time = N / (float)sr;
        float *maxTime = afx_linspace(0, time, maxLen + 1, 0);
        if (!maxTime) st = AFX_ERR_NOMEM;
        for (int i = 0; i < num && st == AFX_OK; i++) {
            const float curLen = (float)pl->len[i];
            const float det = (curLen - 2 >= 0 ? curLen - 2 : 0);
            const float offset = time / (curLen + det);
            float *t = afx_linspace(-offset, time + offset, pl->len[i] + 1, 0);
            if (!t) {
                st = AFX_ERR_NOMEM;
                break;
            }
            int start = 0, *row = pl->colMap + (size_t)i * maxLen;
            for (int j = 0; j < maxLen; j++) {
                int k = start;
                while (k < pl->len[i] + 1 && !(maxTime[j] < t[k])) k++;
                if (k > pl->len[i]) k = pl->len[i]; /* (no entry is greater: the reference would leave the column unwritten) */
                else start = k;
                row[j] = k > 0 ? k - 1 : 0;
            }
            free(t);
        }
        free(maxTime);
    }
    if (st != AFX_OK) plan_free_host(pl);
    return st;
}

int afx_nsgt_plan_host(int num, int radix2Exp, int *samplate, float *lowFre, float *highFre, int *binPerOctave,
                       int *minLength, NSGTFilterBankType *nsgtFilterBankType,
                       SpectralFilterBankScaleType *filterScaleType, SpectralFilterBankStyleType *filterStyleType,
                       SpectralFilterBankNormalType *filterNormalType, int *lengthArr, int *offsetArr, int *binArr,
                       float *freArr, float *windowArr, int *maxLength, int *totalLength, int *colMapArr) {
    NsgtParams p;
    NsgtPlan pl;
    int st = resolve_params(num, radix2Exp, samplate, lowFre, highFre, binPerOctave, minLength, nsgtFilterBankType,
                            filterScaleType, filterStyleType, filterNormalType, &p);
    if (st != 0) return st;
    st = plan_build_host(&p, &pl);
    if (st != AFX_OK) return st;
    if (lengthArr) memcpy(lengthArr, pl.len, sizeof(int) * (size_t)num);
    if (offsetArr) memcpy(offsetArr, pl.offset, sizeof(int) * (size_t)num);
    if (binArr) memcpy(binArr, pl.bin, sizeof(int) * (size_t)num);
    if (freArr) memcpy(freArr, pl.fre, sizeof(float) * (size_t)num);
    if (windowArr) memcpy(windowArr, pl.window, sizeof(float) * (size_t)pl.totalLength);
    if (colMapArr) memcpy(colMapArr, pl.colMap, sizeof(int) * (size_t)num * pl.maxLength);
    if (maxLength) *maxLength = pl.maxLength;
    if (totalLength) *totalLength = pl.totalLength;
    plan_free_host(&pl);
    return 0;
}

/* ---- the device plan --------------------------------------------------------------------------------------------------- */
static void plan_free(NsgtPlan *pl) {
    afxdev_free(pl->dBands);
    afxdev_free(pl->dItems);
    afxdev_free(pl->dColMap);
    afxdev_free(pl->dCellCol);
    afxdev_free(pl->dWindow);
    afxdev_free(pl->dTwiddle);
    afxdev_free(pl->dOut);
    afxdev_free(pl->dCell);
    plan_free_host(pl);
    memset(pl, 0, sizeof(*pl));
}

typedef struct {
    int len, band;
} LenBand;

static int len_band_cmp(const void *a, const void *b) {
    const LenBand *x = (const LenBand *)a, *y = (const LenBand *)b;
    if (x->len != y->len) return y->len - x->len; /* longest first */
    return x->band - y->band;
}

static int up(void **d, const void *h, size_t bytes, void *stream) {
    int st = afxdev_malloc(d, bytes);
    if (st == AFX_OK) st = afxdev_h2d(*d, h, bytes, stream);
    return st;
}

/* band table, twiddle tables (one per distinct length, double -> float32), cell -> first column table, launch order */
static int plan_upload(NsgtPlan *pl, void *stream) {
    const int num = pl->num, maxLen = pl->maxLength;
    AfxNsgtBand *bands = (AfxNsgtBand *)calloc((size_t)num, sizeof(AfxNsgtBand));
    LenBand *order = (LenBand *)calloc((size_t)num, sizeof(LenBand));
    int *cellCol = (int *)calloc((size_t)pl->totalLength + num, sizeof(int));
    int st = (bands && order && cellCol) ? AFX_OK : AFX_ERR_NOMEM;
    float *tw = NULL;
    int *items = NULL;
    long long twFloat2 = 0, nItems = 0;
    if (st == AFX_OK) {
        int cell = 0;
        for (int i = 0; i < num; i++) {
            bands[i].len = pl->len[i];
            bands[i].offset = pl->offset[i];
            bands[i].cell = cell;
            bands[i].cellCol = cell + i;
            /* entry n: the first column whose cell index is >= n (the map is monotone along a row) */
            const int *row = pl->colMap + (size_t)i * maxLen;
            int *cc = cellCol + bands[i].cellCol, j = 0;
            for (int n = 0; n <= pl->len[i]; n++) {
                while (j < maxLen && row[j] < n) j++;
                cc[n] = j;
            }
            cc[pl->len[i]] = maxLen;
            cell += pl->len[i];
            order[i].len = pl->len[i];
            order[i].band = i;
            nItems += (pl->len[i] + AFX_NSGT_BLOCK - 1) / AFX_NSGT_BLOCK;
        }
        qsort(order, (size_t)num, sizeof(LenBand), len_band_cmp);
        for (int q = 0; q < num; q++) { /* equal lengths are neighbours now: one table each */
            if (q > 0 && order[q].len == order[q - 1].len) {
                bands[order[q].band].twiddle = bands[order[q - 1].band].twiddle;
            } else {
                bands[order[q].band].twiddle = (int)twFloat2;
                twFloat2 += order[q].len;
            }
        }
        tw = (float *)malloc(sizeof(float) * 2 * (size_t)twFloat2);
        items = (int *)malloc(sizeof(int) * 2 * (size_t)nItems);
        if (!tw || !items) st = AFX_ERR_NOMEM;
    }
    if (st == AFX_OK) {
        long long it = 0;
        for (int q = 0; q < num; q++) {
            const int L = order[q].len, band = order[q].band;
            if (q == 0 || L != order[q - 1].len) {
                float *t = tw + 2 * (size_t)bands[band].twiddle;
                for (int m = 0; m < L; m++) {
                    t[2 * m] = (float)cos(2.0 * M_PI * m / L);
                    t[2 * m + 1] = (float)sin(2.0 * M_PI * m / L);
                }
            }
            for (int n0 = 0; n0 < L; n0 += AFX_NSGT_BLOCK, it++) {
                items[2 * it] = band;
                items[2 * it + 1] = n0;
            }
        }
        pl->nItems = (int)nItems;
    }
    if (st == AFX_OK) st = up((void **)&pl->dBands, bands, sizeof(AfxNsgtBand) * (size_t)num, stream);
    if (st == AFX_OK) st = up((void **)&pl->dItems, items, sizeof(int) * 2 * (size_t)nItems, stream);
    if (st == AFX_OK) st = up((void **)&pl->dColMap, pl->colMap, sizeof(int) * (size_t)num * maxLen, stream);
    if (st == AFX_OK) st = up((void **)&pl->dCellCol, cellCol, sizeof(int) * ((size_t)pl->totalLength + num), stream);
    if (st == AFX_OK) st = up((void **)&pl->dWindow, pl->window, sizeof(float) * (size_t)pl->totalLength, stream);
    if (st == AFX_OK) st = up((void **)&pl->dTwiddle, tw, sizeof(float) * 2 * (size_t)twFloat2, stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&pl->dOut, sizeof(float) * 2 * (size_t)num * maxLen);
    if (st == AFX_OK) st = afxdev_malloc((void **)&pl->dCell, sizeof(float) * 2 * (size_t)pl->totalLength);
    if (st == AFX_OK) st = afxdev_stream_sync(stream);
    free(bands);
    free(order);
    free(cellCol);
    free(tw);
    free(items);
    return st;
}

static void fill_args(NSGTObj o, const float *Xt, int chunks, float *outRe, float *outIm, float *cellRe, float *cellIm,
                      AfxNsgtArgs *a) {
    const NsgtPlan *pl = &o->plan;
    memset(a, 0, sizeof(*a));
    a->r1 = o->dims.r1;
    a->r2 = o->dims.r2;
    a->num = pl->num;
    a->maxLength = pl->maxLength;
    a->totalLength = pl->totalLength;
    a->bands = pl->dBands;
    a->items = pl->dItems;
    a->nItems = pl->nItems;
    a->window = pl->dWindow;
    a->twiddle = pl->dTwiddle;
    a->colMap = pl->dColMap;
    a->cellCol = pl->dCellCol;
    a->Xt = Xt;
    a->chunks = chunks;
    a->outRe = outRe;
    a->outIm = outIm;
    a->cellRe = cellRe;
    a->cellIm = cellIm;
}

/* ---- the object -------------------------------------------------------------------------------------------------------- */
int nsgtObj_new(NSGTObj *nsgtObj, int num, int radix2Exp, int *samplate, float *lowFre, float *highFre,
                int *binPerOctave, int *minLength, NSGTFilterBankType *nsgtFilterBankType,
                SpectralFilterBankScaleType *filterScaleType, SpectralFilterBankStyleType *filterStyleType,
                SpectralFilterBankNormalType *filterNormalType) {
    if (!nsgtObj) return -1;
    *nsgtObj = NULL;
    NsgtParams p;
    int st = resolve_params(num, radix2Exp, samplate, lowFre, highFre, binPerOctave, minLength, nsgtFilterBankType,
                            filterScaleType, filterStyleType, filterNormalType, &p);
    if (st != 0) return st;
    /* the forward pass (afx_cwt.hip) factors N = 2^r1 2^r2, r1 = r / 2, with column tiles of <= 64 KB of LDS; checked
     * here on 2^8 ... 2^17 -- lengths outside 2^4 ... 2^20 are refused rather than left untried */
    if (radix2Exp < 4 || radix2Exp > 20) {
        afxdev_set_error("nsgtObj_new: chunks of 2^%d samples are not supported (2^4 ... 2^20)", radix2Exp);
        return AFX_ERR_UNSUPPORTED;
    }
    NSGTObj o = (NSGTObj)calloc(1, sizeof(struct OpaqueNSGT));
    if (!o) return AFX_ERR_NOMEM;
    o->prm = p;
    st = plan_build_host(&p, &o->plan); /* (before the device: a refused plan is refused without one) */
    if (st == AFX_OK) st = afxdev_ensure();
    const size_t N = (size_t)1 << radix2Exp;
    float *tw = NULL;
    if (st == AFX_OK) {
        o->dims.r1 = radix2Exp / 2;
        o->dims.r2 = radix2Exp - radix2Exp / 2;
        o->dims.dataLength = (int)N;
        o->dims.pad = 0;
        int c = 8192 >> o->dims.r1; /* <= 64 KB of LDS per column tile (afx_cwt.c) */
        if (c > 16) c = 16;
        if (c > (1 << o->dims.r2)) c = 1 << o->dims.r2;
        if (c < 1) c = 1;
        o->dims.tileCols = c;
        tw = afx_twiddle_table((int)N);
        if (!tw) st = AFX_ERR_NOMEM;
    }
    if (st == AFX_OK) st = afxdev_stream_create(&o->stream);
    if (st == AFX_OK) st = up((void **)&o->dTw, tw, sizeof(float) * N, o->stream);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dX, sizeof(float) * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dA, sizeof(float) * 2 * N);
    if (st == AFX_OK) st = afxdev_malloc((void **)&o->dXt, sizeof(float) * 2 * N);
    if (st == AFX_OK) st = plan_upload(&o->plan, o->stream);
    free(tw);
    if (st != AFX_OK) {
        nsgtObj_free(o);
        return st;
    }
    *nsgtObj = o;
    return 0;
}

void nsgtObj_setMinLength(NSGTObj o, int minLength) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("nsgtObj_setMinLength: NULL object");
        return;
    }
    if (minLength == o->prm.minLength || minLength < 1) return;
    NsgtParams p = o->prm;
    NsgtPlan pl;
    p.minLength = minLength;
    int st = plan_build_host(&p, &pl);
    if (st == AFX_OK) {
        st = plan_upload(&pl, o->stream);
        if (st != AFX_OK) plan_free(&pl);
    }
    if (st != AFX_OK) { /* the object stays as it was */
        AFX_FAIL(o, st, "nsgtObj_setMinLength");
        return;
    }
    afxdev_stream_sync(o->stream);
    afx_scratch_drain(&o->scratchStream); /* a caller's stream may still read the old plan */
    plan_free(&o->plan);
    o->plan = pl;
    o->prm = p;
}

static int batch_device(NSGTObj o, const float *dData, int chunks, long long chunkStride, float *dReal, float *dImag,
                        float *dCellReal, float *dCellImag, void *hipStream, const char *who) {
    const size_t N = (size_t)o->dims.dataLength;
    int st = afx_scratch_wait(&o->scratchStream, hipStream);
    /* spectra of a pass: at most 128 MB each for the scratch and the result, and a launch takes 65535 chunks */
    long long pass = (long long)((128u << 20) / (8 * N));
    if (pass < 1) pass = 1;
    if (pass > 65535) pass = 65535;
    if (pass > chunks) pass = chunks;
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dGA, &o->capGA, sizeof(float) * 2 * N * (size_t)pass);
    if (st == AFX_OK) st = afxdev_reserve((void **)&o->dGXt, &o->capGXt, sizeof(float) * 2 * N * (size_t)pass);
    const size_t plane = (size_t)o->plan.num * o->plan.maxLength, cells = (size_t)o->plan.totalLength;
    for (long long c = 0; c < chunks && st == AFX_OK; c += pass) {
        const int n = (int)(chunks - c < pass ? chunks - c : pass);
        st = afxk_nsgt_spectrum(&o->dims, o->dTw, dData + c * chunkStride, chunkStride, n, o->dGA, o->dGXt, hipStream);
        if (st == AFX_OK) {
            AfxNsgtArgs a;
            fill_args(o, o->dGXt, n, dReal + (size_t)c * plane, dImag + (size_t)c * plane,
                      dCellReal ? dCellReal + (size_t)c * cells : NULL, dCellImag ? dCellImag + (size_t)c * cells : NULL, &a);
            st = afxk_nsgt_bands(&a, hipStream);
        }
    }
    afx_scratch_mark(&o->scratchStream, hipStream);
    if (st != AFX_OK) AFX_FAIL(o, st, who);
    return st;
}

int nsgtObj_nsgtBatchDevice(NSGTObj o, const float *dData, int chunks, long long chunkStride, float *dReal,
                            float *dImag, float *dCellReal, float *dCellImag, void *hipStream) {
    AFX_ENTER(o);
    if (!o || !dData || !dReal || !dImag || (dCellReal == NULL) != (dCellImag == NULL) || chunks <= 0 ||
        chunkStride < o->dims.dataLength) {
        afxdev_set_error("nsgtObj_nsgtBatchDevice: bad argument");
        return AFX_ERR_ARG;
    }
    if (hipStream) { /* the plan lives on the object's device */
        const int dev = afxdev_current_device();
        int st = afxdev_bind_stream(hipStream);
        if (st == AFX_OK && afxdev_current_device() != dev) {
            (void)afxdev_bind_stream(o->stream);
            afxdev_set_error("nsgtObj_nsgtBatchDevice: the stream belongs to another device than the object");
            st = AFX_ERR_ARG;
        }
        if (st != AFX_OK) return st;
    }
    return batch_device(o, dData, chunks, chunkStride, dReal, dImag, dCellReal, dCellImag, hipStream,
                        "nsgtObj_nsgtBatchDevice");
}

void nsgtObj_nsgt(NSGTObj o, float *dataArr, float *mRealArr3, float *mImageArr3) {
    AFX_ENTER(o);
    if (!o) {
        afxdev_set_error("nsgtObj_nsgt: NULL object");
        return;
    }
    if (!dataArr || !mRealArr3 || !mImageArr3) {
        afxdev_set_error("nsgtObj_nsgt: NULL array");
        AFX_FAIL(o, AFX_ERR_ARG, "nsgtObj_nsgt");
        return;
    }
    NsgtPlan *pl = &o->plan;
    const size_t N = (size_t)o->dims.dataLength, plane = (size_t)pl->num * pl->maxLength, cells = (size_t)pl->totalLength;
    int st = afxdev_h2d(o->dX, dataArr, sizeof(float) * N, o->stream);
    if (st == AFX_OK) st = afxk_nsgt_spectrum(&o->dims, o->dTw, o->dX, (long long)N, 1, o->dA, o->dXt, o->stream);
    if (st == AFX_OK) {
        AfxNsgtArgs a;
        fill_args(o, o->dXt, 1, pl->dOut, pl->dOut + plane, pl->dCell, pl->dCell + cells, &a);
        st = afxk_nsgt_bands(&a, o->stream);
    }
    if (st == AFX_OK) st = afxdev_d2h(mRealArr3, pl->dOut, sizeof(float) * plane, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(mImageArr3, pl->dOut + plane, sizeof(float) * plane, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(pl->cellRe, pl->dCell, sizeof(float) * cells, o->stream);
    if (st == AFX_OK) st = afxdev_d2h(pl->cellIm, pl->dCell + cells, sizeof(float) * cells, o->stream);
    if (st == AFX_OK) st = afxdev_stream_sync(o->stream);
    if (st != AFX_OK) AFX_FAIL(o, st, "nsgtObj_nsgt");
}

void nsgtObj_getCellData(NSGTObj o, float **realArr3, float **imageArr3) {
    if (!o) {
        afxdev_set_error("nsgtObj_getCellData: NULL object");
        if (realArr3) *realArr3 = NULL;
        if (imageArr3) *imageArr3 = NULL;
        return;
    }
    if (realArr3) *realArr3 = o->plan.cellRe;
    if (imageArr3) *imageArr3 = o->plan.cellIm;
}

int nsgtObj_getMaxTimeLength(NSGTObj o) { return o ? o->plan.maxLength : 0; }
int nsgtObj_getTotalTimeLength(NSGTObj o) { return o ? o->plan.totalLength : 0; }
int *nsgtObj_getTimeLengthArr(NSGTObj o) { return o ? o->plan.len : NULL; }
float *nsgtObj_getFreBandArr(NSGTObj o) { return o ? o->plan.fre : NULL; }
int *nsgtObj_getBinBandArr(NSGTObj o) { return o ? o->plan.bin : NULL; }

void nsgtObj_free(NSGTObj o) {
    if (!o) return;
    if (o->stream) {
        (void)afxdev_bind_stream(o->stream);
        afxdev_stream_sync(o->stream);
    }
    afx_scratch_drain(&o->scratchStream); /* the caller's stream may still run our kernels */
    plan_free(&o->plan);
    afxdev_free(o->dTw);
    afxdev_free(o->dX);
    afxdev_free(o->dA);
    afxdev_free(o->dXt);
    afxdev_free(o->dGA);
    afxdev_free(o->dGXt);
    afxdev_stream_destroy(o->stream);
    free(o);
}
