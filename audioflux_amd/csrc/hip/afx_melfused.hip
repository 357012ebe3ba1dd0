// afx_melfused.hip -- fused STFT -> filter bank, one 64-lane wave per frame: the ONE host plan layer of the four transform
// sizes.  Plan, band-plan packing, create / destroy, plan kinds and the size-independent argument checks live here; a size
// contributes an AfxMelSize (afx_melplan.h): its tap variants, its table-fill function and its launchers -- n_fft 512
// afx_melfused512.hip, 1024 afx_melfused1k.hip, 2048 afx_melfused2.hip (real AND complex results: bftObj_setResultType(0), the
// reference wrapper's default, bft_algorithm.c:457-485), 4096 afx_melfused4k2.hip.  The device pieces the four kernels share
// are in afx_melparts.h.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "afx_melplan.h"
#include "afx_bandpack.h"

namespace {

const AfxMelSize *size_of(int radix2Exp) {
    switch (radix2Exp) {
        case 9: return afx_mel_size512();
        case 10: return afx_mel_size1k();
        case 11: return afx_mel_size2k();
        case 12: return afx_mel_size4k();
        default: return nullptr;
    }
}

// AfxBandPlan -> the lane-weight block wL [64][WP] (A taps, then at TA the B taps of variant (TA, TB)) and meta[384]
void pack_band(const AfxBandPlan *band, int TA, int WP, float *wL, int *meta) {
    for (int l = 0; l < 64; ++l) {
        for (int t = 0; t < band->tapsA; ++t) wL[(size_t)l * WP + t] = band->wA[(size_t)t * 64 + l];
        for (int t = 0; t < band->tapsB; ++t) wL[(size_t)l * WP + TA + t] = band->wB[(size_t)t * 64 + l];
        meta[l] = band->startA[l];
        meta[64 + l] = band->startB[l];
        meta[128 + l] = band->rowA[l];
        meta[192 + l] = band->rowB[l];
        meta[256 + l] = (int)band->segIdx[l];
        meta[320 + l] = (int)band->segIdx[64 + l];
    }
}

// AfxBandPack -> the lane-weight block wL [64][WP] (the lane's stream a | b | c) and meta[512]
void pack_band3(const AfxBandPack *pk, int WP, float *wL, int *meta) {
    for (int l = 0; l < 64; ++l) {
        for (int t = 0; t < pk->slots; ++t) wL[(size_t)l * WP + t] = pk->w[(size_t)t * 64 + l];
        for (int q = 0; q < 3; ++q) {
            meta[64 * q + l] = pk->base[q][l];
            meta[192 + 64 * q + l] = pk->row[q][l];
        }
        meta[384 + l] = pk->cont[1][l];
        meta[448 + l] = pk->cont[2][l];
    }
}

}  // namespace

extern "C" int afxk_melfused_pack(const void *plan) { return plan ? static_cast<const AfxMelPlan *>(plan)->pack : 0; }

extern "C" int afxk_melfused_variant(int radix2Exp, int tapsA, int tapsB) {
    const AfxMelSize *s = size_of(radix2Exp);
    if (afxdev_no_fused() || !s) return -1;
    for (int i = 0; i < s->numVariants; ++i)
        if (tapsA <= s->variants[i].tapsA && tapsB <= s->variants[i].tapsB) return i;
    return -1;
}

extern "C" int afxk_melfused_kind(const void *plan) {
    const AfxMelPlan *p = static_cast<const AfxMelPlan *>(plan);
    return !p ? 0 : size_of(p->radix2Exp)->kindBase + (p->split ? 2 : 1);
}

extern "C" void afxk_melfused_destroy(void *plan) {
    AfxMelPlan *p = static_cast<AfxMelPlan *>(plan);
    if (!p) return;
    afxdev_free(p->dTab);
    afxdev_free(p->dMeta);
    free(p);
}

extern "C" int afxk_melfused_create(void **plan, int radix2Exp, const float *hWindow,
                                    const AfxBandPlan *band, void *stream) {
    *plan = nullptr;
    const int variant = afxk_melfused_variant(radix2Exp, band->tapsA, band->tapsB);
    if (variant < 0) return AFX_ERR_UNSUPPORTED;
    const AfxMelSize *s = size_of(radix2Exp);
    const int TA = s->variants[variant].tapsA, TB = s->variants[variant].tapsB;
    // a whole-row plan of the cheapest variant is re-packed where the size's kernel has a packed form that runs fewer tap slots
    // (afx_bandpack_build declines otherwise); AFX_MEL_NOPACK=1, read here, keeps the plan as it came
    AfxBandPack pk = {};
    int pack = 0;
    const char *nopack = getenv("AFX_MEL_NOPACK");
    if (s->numPacks > 0 && variant == 0 && !(nopack && atoi(nopack) != 0) &&
        afx_bandpack_build(band, s->packs, s->numPacks, s->rowCap, TA + TB, &pk) == 0) {
        for (int i = 0; i < s->numPacks; ++i)
            if (s->packs[i][0] == pk.taps[0] && s->packs[i][1] == pk.taps[1] && s->packs[i][2] == pk.taps[2]) pack = i + 1;
        if (!pack) afx_bandpack_free(&pk);  // (a layout that is not the size's: the planner returns only what it was given)
    }
    const int WP = (pack ? pk.slots : TA + TB) + 4;
    const size_t bytes = (size_t)s->bandOff + (size_t)64 * WP * 4;
    AfxMelPlan *p = static_cast<AfxMelPlan *>(calloc(1, sizeof(AfxMelPlan)));
    float *tab = static_cast<float *>(calloc(bytes, 1));
    if (!p || !tab) {
        free(p);
        free(tab);
        if (pack) afx_bandpack_free(&pk);
        return AFX_ERR_NOMEM;
    }
    p->radix2Exp = radix2Exp;
    p->variant = variant;
    p->num = band->num;
    p->split = band->split;
    p->pack = pack;
    s->fill(tab, hWindow);
    int meta[512];
    const size_t metaBytes = (pack ? 512 : 384) * sizeof(int);
    if (pack) {
        pack_band3(&pk, WP, tab + s->bandOff / 4, meta);
        afx_bandpack_free(&pk);
    } else {
        pack_band(band, TA, WP, tab + s->bandOff / 4, meta);
    }
    int st = afxdev_malloc(reinterpret_cast<void **>(&p->dTab), bytes);
    if (st == AFX_OK) st = afxdev_h2d(p->dTab, tab, bytes, stream);
    if (st == AFX_OK) st = afxdev_malloc(reinterpret_cast<void **>(&p->dMeta), metaBytes);
    if (st == AFX_OK) st = afxdev_h2d(p->dMeta, meta, metaBytes, stream);
    if (st == AFX_OK) st = afxdev_stream_sync(stream);  // host staging buffers are freed below
    free(tab);
    if (st != AFX_OK) {
        afxk_melfused_destroy(p);
        return st;
    }
    *plan = p;
    return AFX_OK;
}

// specMap 0 / 1 / 2: real results, 3 / 4: complex results (out + outIm); AFX_ERR_UNSUPPORTED when the requested fusion
// (cepstra / temporal features) does not apply to this plan
extern "C" int afxk_melfused_run(void *plan, const AfxMelFusedArgs *a, void *stream) {
    const AfxMelPlan *p = static_cast<const AfxMelPlan *>(plan);
    if (!p) return AFX_ERR_ARG;
    if (a->energy && p->radix2Exp != 11) return AFX_ERR_UNSUPPORTED;  // temporal features ride along at n_fft 2048 only (cepstra: every size)
    if (a->specMap > 4) return AFX_ERR_ARG;
    return size_of(p->radix2Exp)->run(p, a, stream);
}
