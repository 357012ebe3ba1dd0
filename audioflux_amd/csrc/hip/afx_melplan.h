// afx_melplan.h -- the host side the four fused STFT -> filter-bank translation units share with their dispatcher
// (afx_melfused.hip): the plan, what a transform size contributes to it, and the frame distribution of their launchers.
#ifndef AFX_MELPLAN_H
#define AFX_MELPLAN_H

#include "afx_hipcheck.h"

// One plan for every size.  dTab is the size's table blob as the kernel copies it to LDS: the transform's tables (window
// included), then at byte offset AfxMelSize.bandOff the band weights per lane, [64][tapsA + tapsB + 4] floats, A taps then B
// taps of the variant; dMeta is startA | startB | rowA | rowB | segIdx[0..63] | segIdx[64..127] of the band plan, [6][64].
struct AfxMelPlan {
    int radix2Exp;  // the size: 9 .. 12
    int variant;    // index into the size's tap table
    int num;
    int split;      // slots hold row segments (AfxBandPlan.split)
    int pack;       // 0, or 1 + index into the size's packed layouts: the band block is [64][a + b + c + 4] floats, one stream of
                    // three partitions per lane, and dMeta is [8][64]: base a / b / c | row a / b / c | b continues a | c continues b
    float *dTab;
    int *dMeta;
};

struct AfxMelVariant {
    int tapsA, tapsB;
};

// What a transform size contributes (one per afx_melfused{512,1k,2,4k2}.hip)
struct AfxMelSize {
    int radix2Exp;
    int kindBase;  // afxk_melfused_kind: kindBase + 1 (whole rows) / + 2 (split plan)
    const AfxMelVariant *variants;  // ordered by cost
    int numVariants;
    int bandOff;  // bytes of the transform's tables in the blob = offset of the band weights
    void (*fill)(float *tab, const float *hWindow);  // the transform's tables at their byte offsets (hWindow == nullptr: no window)
    int (*run)(const AfxMelPlan *p, const AfxMelFusedArgs *a, void *stream);  // argument checks common to all sizes are done
    // packed plans (afx_bandpack.h), for banks that run variant 0 in whole rows: the layouts (a, b, c) the size's kernel is
    // compiled for (none: nullptr, 0) and the floats of its zero-padded power row
    const int (*packs)[3];
    int numPacks;
    int rowCap;
};
const AfxMelSize *afx_mel_size512(), *afx_mel_size1k(), *afx_mel_size2k(), *afx_mel_size4k();

// AfxMelPlan.pack of a plan from afxk_melfused_create (0: not packed, or no plan); beside afxk_melfused_kind, which does not tell.
// Declared here, not in afx_device.h: nothing on the host side calls it.  (tests/emu/mel_pack_emulated_case.py and
// tests/test_mel_pack_gpu.py mirror AfxMelPlan with ctypes to reach dMeta: a change of the struct goes there too.)
extern "C" int afxk_melfused_pack(const void *plan);

// frames per wave and workgroups of a launch with `waves` waves per workgroup: two rounds of workgroups (afx_frame_split, afx_device.h)
static inline long long afx_mel_frames(long long total, int waves, long long *framesPerWave) {
    return afx_frame_split(total, afx_cu_count(), waves, 2, framesPerWave);
}

#endif /* AFX_MELPLAN_H */
