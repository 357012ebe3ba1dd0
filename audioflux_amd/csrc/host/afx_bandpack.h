/* afx_bandpack.h -- the packed band plan (afx_bandplan.c: afx_bandpack_build), shared by the host planner, the plan layer
 * of the fused kernels (afx_melfused.hip) and the tests, which mirror AfxBandPack with ctypes. */
#ifndef AFX_BANDPACK_H
#define AFX_BANDPACK_H

#include "afx_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every lane runs the same tap stream of three partitions, taps[0] | taps[1] | taps[2] (each a multiple of 4); per lane a
 * partition either continues the row of the partition before it or starts a new row at a power-row address of its own.
 * A lane therefore carries one row (a+b+c), two ((a+b | c) or (a | b+c)) or three (a | b | c); as many lanes carry three
 * as carry one, so 64 lanes hold up to 128 rows. */
typedef struct {
    int num;          /* bank rows                                                              */
    int taps[3];      /* the partitions a, b, c                                                 */
    int slots;        /* a + b + c: tap slots every lane runs                                   */
    int conflicts;    /* lane pairs of a 32-lane half that meet on an LDS bank pair within one  */
                      /* partition's power-row reads (0: every read is conflict-free)           */
    int base[3][64];  /* power-row bin of the partition's first slot (even)                     */
    int row[3][64];   /* bank row whose last partition this is: stored from here (-1: none)     */
    int cont[3][64];  /* 1: the partition continues the row of the one before (cont[0] = 0)     */
    float *w;         /* host, [slots][64], tap-major, zero padded                              */
} AfxBandPack;

/* Re-packs a whole-row plan (afx_bandplan_build) into the shortest of the `n` compiled layouts that holds it.  rowCap:
 * floats of the kernel's zero-padded power row; curSlots: tapsA + tapsB of the variant the plan would otherwise run.
 * Returns 0 and fills *out, or 1 (nothing allocated) when it declines: num <= 64, a split plan, a row longer than every
 * layout, no layout shorter than curSlots, or no such layout placed with at most AFX_BANDPACK_MAX_PAIRS conflicting pairs. */
#define AFX_BANDPACK_MAX_PAIRS 1
int afx_bandpack_build(const AfxBandPlan *plan, const int (*layouts)[3], int n, int rowCap, int curSlots, AfxBandPack *out);
void afx_bandpack_free(AfxBandPack *p);

#ifdef __cplusplus
}
#endif

#endif /* AFX_BANDPACK_H */
