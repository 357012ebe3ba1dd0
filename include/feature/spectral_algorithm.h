/* spectral_algorithm.h -- C ABI of the spectral-descriptor object: per-frame statistics of a [T, num] magnitude or
 * power spectrogram (flatness, flux, rolloff, centroid, spread, skewness, kurtosis, entropy, crest, slope, decrease,
 * band width, rms, energy, hfc, sd, sf, mkl, pd, wpd, nwpd, cd, rcd, broadband, novelty, eef, eer, max, mean, var), on an
 * MI355X: one pass over the rows per call (csrc/hip/afx_descriptors.hip).
 *
 * Replaces the reference functions of the same names (src/feature/spectral_algorithm.h:12-89,
 * src/feature/spectral_algorithm.c:57-1160, src/flux_spectral.c:21-833) as bound by
 * python/audioflux/feature/spectral.py.  The additive device-pointer form -- any list of descriptors in one call on rows
 * that already sit in HBM -- is spectralObj_computeDevice in afx_batch.h.
 *
 * Every descriptor runs over the object's EDGE: bins start .. end (spectralObj_setEdge) or an index list in any order
 * (spectralObj_setEdgeArr); the whole row by default.
 *
 * Where this backend differs from the reference, on purpose:
 *   - the reference caches per-frame sums, centroid, spread, entropy and means between calls and invalidates them only in
 *     setTimeLength / setEdge, so it answers with STALE values when the data changes under an unchanged object; every
 *     call here computes from the data it is handed.  The two agree whenever the reference's caches are valid.
 *   - freBandArr is copied at construction (the reference keeps the caller's pointer).
 *   - entropy, eef and eer of an all-zero frame are NaN (0 / 0) in the reference; the same NaN comes back here.
 * The legacy calls upload timeLength x num floats per call and download the result; consecutive calls on one array
 * upload it again.
 */
#ifndef SPECTRAL_ALGORITHM_H
#define SPECTRAL_ALGORITHM_H

#include "../flux_base.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueSpectral *SpectralObj;

/* num = columns of the spectrogram (>= 2), freBandArr[num] their frequencies.  returns 0, -1 on bad num ("num is
 * error!!!"), <= -2 on backend failure.  replaces spectral_algorithm.c:57-92 */
int spectralObj_new(SpectralObj *spectralObj, int num, float *freBandArr);

/* edge = bins start .. end, both inclusive, 0 <= start < end <= num - 1; anything else is ignored.
 * replaces spectral_algorithm.c:160-186 */
void spectralObj_setEdge(SpectralObj spectralObj, int start, int end);
/* edge = indexArr[0 .. indexLength - 1] (any order, repeats allowed).  TAKES OWNERSHIP of indexArr, which must come from
 * calloc / malloc: it is freed at once when an index is outside 0 .. num - 1 (and nothing changes), later otherwise.
 * replaces spectral_algorithm.c:188-218 */
void spectralObj_setEdgeArr(SpectralObj spectralObj, int *indexArr, int indexLength);

/* frames of the next calls.  replaces spectral_algorithm.c:94-158 */
void spectralObj_setTimeLength(SpectralObj spectralObj, int timeLength);

/* mDataArr / mSpecArr / mPhaseArr [timeLength, num] -> dataArr[timeLength] (max / mean / var: valueArr, freArr) */
/* exp(mean log(x + 2e-16)) / mean x over the edge; 0 when the mean is 0.
 * replaces spectral_algorithm.c:220-248, flux_spectral.c:21-57 */
void spectralObj_flatness(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* step < 1 -> 1, first `step` outputs 0; isExp / type NULL -> 0 (type 0 sum, 1 mean).
 * replaces spectral_algorithm.c:250-280, flux_spectral.c:60-104 */
void spectralObj_flux(SpectralObj spectralObj, float *mDataArr, int step, float p, int isPostive, int *isExp, int *type, float *dataArr);
/* freBandArr at the FIRST edge position whose running sum of |x| reaches threshold * sum x.
 * replaces spectral_algorithm.c:282-309, flux_spectral.c:106-145 */
void spectralObj_rolloff(SpectralObj spectralObj, float *mDataArr, float threshold, float *dataArr);
/* sum f x / sum x; 0 when the sum is 0.
 * replaces spectral_algorithm.c:311-318, flux_spectral.c:147-172 */
void spectralObj_centroid(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* sqrt(sum (f - centroid)^2 x / sum x).
 * replaces spectral_algorithm.c:320-327, flux_spectral.c:174-201 */
void spectralObj_spread(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* sum (f - centroid)^3 x / (spread^3 sum x).
 * replaces spectral_algorithm.c:329-362, flux_spectral.c:203-232 */
void spectralObj_skewness(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* sum (f - centroid)^4 x / (spread^4 sum x).
 * replaces spectral_algorithm.c:364-397, flux_spectral.c:234-263 */
void spectralObj_kurtosis(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* -sum v log2(v + 1e-16), v = x / sum x; isNorm: / log2(edge length).  A silent frame is 0 / 0 = NaN, as in the reference.
 * replaces spectral_algorithm.c:399-406, flux_spectral.c:265-294 */
void spectralObj_entropy(SpectralObj spectralObj, float *mDataArr, int isNorm, float *dataArr);
/* max x / mean x.
 * replaces spectral_algorithm.c:408-435, flux_spectral.c:296-324 */
void spectralObj_crest(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* regression slope of x on f over the edge.
 * replaces spectral_algorithm.c:437-468, flux_spectral.c:326-364 */
void spectralObj_slope(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* sum_{k >= 1} (x_k - x_0) / bin_k / (sum x - x_0): the ABSOLUTE bin index divides.
 * replaces spectral_algorithm.c:470-496, flux_spectral.c:366-397 */
void spectralObj_decrease(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* (sum x (f - centroid)^p)^(1/p); p = 2 is the reference default.
 * replaces spectral_algorithm.c:498-525, flux_spectral.c:399-432 */
void spectralObj_bandWidth(SpectralObj spectralObj, float *mDataArr, float p, float *dataArr);
/* sqrt(2 sum w x^2) / num, w = 1/2 at bin 0 and, for even num, bin num - 1: num, not the edge length.
 * replaces spectral_algorithm.c:527-544, flux_spectral.c:434-459 */
void spectralObj_rms(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* mean of x^2 (isLog: of log(1 + gamma x^2), gamma <= 0 -> 10) over the edge.
 * replaces spectral_algorithm.c:546-565, flux_spectral.c:804-832 */
void spectralObj_energy(SpectralObj spectralObj, float *mDataArr, int isLog, float gamma, float *dataArr);
/* sum x bin: the ABSOLUTE bin index weights.
 * replaces spectral_algorithm.c:567-583, flux_spectral.c:463-484 */
void spectralObj_hfc(SpectralObj spectralObj, float *mDataArr, float *dataArr);
/* sum |x_i - x_{i-step}| (isPostive: positive part); first `step` outputs 0.
 * replaces spectral_algorithm.c:585-602, flux_spectral.c:486-520 */
void spectralObj_sd(SpectralObj spectralObj, float *mDataArr, int step, int isPostive, float *dataArr);
/* the same with squares.
 * replaces spectral_algorithm.c:604-621, flux_spectral.c:522-556 */
void spectralObj_sf(SpectralObj spectralObj, float *mDataArr, int step, int isPostive, float *dataArr);
/* sum log(1 + x_i / (x_{i-1} + 1e-16)); type 1: mean; output 0 is 0.
 * replaces spectral_algorithm.c:623-640, flux_spectral.c:558-587 */
void spectralObj_mkl(SpectralObj spectralObj, float *mDataArr, int type, float *dataArr);
/* mean |second difference of the phase|; outputs 0 and 1 are 0.
 * replaces spectral_algorithm.c:642-658, flux_spectral.c:589-655 */
void spectralObj_pd(SpectralObj spectralObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
/* the same weighted by x.
 * replaces spectral_algorithm.c:660-676, flux_spectral.c:589-666 */
void spectralObj_wpd(SpectralObj spectralObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
/* wpd / (mean x + 1e-16).
 * replaces spectral_algorithm.c:678-694, flux_spectral.c:589-677 */
void spectralObj_nwpd(SpectralObj spectralObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
/* sum |X_i - predicted X_i| in the complex domain; output 0 is 0.
 * replaces spectral_algorithm.c:696-712, flux_spectral.c:679-747 */
void spectralObj_cd(SpectralObj spectralObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
/* cd over the rising bins only.
 * replaces spectral_algorithm.c:714-730, flux_spectral.c:679-757 */
void spectralObj_rcd(SpectralObj spectralObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
/* COUNT of bins with 10 log10(x_i / x_{i-1}) > threshold; output 0 is 0 (the reference increments dataArr: this backend stores the count).
 * replaces spectral_algorithm.c:733-750, flux_spectral.c:759-778 */
void spectralObj_broadband(SpectralObj spectralObj, float *mDataArr, float threshold, float *dataArr);
/* sum (Value) or COUNT (Number) of the per-bin terms above threshold; NULL -> Sub / Value; first `step` outputs 0.
 * replaces spectral_algorithm.c:758-779, flux_spectral.c:780-802 */
void spectralObj_novelty(SpectralObj spectralObj, float *mDataArr, int step, float threshold, SpectralNoveltyMethodType *methodType, SpectralNoveltyDataType *dataType, float *dataArr);
/* sqrt(1 + |energy entropy|); NaN on a silent frame, as in the reference.
 * replaces spectral_algorithm.c:781-816 */
void spectralObj_eef(SpectralObj spectralObj, float *mDataArr, int isNorm, float *dataArr);
/* sqrt(1 + |log(1 + gamma energy) / entropy|); NaN on a silent frame, as in the reference.
 * replaces spectral_algorithm.c:818-853 */
void spectralObj_eer(SpectralObj spectralObj, float *mDataArr, int isNorm, float gamma, float *dataArr);
/* the FIRST maximum of the edge and its frequency.
 * replaces spectral_algorithm.c:855-891 */
void spectralObj_max(SpectralObj spectralObj, float *mDataArr, float *valueArr, float *freArr);
/* mean x and mean f of the edge (the plain means: the reference adds onto meanFreArr[0] from call to call).
 * replaces spectral_algorithm.c:893-901, :1097-1147 */
void spectralObj_mean(SpectralObj spectralObj, float *mDataArr, float *valueArr, float *freArr);
/* sum (mean - x)^2 / (edge length - 1) and the same for f; an edge of one bin writes nothing.
 * replaces spectral_algorithm.c:903-961 */
void spectralObj_var(SpectralObj spectralObj, float *mDataArr, float *valueArr, float *freArr);

/* NULL-safe.  replaces spectral_algorithm.c:1149-1195 (which frees nothing) */
void spectralObj_free(SpectralObj spectralObj);

#ifdef __cplusplus
}
#endif

#endif /* SPECTRAL_ALGORITHM_H */
