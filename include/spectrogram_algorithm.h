/* spectrogram_algorithm.h -- C ABI of the spectrogram object (core): STFT -> power / magnitude
 * -> linear slice | mel / bark / erb / octave / linspace / log filter bank | STFT-chroma |
 * log-chroma, optional streaming continuation, cepstral coefficients of the result
 * (mfcc / bfcc / gtcc / xxcc) and the spectral deconvolution.  This is what the reference's
 * MelSpectrogram / BarkSpectrogram / ErbSpectrogram / Spectrogram / Linear / Mel / Bark / Erb /
 * Chroma wrapper classes and its published benchmark (benchmark/run_audioflux.py:15-22) call.
 *
 * Replaces the reference functions of the same names (src/spectrogram_algorithm.h:43-106,
 * src/spectrogram_algorithm.c:186-1525, :1540-1612, :3029-3200) as bound by
 * python/audioflux/spectrogram.py.  Execution: the kernels of the BFT path (fused STFT ->
 * banded filter bank, size-generic STFT, MFMA GEMM, MFMA cepstra) plus k_spec_map / k_row_post.
 *
 * The spectral descriptors of the result (spectrogramObj_flatness ... spectrogramObj_var) forward to
 * the descriptor object of feature/spectral_algorithm.h, which the spectrogram object owns.
 *
 * Not provided by this backend: the "deep" salience scales (newDeep /
 * newDeepChroma return -4).
 */
#ifndef SPECTROGRAM_ALGORITHM_H
#define SPECTROGRAM_ALGORITHM_H

#include "flux_base.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OpaqueSpectrogram *SpectrogramObj;

/* every pointer argument is optional (NULL -> reference default): samplate 32000, lowFre 0
 * (octave-like scales: C1 .. 38 semitones above A4), highFre samplate/2, binPerOctave 12,
 * radix2Exp 12, window Hann, slideLength fftLength/4, isContinue 0, dataType Power, scale
 * Linear, style Slaney, normal None.  Linear: num is derived from [lowFre, highFre]
 * (spectrogramObj_getBandNum).  returns 0, -100 bad radix2Exp, -1 bad num / range,
 * -4 deep scales, <= -2 backend failure.  replaces spectrogram_algorithm.c:326-582 */
int spectrogramObj_new(SpectrogramObj *spectrogramObj, int num, int *samplate, float *lowFre,
                       float *highFre, int *binPerOctave, int *radix2Exp, WindowType *windowType,
                       int *slideLength, int *isContinue, SpectralDataType *dataType,
                       SpectralFilterBankScaleType *filterScaleType,
                       SpectralFilterBankStyleType *filterStyleType,
                       SpectralFilterBankNormalType *filterNormalType);

/* replace spectrogram_algorithm.c:186-324 */
int spectrogramObj_newLinear(SpectrogramObj *spectrogramObj, int samplate, int radix2Exp, int *isContinue);
int spectrogramObj_newMel(SpectrogramObj *spectrogramObj, int num, int samplate, int radix2Exp, int *isContinue);
int spectrogramObj_newBark(SpectrogramObj *spectrogramObj, int num, int samplate, int radix2Exp, int *isContinue);
int spectrogramObj_newErb(SpectrogramObj *spectrogramObj, int num, int samplate, int radix2Exp, int *isContinue);
int spectrogramObj_newChroma(SpectrogramObj *spectrogramObj, int samplate, int radix2Exp, int *isContinue);
int spectrogramObj_newDeep(SpectrogramObj *spectrogramObj, int num, int samplate, int radix2Exp, int *isContinue);
int spectrogramObj_newDeepChroma(SpectrogramObj *spectrogramObj, int samplate, int radix2Exp, int *isContinue);

/* replace spectrogram_algorithm.c:822-846 */
void spectrogramObj_setDeepOrder(SpectrogramObj spectrogramObj, int deepOrder);
void spectrogramObj_setChromaDataNormalType(SpectrogramObj spectrogramObj, ChromaDataNormalType dataNormType);
void spectrogramObj_setDataNormValue(SpectrogramObj spectrogramObj, float normValue);

/* replace spectrogram_algorithm.c:848-853, :3171-3200 */
int spectrogramObj_calTimeLength(SpectrogramObj spectrogramObj, int dataLength);
void spectrogramObj_enableDebug(SpectrogramObj spectrogramObj, int flag);
float *spectrogramObj_getFreBandArr(SpectrogramObj spectrogramObj);
int *spectrogramObj_getBinBandArr(SpectrogramObj spectrogramObj);
int spectrogramObj_getBandNum(SpectrogramObj spectrogramObj);
int spectrogramObj_getBinBandLength(SpectrogramObj spectrogramObj);

/* dataArr[dataLength] -> mSpectArr [T, num]; mPhaseArr [T, num] (linear scale only, may be NULL).
 * replaces spectrogram_algorithm.c:864-1393 */
void spectrogramObj_spectrogram(SpectrogramObj spectrogramObj, float *dataArr, int dataLength,
                                float *mSpectArr, float *mPhaseArr);
/* the same from a caller-supplied STFT mRealArr/mImageArr [nLength, mLength == fftLength].
 * replaces spectrogram_algorithm.c:1397-1402 */
void spectrogramObj_spectrogram1(SpectrogramObj spectrogramObj, float *mRealArr, float *mImageArr,
                                 int nLength, int mLength, float *mSpectArr, float *mPhaseArr);

/* cepstral coefficients of the LAST spectrogram's frame count: mDataArr1 [T, num] ->
 * mDataArr2 [T, ccNum].  mfcc / bfcc / gtcc act only on a mel / bark scale / gammatone style
 * object, as in the reference.  replace spectrogram_algorithm.c:1409-1525 */
void spectrogramObj_mfcc(SpectrogramObj spectrogramObj, float *mDataArr1, int ccNum, float *mDataArr2);
void spectrogramObj_gtcc(SpectrogramObj spectrogramObj, float *mDataArr1, int ccNum, float *mDataArr2);
void spectrogramObj_bfcc(SpectrogramObj spectrogramObj, float *mDataArr1, int ccNum, float *mDataArr2);
void spectrogramObj_xxcc(SpectrogramObj spectrogramObj, float *mDataArr1, int ccNum,
                         CepstralRectifyType *rectifyType, float *mDataArr2);
/* empty in the reference (spectrogram_algorithm.c:1527-1538); kept for ABI compatibility */
void spectrogramObj_mfccStandard(SpectrogramObj spectrogramObj, float *mDataArr1, int *deltaWindowLength,
                                 CepstralEnergyType *energyType, CepstralRectifyType *rectifyType,
                                 float *mDataArr2);
void spectrogramObj_xxccStandard(SpectrogramObj spectrogramObj, float *mDataArr1, int *deltaWindowLength,
                                 CepstralEnergyType *energyType, CepstralRectifyType *rectifyType,
                                 float *mDataArr2);

/* mDataArr1 [T, num] -> timbre (formant) mDataArr2, pitch mDataArr3, both [T, num].
 * replaces spectrogram_algorithm.c:1546-1612 */
void spectrogramObj_deconv(SpectrogramObj spectrogramObj, float *mDataArr1, float *mDataArr2, float *mDataArr3);

/* ---- spectral descriptors of a result of spectrogramObj_spectrogram (src/spectrogram_algorithm.h:123-182,
 * src/spectrogram_algorithm.c:2020-3027).  Delegation: the object owns one descriptor object
 * (feature/spectral_algorithm.h, where every descriptor is defined) over its num bands and freBandArr; timeLength is that
 * of the last spectrogramObj_spectrogram call; spectrogramObj_energy takes power rows as they are when the object's
 * dataType is Power (spectrogram_algorithm.c:2648-2662; spectralObj_energy always squares). */
/* start / end count the object's bands 0 .. num - 1.  replaces spectrogram_algorithm.c:2020-2046 */
void spectrogramObj_setEdge(SpectrogramObj spectrogramObj, int start, int end);
/* takes ownership of the calloc'ed indexArr.  replaces spectrogram_algorithm.c:2048-2078 */
void spectrogramObj_setEdgeArr(SpectrogramObj spectrogramObj, int *indexArr, int indexLength);
/* mDataArr1 [T, num] / (sum of the window / 2: magnitude; (sum)^2 / 2: power), bins 0 and fftLength / 2 halved, into
 * mDataArr3 (NULL: in place).  replaces spectrogram_algorithm.c:2080-2120 */
void spectrogramObj_preprocess(SpectrogramObj spectrogramObj, float *mDataArr1, float *mDataArr3);

void spectrogramObj_flatness(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_flux(SpectrogramObj spectrogramObj, float *mDataArr, int step, float p, int isPostive, int *isExp, int *type, float *dataArr);
void spectrogramObj_rolloff(SpectrogramObj spectrogramObj, float *mDataArr, float threshold, float *dataArr);
void spectrogramObj_centroid(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_spread(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_skewness(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_kurtosis(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_entropy(SpectrogramObj spectrogramObj, float *mDataArr, int isNorm, float *dataArr);
void spectrogramObj_crest(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_slope(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_decrease(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_bandWidth(SpectrogramObj spectrogramObj, float *mDataArr, float p, float *dataArr);
void spectrogramObj_rms(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_energy(SpectrogramObj spectrogramObj, float *mDataArr, int isLog, float gamma, float *dataArr);
void spectrogramObj_hfc(SpectrogramObj spectrogramObj, float *mDataArr, float *dataArr);
void spectrogramObj_sd(SpectrogramObj spectrogramObj, float *mDataArr, int step, int isPostive, float *dataArr);
void spectrogramObj_sf(SpectrogramObj spectrogramObj, float *mDataArr, int step, int isPostive, float *dataArr);
void spectrogramObj_mkl(SpectrogramObj spectrogramObj, float *mDataArr, int type, float *dataArr);
void spectrogramObj_pd(SpectrogramObj spectrogramObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
void spectrogramObj_wpd(SpectrogramObj spectrogramObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
void spectrogramObj_nwpd(SpectrogramObj spectrogramObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
void spectrogramObj_cd(SpectrogramObj spectrogramObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
void spectrogramObj_rcd(SpectrogramObj spectrogramObj, float *mSpecArr, float *mPhaseArr, float *dataArr);
void spectrogramObj_broadband(SpectrogramObj spectrogramObj, float *mDataArr, float threshold, float *dataArr);
void spectrogramObj_novelty(SpectrogramObj spectrogramObj, float *mDataArr, int step, float threshold, SpectralNoveltyMethodType *methodType, SpectralNoveltyDataType *dataType, float *dataArr);
void spectrogramObj_eef(SpectrogramObj spectrogramObj, float *mDataArr, int isNorm, float *dataArr);
void spectrogramObj_eer(SpectrogramObj spectrogramObj, float *mDataArr, int isNorm, float gamma, float *dataArr);
void spectrogramObj_max(SpectrogramObj spectrogramObj, float *mDataArr, float *valueArr, float *freArr);
void spectrogramObj_mean(SpectrogramObj spectrogramObj, float *mDataArr, float *valueArr, float *freArr);
void spectrogramObj_var(SpectrogramObj spectrogramObj, float *mDataArr, float *valueArr, float *freArr);

/* NULL-safe.  replaces spectrogram_algorithm.c:3029-3169 */
void spectrogramObj_free(SpectrogramObj spectrogramObj);

#ifdef __cplusplus
}
#endif
#endif /* SPECTROGRAM_ALGORITHM_H */
