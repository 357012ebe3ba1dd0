/* afx_objects.h -- layouts of the opaque handles (library-internal). */
#ifndef AFX_OBJECTS_H
#define AFX_OBJECTS_H

#include <stddef.h>

#include "afx_frametail.h"
#include "afx_objkit.h"
#include "afx_pitchkit.h"
#include "flux_base.h"
#include "reassign_algorithm.h"
#include "dsp/resample_algorithm.h"

#ifdef __cplusplus
extern "C" {
#endif

struct AfxMelFusedPlan; /* afx_melfused.hip */

struct OpaqueBFT {
    /* plan */
    int fftLength, radix2Exp, F, num;
    int samplate;
    float lowFre, highFre;
    int lowIndex, highIndex; /* linear scale: first/last bin */
    int binPerOctave;
    WindowType windowType;
    int slideLength;
    SpectralDataType dataType;
    SpectralFilterBankScaleType scale;
    SpectralFilterBankStyleType style;
    SpectralFilterBankNormalType normal;
    int resultType;  /* 0 complex, 1 real */
    float normValue; /* default 1 */
    int isTemporal;
    float *freBandArr; /* host, num+2 */
    int *binBandArr;
    /* device constants */
    void *stream;
    float *dWindow, *dTwiddle, *dBank;
    int bankPitch; /* floats per row of dBank: F rounded up to 4 (zero padded) so that the MFMA GEMM
                    * loads 16-byte aligned rows */
    /* banded (row span) view of the bank for the in-kernel filter-bank epilogue of the
     * size-generic STFT kernel; NULL when the bank is too dense for it */
    int *dBandMeta;   /* [3][num]: start, len, offset */
    float *dBandW;
    struct AfxMelFusedPlan *fast; /* NULL when the fused kernel does not apply */
    struct OpaqueReassign *reassign; /* isReassign = 1: the reassigned spectrum replaces the STFT */
    /* grow-only device scratch of the legacy host-pointer calls */
    void *dBankImage; /* dense banks: dBank as three bf16 word planes in the GEMM's staging order (afxk_gemm_bank_prepare),
                       * built on the first dense call; bankImageTried: the stand-in / a failure left none -- float bank then */
    int bankImageTried;
    float *dX, *dSpec, *dOut, *dTemporal;
    size_t capX, capSpec, capOut, capTemporal;
    /* host copies for bftObj_getTemporalData */
    float *hTemporal;
    int hTemporalCap, hTemporalFrames;
    int lastTimeLength;
    int status; /* last failure of a void entry point */
    AfxScratchStream scratchStream; /* stream of the previous launch (the scratch is shared; afx_objkit.h) */
};

struct OpaqueXXCC {
    int num;
    int timeLength;
    void *stream;
    float *dDct; /* device [num, num] orthonormal DCT-II */
    float *dIn, *dOut;
    size_t capIn, capOut;
    int status;
};

/* the spectral-descriptor object (afx_descriptor.c, feature/spectral_algorithm.h) */
struct OpaqueSpectral {
    int num;
    int timeLength;
    float *freBandArr;  /* host copy [num] */
    float *dFre;        /* device [num] */
    int *indexArr;      /* host: the edge, indexLength entries (owned) */
    int indexLength;
    int start, end;     /* first / last entry of indexArr */
    int isRange;        /* indexArr is start .. end: the kernels need no index table */
    int *dIndex;        /* device copy of indexArr for an index-list edge */
    size_t capIndex;
    float meanFre, slopeDen, varFre; /* per-edge constants of slope / mean / var, summed in the reference's order */
    int isPower;        /* energy: rows are power already (the spectrogram object's dataType) */
    void *stream;
    float *dIn, *dPhase, *dOut; /* grow-only device buffers of the host-pointer calls */
    size_t capIn, capPhase, capOut;
    int status;
};

struct OpaqueSTFT {
    int fftLength, radix2Exp, slideLength;
    WindowType windowType;
    int isPad;
    PaddingPositionType positionType;
    PaddingModeType modeType;
    float padValue1, padValue2;
    float *windowDataArr; /* host [fftLength]; stftObj_useWindowDataArr overwrites it */
    int windowDirty;      /* dWindow is stale */
    AfxFrameTail tail;    /* isContinue and the samples carried to the next streaming call; its hop follows slideLength */
    int timeLength;       /* frames of the last stft call */
    int methodType;       /* inverse: 0 weighted overlap-add, 1 overlap-add, -1 not built */
    float *winArr1, *winArr2; /* host: window^e, window^(e+1) */
    void *stream;
    float *dWindow, *dTwiddle, *dWin12;
    float *dX, *dOut, *dFrames; /* grow-only device scratch */
    size_t capX, capOut, capFrames;
    AfxScratchStream scratchStream;
    int status;
};

struct OpaqueReassign {
    int radix2Exp, fftLength, F, samplate, slideLength, isPadding;
    WindowType windowType;
    ReassignType resType;
    float thresh;
    int resultType, order;
    void *stream;
    float *dWin;      /* device [3][N]: h, dh, t.h */
    float *dTwiddle, *dFre;
    float *dPlanes, *dX, *dOut; /* grow-only scratch */
    int *dIdx;
    size_t capPlanes, capIdx, capX, capOut;
    AfxScratchStream scratchStream;
    int status;
};

/* the harmonic / percussive separation object (afx_hpss.c, mir/hpss_algorithm.h) */
struct OpaqueHPSS {
    struct OpaqueSTFT *stft; /* owned: Hamm by default, hop fftLength/4, no padding, not continuing; its stream is the object's */
    int radix2Exp, fftLength, slideLength;
    int hOrder, pOrder;
    void *stream;
    float *dSpec;            /* grow-only chunk scratch: half spectrum re | im, then the full spectra of the outputs */
    size_t capSpec;
    float *dX, *dH, *dP;     /* grow-only device buffers of the host-pointer call */
    size_t capX, capH, capP;
    AfxScratchStream scratchStream;
    int status;
};

/* The pitch trackers: `head` (afx_pitchkit.h) holds the sizes, the tail, the stream, the staging buffers and the status. */

/* YIN (afx_pitch_yin.c, mir/_pitch_yin.h); head.dOut holds [3][T] */
struct OpaquePitchYIN {
    AfxPitchHead head;
    int autoLength;
    int minIndex, maxIndex, diffLength, yinLength; /* lags of the curve: minIndex ... maxIndex < diffLength = fftLength - autoLength */
    float thresh;
    float *dTwiddle;
    float *dCand;            /* grow-only, of the host-pointer call: [2][T, mLen] + lengths */
    size_t capCand;
    float *hOut;             /* host staging [3][T] */
    float *mFreArr, *mTroughArr; /* host [T, mLen]: pitchYINObj_getTroughData */
    int *lenArr;
    size_t capHost;          /* frames the host arrays hold */
};

/* harmonic product spectrum and log-harmonic sum (afx_pitch_hs.c, mir/_pitch_hps.h, mir/_pitch_lhs.h): one layout, `kind`
 * selects the combining operator */
struct OpaquePitchHS {
    AfxPitchHead head;
    int kind;                /* AFX_PITCH_HPS / AFX_PITCH_LHS */
    int interpLength, interpExp; /* M = 2^interpExp: the zero-padded transform the reference runs per frame */
    int minIndex, maxIndex, harmonicCount;
    int lastBin;             /* maxIndex * harmonicCount: the highest bin of the M-point spectrum a curve reads */
    int sliceInLds;          /* the spectrum slice fits in LDS beside the transform buffer and the frame */
    int transforms;          /* fftLength-point transforms per frame */
    WindowType windowType;
    float *dWindow, *dTwiddle, *dRoots;
    float *dSlice;           /* grow-only: [groups][slice floats] of the plans whose slice does not fit in LDS */
    size_t capSlice;
    AfxScratchStream scratchStream;
};

/* the pitch-estimation filter (afx_pitch_pef.c, mir/_pitch_pef.h) */
struct OpaquePitchPEF {
    AfxPitchHead head;
    int minIndex, maxIndex, filterPadNum;
    int pwLength;            /* bins of the power spectrum the log grid reads */
    float lowFre, highFre, cutFre, alpha, beta, gamma;
    WindowType windowType;
    float *dWindow, *dTwiddle, *dTaps, *dFilterSpec, *dLg; /* uploaded once: [N], [4N], [2N] taps, [2N + 1] float2, [2N] */
};

/* the lag-domain trackers: normalised autocorrelation and cepstrum (afx_pitch_lag.c, mir/_pitch_ncf.h, mir/_pitch_cep.h):
 * one layout, `mode` selects the function of the spectrum */
struct OpaquePitchLag {
    AfxPitchHead head;
    int mode;                /* AFX_PITCH_LAG_NCF / AFX_PITCH_LAG_CEP */
    int minIndex, maxIndex;
    float lowFre, highFre;
    WindowType windowType;
    float *dWindow, *dTwiddle; /* uploaded once: [N] (NULL for the rectangular window), [2N] */
};
struct OpaquePitchNCF {
    struct OpaquePitchLag lag;
};
struct OpaquePitchCEP {
    struct OpaquePitchLag lag;
};

/* the harmonic ratio (afx_harmonic_ratio.c, mir/harmonicRatio_algorithm.h); head.fftLength is the WINDOW length N (the frame
 * the call layer counts in), the transforms have 2N points */
struct OpaqueHarmonicRatio {
    AfxPitchHead head;
    int maxLength;
    float lowFre;
    float *dWindow, *dTwiddle; /* uploaded once: [N], [2N] */
    int *dScratch;           /* grow-only: afx_harmonic_ratio_scratch_ints(frames of a call) */
    size_t capScratch;
    AfxScratchStream scratchStream;
};

/* the onset detector (afx_onset.c, mir/onset_algorithm.h) */
struct OpaqueOnset {
    int noveltyType;         /* taken unchecked: anything that is not a named kind runs flux */
    int nLength, mLength, order;
    int preMax, postMax, preAvg, postAvg, wait;
    float delta;
    int step;                /* of the last call (onsetObj_debug prints it) */
    void *stream;
    float *dFre;             /* [mLength] zeros: the descriptor launcher wants a frequency table, no novelty kind reads it */
    int *hIndex, *dIndex;    /* the index table of the last call that brought one, host copy and device copy */
    int indexLength;
    size_t capIndex;
    float *dFilt, *dRaw;     /* grow-only scratch: the filtered rows of a chunk of clips (order >= 2), the raw novelty */
    size_t capFilt, capRaw;
    float *dIn, *dPhase, *dEvn; /* grow-only device buffers of the host-pointer call */
    int *dPoint;             /* [nLength + 1]: the points, then their count */
    size_t capIn, capPhase, capEvn, capPoint;
    AfxScratchStream scratchStream;
    int status;
};

/* the resampler (afx_resample.c, dsp/resample_algorithm.h) */
struct OpaqueResample {
    AfxResamplePlan plan;    /* what the constructor and the rate setters decided; plan.table is interpArr, host,
                              * [interpLength + 1]: the last entry repeated for the kernel's neighbour difference */
    void *stream;
    float *dTable;           /* [interpLength + 1], uploaded by the constructor and by every setter that rescales */
    float *dX, *dOut;        /* grow-only device buffers of the host-pointer call */
    size_t capX, capOut;
    AfxScratchStream batchStream; /* of the last batched call: a setter drains it before the table changes */
    int status;
};

/* the time-stretch object (afx_timestretch.c, mir/timeStretch_algorithm.h) */
struct OpaqueTimeStretch {
    struct OpaqueSTFT *stft; /* owned: no padding, not continuing; its stream is the object's */
    int radix2Exp, fftLength, slideLength;
    long long scratchLimit;  /* bytes dScratch may grow to (one clip is always taken) */
    void *stream;
    float *dScratch;         /* grow-only chunk scratch: output spectrum re | im, half spectrum re | im, inverse transform */
    size_t capScratch;
    float *dX, *dOut;        /* grow-only device buffers of the host-pointer call */
    size_t capX, capOut;
    AfxScratchStream scratchStream;
    int status;
};

/* the pitch-shift object (afx_pitchshift.c, mir/pitchShift_algorithm.h) */
struct OpaquePitchShift {
    struct OpaqueTimeStretch *stretch; /* owned; its stream is the object's */
    struct OpaqueResample *resample;   /* owned: Fast, isScale 1 */
    float lastRate;                    /* the ratio the resampler was last set to by this object (rateSet: it was set at all) */
    int rateSet;
    long long scratchLimit;
    void *stream;
    float *dScratch;         /* grow-only chunk scratch: stretched clips, resampled clips */
    size_t capScratch;
    float *dX, *dOut;
    size_t capX, capOut;
    AfxScratchStream scratchStream;
    int status;
};

/* validated parameters of a BFT execution plan (afx_bft.c) */
typedef struct {
    int num, radix2Exp, samplate;
    float lowFre, highFre;
    int lowIndex, highIndex, binPerOctave;
    WindowType windowType;
    int slideLength;
    SpectralDataType dataType;
    SpectralFilterBankScaleType scale;
    SpectralFilterBankStyleType style;
    SpectralFilterBankNormalType normal;
    int isTemporal, isReassign;
    const float *customBank; /* optional host [num, fftLength/2+1] matrix used instead of the
                              * auditory bank of `scale` (band arrays are then left zero) */
} AfxBftPlan;
int afx_bft_create(const AfxBftPlan *p, struct OpaqueBFT **bftObj);

/* fused-kernel hooks (afx_melfused.hip) */
int afx_bft_plan_fast(struct OpaqueBFT *o, const float *hWindow, const float *hBank);
int afx_bft_try_fast(struct OpaqueBFT *o, const float *dData, int batch, int dataLength,
                     long long clipStride, float *dRe, float *dIm, float *dTemporal, void *stream,
                     int *used);
int afx_bft_try_fast_cc(struct OpaqueBFT *o, struct OpaqueXXCC *x, const float *dData, int batch,
                        int dataLength, long long clipStride, int ccNum,
                        CepstralRectifyType *rectifyType, float *dMel, float *dCc, void *stream,
                        int *used);
void afx_bft_free_fast(struct OpaqueBFT *o);

int afx_bft_run_device(struct OpaqueBFT *o, const float *dData, int batch, int dataLength,
                       long long clipStride, float *dRe, float *dIm, float *dTemporal,
                       void *stream);

/* afx_spectrogram.c: the descriptor object a spectrogram object owns (built on first use over its num bands and
 * freBandArr, isPower from its dataType) and the frame count of its last spectrogram call; NULL on failure (reported) */
struct OpaqueSpectrogram;
struct OpaqueSpectral *afx_spectrogram_descriptor(struct OpaqueSpectrogram *o, const char *who, int *timeLength);

#ifdef __cplusplus
}
#endif
#endif /* AFX_OBJECTS_H */
