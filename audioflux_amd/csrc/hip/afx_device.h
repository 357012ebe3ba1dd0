/* afx_device.h -- the thin C interface between the C host objects
 * (csrc/host) and the HIP layer (csrc/hip).
 *
 * The host side is plain C99 and never sees a HIP type: device buffers are
 * `void*`/`float*` device addresses, streams are opaque `void*`
 * (a hipStream_t underneath).  Every function returns 0 on success and a
 * negative status on failure; the text of the last failure is available from
 * afxdev_last_error().  There is NO CPU fallback anywhere behind this
 * interface: when no gfx950 device/runtime is usable the calls fail.
 */
#ifndef AFX_DEVICE_H
#define AFX_DEVICE_H

#include <math.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes returned through the public *_new functions as well */
#define AFX_OK 0
#define AFX_ERR_NODEVICE (-2)  /* HIP runtime / device missing            */
#define AFX_ERR_HIP (-3)       /* a HIP call or kernel launch failed      */
#define AFX_ERR_UNSUPPORTED (-4) /* parameter combination not implemented */
#define AFX_ERR_NOMEM (-5)
#define AFX_ERR_ARG (-6)

/* ---- runtime ---------------------------------------------------------- */
int afxdev_ensure(void);              /* initialise HIP, select device      */
const char *afxdev_last_error(void);
void afxdev_set_error(const char *fmt, ...);
int afxdev_device_count(void);
int afxdev_set_device(int ordinal);   /* process-wide default for new objects */
int afxdev_current_device(void);      /* this thread's HIP device, -1 if none */
int afxdev_bind_stream(void *stream); /* thread's device := the stream's device */
#define AFX_MAX_DEVICES 16           /* power of two; per-device one-time flags */
int afxdev_error_count(void);         /* failures reported on this thread so far */
/* a void entry point ends in failure `st`: one stderr line (who, status, last message) and the thread's
 * failure count advances even when no message was recorded on the way (the wrappers raise on it) */
void afxdev_report_failure(const char *who, int st);
/* process-wide switches, read from the environment once: AFX_NO_FUSED (size-generic kernels only: no wave-level /
 * register-resident / matrix-core specialisation), AFX_CQT_F32 (CQT octave products on the float32 matrix cores) */
int afxdev_no_fused(void);
int afxdev_cqt_f32(void);
/* first statement of every compute entry point: the object's device becomes current */
#define AFX_ENTER(o) do { if ((o) != NULL) (void)afxdev_bind_stream((o)->stream); } while (0)

int afxdev_malloc(void **dptr, size_t bytes);
void afxdev_free(void *dptr);
int afxdev_memset(void *dptr, int value, size_t bytes, void *stream);
int afxdev_h2d(void *dst, const void *src, size_t bytes, void *stream);
int afxdev_d2h(void *dst, const void *src, size_t bytes, void *stream);
int afxdev_d2d(void *dst, const void *src, size_t bytes, void *stream);
int afxdev_stream_create(void **stream);
void afxdev_stream_destroy(void *stream);
int afxdev_stream_sync(void *stream);
int afxdev_stream_wait_stream(void *waiter, void *signaler); /* device-side join: waiter waits for signaler's work so far */

/* grow-only scratch helper: (re)allocates *dptr when *capacity < bytes */
int afxdev_reserve(void **dptr, size_t *capacity, size_t bytes);

/* ---- kernels ---------------------------------------------------------- */

/* what the STFT kernel stores per bin */
enum {
    AFX_SPEC_COMPLEX = 0, /* re, im                       */
    AFX_SPEC_POWER = 1,   /* re^2+im^2                    */
    AFX_SPEC_MAG = 2,     /* sqrt(re^2+im^2)              */
    AFX_SPEC_SQUARE = 3,  /* (re+j im)^2 = re^2-im^2, 2 re im */
    AFX_SPEC_POWER_NORM = 4, /* powf(re^2+im^2, normValue) */
    AFX_SPEC_MAG_NORM = 5,   /* powf(sqrt(re^2+im^2), normValue) */
    AFX_SPEC_PHASE = 6       /* atan2f(im, max(re, 1e-16)) (spectrogram_algorithm.c:1037-1053) */
};

typedef struct {
    const float *x;        /* device, clip b starts at x + b*clipStride      */
    long long clipStride;  /* in samples                                      */
    int batch;             /* clips                                           */
    int dataLength;        /* samples per clip                                */
    int timeLength;        /* frames per clip                                 */
    int radix2Exp;         /* fftLength = 1 << radix2Exp                      */
    int hop;
    const float *window;   /* device [fftLength]                              */
    const float *twiddle;  /* device [fftLength/2] float2: (cos, -sin)(2*pi*m/fftLength)  */
    int mode;              /* AFX_SPEC_*                                      */
    float normValue;
    int binLo;             /* first bin stored                                */
    int binCount;          /* bins stored per frame                           */
    long long outPitch;    /* floats between output rows; 0: binCount         */
    float *outRe;          /* device [batch*timeLength, binCount]             */
    float *outIm;          /* device, modes COMPLEX/SQUARE only               */
    float *energy;         /* optional device [batch*timeLength] (or NULL)    */
    float *rms;
    float *zcr;
    /* centre zero padding used by the CQT octaves: frame i covers samples
     * [i*hop - padLeft, i*hop - padLeft + fftLength) of the clip, reads
     * outside [0,dataLength) give 0 */
    int padLeft;
    /* optional banded filter bank applied in the same launch (all NULL/0: bins are stored):
     * row j = sum_q bandW[q * bandNum + j] * value[bandStart[j] + q], q < bandLen[j]
     * (weights tap-major so that the rows of a wave read neighbouring words; bandOff unused);
     * outRe/outIm then are [batch*timeLength, bandNum]; bandPost = AFX_MAP_POW applies
     * powf(., bandPostArg) to the real plane.  The spans must lie inside [binLo, binLo+binCount) */
    const int *bandStart, *bandLen, *bandOff;
    const float *bandW;
    int bandNum, bandPost;
    float bandPostArg;
    /* stftObj_stft: bins binLo+j above fftLength/2 are stored as the conjugate mirror
     * X[N-k]* (the reference keeps all fftLength bins of its complex transform) */
    int fullSpectrum;
    /* what a frame reads outside [0, dataLength): AFX_PAD_ZERO, or the stftObj padding modes
     * (stft_algorithm.c:601-694) applied as an index map -- no padded copy of the clip exists */
    int padMode;
    float padValueL, padValueR; /* AFX_PAD_CONST: left of sample 0 / right of the last sample */
} AfxStftArgs;
enum { AFX_PAD_ZERO = 0, AFX_PAD_CONST = 1, AFX_PAD_REFLECT = 2, AFX_PAD_WRAP = 3 };
/* clip index a padded position maps to (-1: constant), shared by the kernel and the host tests */
#ifdef __HIPCC__
#define AFX_HD __host__ __device__
#else
#define AFX_HD
#endif
AFX_HD static inline long long afx_pad_index(long long q, int n, int mode) {
    if (q >= 0 && q < n) return q;
    if (n < 2) return -1;
    if (mode == AFX_PAD_REFLECT) {
        const long long P = 2LL * (n - 1);
        long long m = q % P;
        if (m < 0) m += P;
        return m < n ? m : P - m;
    }
    if (mode == AFX_PAD_WRAP) {
        long long m = q % n;
        if (m < 0) m += n;
        return m;
    }
    return -1;
}

/* generic framed FFT, any radix2Exp in 1..14 */
int afxk_stft(const AfxStftArgs *a, void *stream);
/* energy / rms / zcr of the windowed frames alone (x, clipStride, batch, dataLength, timeLength, radix2Exp, hop, window,
 * padLeft / padMode, energy, rms, zcr are read): for bank rows that come from a fused kernel without them */
int afxk_temporal(const AfxStftArgs *a, void *stream);

/* inverse STFT (afx_istft.hip): re/im [batch*timeLength, N] -> out[b*outStride + j],
 * j < (timeLength-1)*hop + N: out = (out + sum_frames ifft*win1) / clamp(sum_frames win2) */
typedef struct {
    const float *re, *im;  /* device, split planes, row pitch N = 1 << radix2Exp            */
    int batch, timeLength, radix2Exp, hop;
    const float *twiddle;  /* device [N/2] float2                                            */
    const float *win1;     /* device [N]: window^e   (e = 1 weighted overlap-add, 0 plain)  */
    const float *win2;     /* device [N]: window^(e+1)                                       */
    float *frames;         /* device scratch [batch*timeLength, N]                           */
    float *out;            /* device; read-modify-write                                      */
    long long outStride;
} AfxIstftArgs;
int afxk_istft(const AfxIstftArgs *a, void *stream);
/* n_fft 256 ... 4096: one wave per frame (the inverse as ONE forward real transform of re + im of the Hermitian part), overlap-add
 * in an LDS ring, no frame scratch (a->frames / a->twiddle are not read); AFX_ERR_UNSUPPORTED: not its case -- run afxk_istft */
int afxk_istft_fused(const AfxIstftArgs *a, void *stream);

/* afx_spectral.hip: per-bin value (AFX_SPEC_*) of the bins [binLo, binLo+binCount) of a complex
 * spectrum re/im [rows, rowPitch] -> out [rows, binCount] (+ out2 for COMPLEX / SQUARE) */
int afxk_spec_map(const float *re, const float *im, long long rows, int rowPitch, int binLo,
                  int binCount, int mode, float normValue, float *out, float *out2, void *stream);
/* in place on data [rows, n]: optional powf(., powArg), then per-row normalisation
 * (normType = ChromaDataNormalType: 0 none, 1 max, 2 min, 3 P2, 4 P1) */
int afxk_row_post(float *data, long long rows, int n, int doPow, float powArg, int normType,
                  void *stream);

enum { AFX_MAP_NONE = 0, AFX_MAP_LOG10 = 1, AFX_MAP_CBRT = 2, AFX_MAP_POW = 3 };

/* C[M,N] = post( pre(A)[M,K] * B[N,K]^T ), row-major, f32 MFMA.
 * pre: AFX_MAP_NONE | LOG10 (log10f(max(a,1e-8))) | CBRT (powf(a,1/3))
 * post: AFX_MAP_NONE | POW (powf(c, postArg))
 * lda/ldc are row pitches in floats. */
int afxk_gemm_nt(const float *A, long long lda, const float *B, int ldb,
                 float *C, long long ldc, long long M, int N, int K,
                 int pre, int post, float postArg, void *stream);

/* the same product with every operand as three bf16 words on the bf16 matrix cores (afx_gemm_bf16.hip,
 * k_gemm_nt128_bf16x3): what afxk_gemm_nt runs for every product with N > 32 and no pre-map whose operands it takes;
 * pre is AFX_MAP_NONE; AFX_ERR_UNSUPPORTED for A or B off a 16-byte boundary or a pitch that is no multiple of 4 floats
 * (afxk_gemm_nt then runs the float32 kernel).  Non-finite values of A and B give the IEEE product (the split puts them
 * whole into the low word, which meets only the other operand's high word). */
int afxk_gemm_nt128_bf16(const float *A, long long lda, const float *B, int ldb, float *C, long long ldc,
                         long long M, int N, int K, int post, float postArg, void *stream);

/* the dense FILTER-BANK product with the bank prepared once per object (afx_gemm_bf16.hip, k_gemm_bank_bf16x3):
 * afxk_gemm_bank_prepare splits bank[N, K] (device, row pitch ldb floats) into its three bf16 word planes in the order the
 * kernel stages them ("bank image", device memory owned by the caller: afxdev_free); afxk_gemm_nt_bank computes
 * C[M, N] = post(A[M, K] . bank^T) with the float32 rows of A split while they are staged.  A: 16-byte aligned, lda a
 * multiple of 4 floats and at least K rounded up to 4 (the last quad of a row is read whole; what it holds behind K, NaN
 * included, reaches no result); AFX_ERR_UNSUPPORTED otherwise (callers then run afxk_gemm_nt on the float bank).
 * Every float32 value of A and of the bank is taken: +-Inf, NaN and values next to FLT_MAX give the IEEE product.
 * The reference's product: __mdot1, src/vector/flux_vector.c:55-86 */
int afxk_gemm_bank_prepare(const float *B, int ldb, int N, int K, void **bankImage, void *stream);
int afxk_gemm_nt_bank(const float *A, long long lda, const void *bankImage, int N, int K, float *C, long long ldc,
                      long long M, int post, float postArg, void *stream);

/* "standard" cepstra post-pass (xxcc_algorithm.c:244-292): per frame, put
 * ln(max(energy,1e-8)) in front of / in place of coefficient 0 and take the
 * causal smoothing-derivative FIR (util_delta, util/flux_util.c:803-815) along
 * the coefficient axis twice.
 *   cc[rows, ccNum] -> coe/delta1/delta2 [rows, outLen], outLen = ccNum (+1 if append)
 *   energyType: 0 replace, 1 append, 2 ignore */
int afxk_xxcc_standard(const float *cc, const float *energy, long long rows, int ccNum,
                       int energyType, int deltaLen, float *coe, float *delta1, float *delta2,
                       void *stream);

/* ---- continuous wavelet transform (afx_cwt.hip) ---------------------------- */
typedef struct {
    int r1, r2;      /* L = 2^(r1+r2): columns FFT 2^r1, rows FFT 2^r2               */
    int dataLength;  /* 2^radix2Exp samples in / per scale out                       */
    int pad;         /* reflect padding on each side                                 */
    int tileCols;    /* columns per workgroup in the column passes (divides 2^r2)    */
    const float *fastTw; /* device float2 tables of the register-FFT kernels (r1 = 8, r2 = 9):
                          * [8][64] W_512^(lane d) | [8][8] W_64^(c d) | [16][16] W_256^(g p);
                          * NULL: size-generic kernels only                            */
    const int *support;  /* device [num][2]: k2 range of each wavelet's non-zeros (or NULL)  */
    /* narrow-band scales (register-FFT plan only): a wavelet whose non-zeros lie in <= 16 rows
     * k2 of the transposed spectrum needs no row pass and no intermediate -- the column kernel
     * forms its operands from the spectrum directly (k_cwt_inv_cols256_nb).
     * order: device [num] scale indices, the nWide wide scales first, then the scales of the
     * classes R = 2, 4, 8, 16 (nNarrow[0..3] of them) and the two-block classes R = 20, 24, 32 (nNarrow[4..6]);
     * NULL: every scale takes both passes */
    const int *order;
    const int *orderLo;  /* device [num][2]: (order[i], support[2 order[i]]) -- one read per workgroup */
    int nWide;
    int nNarrow[7];
    int nTd;                 /* > 0: the FIRST nTd entries of `order` run the time-domain kernel (afx_cwt_td.hip),
                              * the nWide two-pass scales and the narrow-band classes follow */
    const struct AfxCwtTdPlan_ *td;
    const struct AfxCwtTdPlan_ *tdDet; /* the derivative bank's kernels for the same nTd scales; NULL: its scales take both passes */
} AfxCwtPlanDims;
/* ---- short-kernel ("wide") scales in the time domain on the f16 matrix cores (afx_cwt_td.hip) ----
 * pair: two scales share one MFMA column tile -- 32 columns = 2 scales x (re, im) x 8 output phases */
#define AFX_CWT_TD_MAXPAIRS 48 /* pairs of scales one time-domain launch takes (two launches: long and short kernels) */
#define AFX_CWT_TD_MAXK 1024   /* taps (incl. the 8 phase shifts) of the longest kernel the LDS-resident image takes */
typedef struct {
    int scale[2];            /* result rows (C order: row 0 = highest frequency); scale[1] < 0: a single scale */
    int kh;                  /* the window of output n0 starts at position n0 - kh (multiple of 8)           */
    int ks;                  /* K steps of 16 taps (even, >= 4)                                               */
    long long img;           /* byte offset of the pair's image in the blob: [word 2][ks][64 lanes][8] f16,
                              * the B-fragment order of v_mfma_f32_32x32x16_f16 (afx_cqt_time_kernel_f16)     */
    float colMul[32];        /* 2^-s_c of the image columns                                                   */
    float colSum[32];        /* the WHOLE kernel's response to a constant 1 (its spectrum's bin 0), per image column      */
} AfxCwtTdPair;
typedef struct AfxCwtTdPlan_ {
    const AfxCwtTdPair *pairs;   /* device [nPairs], longest kernels first */
    const unsigned char *image;  /* device blob */
    const int *hostKs;           /* host [nPairs]: K steps of every pair (the launcher sizes the workgroup shares) */
    int nPairs, maxKs;
    int wrap;                    /* 0: reflect padding (isPadding, cwt_algorithm.c:404-414), 1: circular */
} AfxCwtTdPlan;
/* chunk c at x + c xStride (dataLength = 2^r samples) -> outRe/outIm [chunks][num][dataLength], rows p->pairs[].scale */
/* AFX_OK when afxk_cwt_td takes this plan for chunks of dataLength samples and `num` output scales (every precondition
 * of the launch: checked once, when the object is planned -- a plan that fails goes back to the FFT path) */
int afxk_cwt_td_fits(const AfxCwtTdPlan *p, int dataLength, int num);
int afxk_cwt_td(const AfxCwtTdPlan *p, const float *x, long long xStride, int chunks, int dataLength, int num,
                float *outRe, float *outIm, void *stream, void *streamShort /* short-kernel class; NULL: `stream` */);
#define AFX_CWT_FASTTW_FLOATS (2 * (8 * 64 + 8 * 8 + 16 * 16))
/* `chunks` signals, chunk c at x + c*xStride -> Xt[c][L] complex (transposed layout:
 * frequency k1 + 2^r1 k2 at [k1][k2]); scratchA: chunks*L complex */
int afxk_cwt_forward(const AfxCwtPlanDims *d, const float *tw, const float *x, long long xStride,
                     int chunks, float *scratchA, float *Xt, void *stream);
/* Xt[chunks][L], bankT[num][L] (same layout) -> outRe/outIm [chunks][num][dataLength];
 * scratchB: chunks*num*L complex (wide part only).  parts: AFX_CWT_WIDE = the scales that take
 * the row pass + column pass (all of them when the plan has no narrow-band order),
 * AFX_CWT_NARROW = the narrow-band scales (no scratch, any number of chunks per launch) */
#define AFX_CWT_WIDE 1
#define AFX_CWT_NARROW 2
/* (the time-domain scales of the plan, d->nTd, are not part of either: afxk_cwt_td runs them from the signal itself) */
int afxk_cwt_inverse(const AfxCwtPlanDims *d, const float *tw, const float *Xt, const float *bankT,
                     int num, int isDet, int chunks, float *scratchB, float *outRe, float *outIm,
                     int parts, void *stream);

/* transforms with L = 2^(r1+r2) <= 8192, entirely in LDS: x (NULL: re-use the spectra in X) ->
 * X[chunks][L] natural order -> outRe/outIm [chunks][num][dataLength]; bankNatural [num][L] */
int afxk_cwt_small(const AfxCwtPlanDims *d, const float *tw, const float *x, long long xStride,
                   int chunks, const float *bankNatural, int num, int isDet, float *X, float *outRe,
                   float *outIm, void *stream);

/* synchrosqueezing pass (afx_wsst.hip): W, W' [batch][num][length] -> out += W at the row the
 * instantaneous frequency maps to.  mode 0: log axis (logMin/logMax = log2f(fmin), log2f(fmax)),
 * 1: linear axis (fmin, fmax), 2: nearest entry of freNorm[num] (band centres / samplate) */
typedef struct {
    const float *wRe, *wIm, *dRe, *dIm;
    float *outRe, *outIm; /* read-modify-write */
    int num, batch;
    long long length;
    int mode;
    float fmin, fmax, logMin, logMax, thresh;
    const float *freNorm;
    int phaseInput; /* 1: dRe holds the instantaneous frequency itself (synsqObj_synsq), dIm unused */
} AfxWsstArgs;
int afxk_wsst_squeeze(const AfxWsstArgs *a, void *stream);
/* phase-difference frequency estimate of a complex matrix re/im [num][length] -> phase [num][length] */
int afxk_synsq_phase(const float *re, const float *im, int num, long long length, float *phase, void *stream);

/* time-frequency reassignment (afx_reassign.hip): planes are [batch][timeLength][F] */
typedef struct {
    const float *hRe, *hIm;   /* STFT with the analysis window                         */
    const float *dhRe, *dhIm; /* ... with its derivative (doFre)                       */
    const float *thRe, *thIm; /* ... with the time-weighted window (doTime)            */
    const float *freArr;      /* device [F]: bin centre frequencies                    */
    int *timeIdx, *freIdx;    /* device scratch, same shape as the planes              */
    float *outRe, *outIm;     /* accumulated into (float atomics); outIm unused for amplitudes */
    int batch, timeLength, F, hop, samplate;
    int doFre, doTime, resultType;
    float thresh, freScale /* -0.5 sr / pi */, timeScale /* 1 / sr */;
} AfxReassignArgs;
int afxk_reassign(const AfxReassignArgs *a, int order, int *idxScratch, void *stream);

/* ---- constant-Q transform (afx_cqt.hip) ----------------------------------- */
typedef struct {
    const float *x;        /* device: this octave's signal                            */
    int validLength;       /* samples framed (length minus the dropped tail)          */
    int timeLength, radix2Exp, hop;
    const float *twiddle;  /* device [N/2] float2                                     */
    const int *kStart, *kLen, *kOff; /* device, per kernel row: first bin, taps, offset */
    const float *kTaps;    /* device float2 taps, rows packed back to back            */
    int rowBase;           /* first kernel row of this octave (0 unless variable-Q)   */
    int rows;              /* bins per octave                                         */
    const float *scale;    /* device [num]: sqrt(len_j) (or 1 when scaling is off)    */
    float octScale;        /* sqrt(2^k) of the octave                                 */
    int num, colBase;      /* output row pitch / first output column of this octave   */
    float *outRe, *outIm;  /* device [batch][T, num]                                  */
    int batch;             /* clips per launch (grid.y)                               */
    long long xStride;     /* samples between consecutive clips in x                  */
    long long outStride;   /* floats between consecutive clips in outRe/outIm         */
    const float *timeKernel; /* device [N][colTiles*32] time-domain kernels of this octave,
                              * columns [Re 0..rows-1 | Im 0..rows-1]; NULL: FFT path      */
    int colTiles;
    const unsigned short *timeKernelH; /* device [2][N/16][64][8] f16 (hi, lo) words of the scaled image in
                              * MFMA fragment order (afx_cqt_f16.hip); NULL: float32 kernels     */
    const float *colMul;     /* device [32]: 2^-s_j of the image columns                          */
    int rightPad;            /* 0: frame t covers samples [t hop - N/2, t hop + N/2) (centre padding, the default);
                              * 1: [t hop, t hop + N) (cqt_algorithm.c:1303-1318: the streaming object pads on the right) */
} AfxCqtOctaveArgs;
int afxk_cqt_octave(const AfxCqtOctaveArgs *a, void *stream);
/* f16 matrix-core variant; AFX_ERR_UNSUPPORTED when the plan / alignment is outside its scope */
int afxk_cqt_octave_f16(const AfxCqtOctaveArgs *a, void *stream);
/* The whole default ladder in ONE persistent launch (afx_cqt_f16.hip: k_cqt_pyramid): N = 512, 12 bins per octave,
 * seven octaves, hop 128 halving to 2.  Every workgroup walks a run of 32-frame tiles of one clip; its seven waves own
 * one octave each (window -> f16 (hi, lo) planes -> matrix-core product -> rows) and make the next level's samples
 * from the same planes (the 63-tap 2:1 resampler as one more matrix-core product); the level signals live in
 * per-workgroup rings of `ring` that stay in the L2, so a clip is read from HBM once and no level signal goes back to it.
 * cqt_algorithm.c:951-1048 (octave recursion), dsp/resample_algorithm.c:430-521 (the resampler). */
#define AFX_CQT_PYR_LEVELS 7
#define AFX_CQT_PYR_RING_FLOATS 17408 /* per workgroup: rings of 8192, 4096, 2048, 1024, 1024, 1024 samples */
#define AFX_CQT_PYR_MAX_WGS 256
#define AFX_CQT_PYR_TAB_COPY 704       /* bytes of one shifted copy of the tap table (328 f16 entries, padded) */
#define AFX_CQT_PYR_TAB_HALFS (2 * 4 * AFX_CQT_PYR_TAB_COPY / 2) /* [2 words][4 copies]                */
typedef struct {
    const float *x;          /* device clips (level 0)                                  */
    long long xStride;       /* samples between clips                                   */
    int batch, timeLength, num; /* clips, frames per clip, output row pitch (84)       */
    int len[AFX_CQT_PYR_LEVELS];   /* samples of every level (floorf(len/2) ladder)    */
    int valid[AFX_CQT_PYR_LEVELS]; /* framed samples of every level (stft_algorithm.c:838-843) */
    const unsigned short *timeKernelH; /* as AfxCqtOctaveArgs                           */
    const float *colMul, *scale;
    float octScale[AFX_CQT_PYR_LEVELS]; /* sqrt(2^k) of level k (cqt_algorithm.c:1218-1221)   */
    float *outRe, *outIm;    /* device [batch][T, num]                                  */
    long long outStride;
    float *ring;             /* device scratch, AFX_CQT_PYR_RING_FLOATS floats per workgroup */
    const unsigned short *decTab; /* device [AFX_CQT_PYR_TAB_HALFS]: the resampler taps h[|d|] 2^15 as f16 (hi, lo)
                              * words, d = -160 ... 167, four copies shifted by 0, 2, 4, 6 entries (afx_cqt_dec_table) */
    float decMul;            /* 2^-15 / sqrt(ratio): undoes the table scaling, applies the resampler's isScale   */
    int chunksPerClip, tilesPerChunk; /* work items: clip-major runs of tiles            */
    /* chroma in the same launch (chromaNum == 12 == bins per octave): NULL = off         */
    float *chroma;           /* device [batch][T, 12]                                   */
    int chromaClass[12];     /* class of bin j of an octave (the 0/1 folding matrix)    */
    int chromaMag, chromaNorm; /* |Q| instead of |Q|^2; 0 none 1 max 2 min 3 P2 4 P1     */
    unsigned long long *timing; /* NULL, or device [workgroups][11 waves][8]: shader cycles per phase, summed
                              * (the instrumented instantiation; tools/pyr_phases.py)      */
} AfxCqtPyramidArgs;
/* workgroups the launch will use (the caller sizes `ring` with it) */
int afxk_cqt_pyramid_plan(int batch, int timeLength, int maxTiles, int *chunksPerClip, int *tilesPerChunk);
int afxk_cqt_pyramid(const AfxCqtPyramidArgs *a, void *stream);
/* batch clips: x + b*xStride -> y + b*yStride */
int afxk_cqt_decimate(const float *x, int srcLen, long long xStride, float *y, int dstLen,
                      long long yStride, int batch, const float *taps32, float sqrtRatio,
                      void *stream);
/* cqhc / deconv: in[rows, num] -> timbre / pitch [rows, num] and/or hc [rows, hcNum]
 * (hcIdx[hcNum]: positions in the timbre sequence); transform length 2^radix2Exp >= 2 num;
 * twiddle: device [M/2] float2 */
int afxk_cqt_deconv(const float *in, long long rows, int num, int radix2Exp, const float *twiddle,
                    const int *hcIdx, int hcNum, float *outTimbre, float *outPitch, float *outHc,
                    void *stream);
/* the 0/1 folding matrix as per-class bin lists: class c owns bins[start[c] .. start[c+1]) in ascending order
 * (the order of the matrix product); chromaNum <= 64, num <= 255 (afx_cqt.c: afx_chroma_lists) */
typedef struct AfxChromaLists_ {
    unsigned short start[65];
    unsigned char bins[256];
} AfxChromaLists;
/* fold: device 0/1 matrix [chromaNum][num]; lists: the same as bin lists (host struct, a kernel argument of
 * k_cqt_chroma); NULL or a plan beyond the list form (num > 255, chromaNum > 64): the size-generic flag scan */
int afxk_cqt_chroma(const float *re, const float *im, long long rows, int num,
                    const unsigned char *fold, const AfxChromaLists *lists, int chromaNum, int isMag,
                    int normType, float *out, void *stream);

/* cepstrogram (afx_cepstrogram.hip): one clip, timeLength frames */
typedef struct {
    const float *x;      /* device samples, or NULL to start from specRe/specIm     */
    int timeLength, radix2Exp, hop, cepNum;
    const float *window; /* device [N]                                              */
    const float *twiddle;/* device [N/2] float2                                     */
    float *specRe;       /* device [T,N] spectrum cache: written when x != NULL     */
    float *specIm;       /*   (may be NULL), read when x == NULL                    */
    float *out1, *out2, *out3; /* device [T, N/2+1]; any may be NULL                */
    int framesPerClip;   /* > 0: timeLength counts the frames of several clips,      */
    long long clipStride;/*      frame f starts at x + (f / fpc) * clipStride + (f % fpc) * hop */
    const float *fastTab;/* device tables of the wave kernels for N = 2048 / 4096
                          * (afxk_cepstrogram_fast_tables), or NULL: size-generic kernel only */
} AfxCepstrogramArgs;
int afxk_cepstrogram(const AfxCepstrogramArgs *a, void *stream);
/* host: fills tab[AFX_CEPSTROGRAM_FASTTAB_FLOATS] for AfxCepstrogramArgs.fastTab (fftLength 2048 or 4096) */
#define AFX_CEPSTROGRAM_FASTTAB_FLOATS (2 * (16 * 64 + 72 + 1024 + 1025))
void afxk_cepstrogram_fast_tables(float *tab, int fftLength);

/* specialised rectify + DCT for cepstra (afx_cepstrum.hip): out[rows, ccNum] =
 * pre(in)[rows, num] . dct[ccNum, num]^T */
int afxk_cepstrum_supported(const float *in, int num, int ccNum);
int afxk_cepstrum(const float *in, long long rows, int num, const float *dct, int ccNum, int pre,
                  float *out, void *stream);

/* ---- fused STFT -> banded filter bank kernel (afx_melfused.hip) ---------- */

/* Banded view of a filter bank, one entry per lane of a 64-lane wave: every
 * lane owns up to two bank rows, a long one (A) and a short one (B); each row
 * is the contiguous bin range [start, start+len) that holds all its non-zero
 * weights.  Weight arrays are tap-major, [taps][64], zero padded. */
typedef struct {
    int num;        /* bank rows                                  */
    int tapsA;      /* longest A row                              */
    int tapsB;      /* longest B row                              */
    int startA[64];
    int startB[64];
    int rowA[64];   /* bank row stored by lane (-1: none)         */
    int rowB[64];
    float *wA;      /* host, [tapsA][64]                          */
    float *wB;      /* host, [tapsB][64]                          */
    /* split plans (afx_bandplan_build_split): a slot holds a SEGMENT of a row, rowA/rowB are -1
     * and bank row r is the sum of up to four slot results, in ascending bin order:
     * segIdx[r] packs four slot indices, 8 bits each, lowest byte first -- lane l's A slot is
     * l, its B slot 64 + l, 128 = none (contributes zero) */
    int split;
    unsigned segIdx[128];
} AfxBandPlan;

typedef struct {
    const float *x;
    long long clipStride;
    int batch, dataLength, timeLength, hop;
    int specMap;    /* 0 |S|^2, 1 |S|, 2 |S|^(2*normValue); complex results:
                     * 3 S, 4 S^2 (real plane -> out, imaginary plane -> outIm) */
    int postPow;    /* 1: powf(result, normValue)                           */
    float normValue;
    float *out;     /* device [batch*timeLength, num]                       */
    float *outIm;   /* device, same shape; complex result modes only        */
    /* optional fusions: cepstra (every fused kernel, real results) and temporal features (n_fft 2048); a run that cannot
     * honour them returns AFX_ERR_UNSUPPORTED and the caller takes the separate kernels */
    const float *dct; /* device [num, num] orthonormal DCT-II: cepstra of the rows in the same launch */
    int ccNum;        /*   first ccNum (<= 16) coefficients of the rectified rows; needs `out`           */
    int ccRectify;    /*   0: log10f(max(row, 1e-8)), 1: powf(row, 1/3) (xxcc_algorithm.c:124-137)        */
    float *cc;        /*   device [batch*timeLength, ccNum]                                          */
    float *energy, *rms, *zcr; /* device [batch*timeLength]: temporal features of the windowed frame */
} AfxMelFusedArgs;

/* One plan type and one create / run / destroy for the four transform sizes (afx_melfused.hip, afx_melplan.h); every size
 * (n_fft 512: afx_melfused512.hip, 1024: afx_melfused1k.hip, 2048: afx_melfused2.hip, 4096: afx_melfused4k2.hip) contributes
 * its tap variants, its table-fill function and its launchers.
 * afxk_melfused_variant: index into the size's variant table able to run (tapsA, tapsB), or -1 */
int afxk_melfused_variant(int radix2Exp, int tapsA, int tapsB);
int afxk_melfused_create(void **plan, int radix2Exp, const float *hWindow,
                         const AfxBandPlan *band, void *stream);
int afxk_melfused_run(void *plan, const AfxMelFusedArgs *a, void *stream);
void afxk_melfused_destroy(void *plan);
/* 0: no plan; otherwise 1: rows in whole slots, 2: split plan (row segments), plus the size's base -- 0 at n_fft 2048,
 * 100 at 1024, 200 at 4096, 300 at 512 (bftObj_fusedPlanKind: 1 / 2, 101 / 102, 201 / 202, 301 / 302) */
int afxk_melfused_kind(const void *plan);

/* How the fused kernels and their STFT instantiations spread `total` frames over the device: `rounds` rounds of workgroups
 * of `wavesPerWg` waves (one workgroup is resident per CU), every wave a contiguous run of *framesPerWave frames; returns
 * the workgroups to launch (0: nothing to do).  Long runs per wave (register re-use of the overlapping frames) once a round
 * of workgroups is full -- 1 / 2 / 3 rounds measure the same at the headline size (1.558 / 1.559 / 1.559 ms per step), 6
 * rounds + 1.2 %, two keep the tail short.  A call that cannot fill one round with 16-frame runs -- the one-clip legacy
 * entry points: 1000 frames -- is spread over all CUs instead (16 frames in sequence per wave were 75 us of a 1000-frame
 * call's 190, profiles/r05_legacy_phases.txt).  Shared with the host tests (tests/test_bandplan.py).
 * n_fft 2048 (afx_melfused2.hip, round 7) takes only the workgroups' ranges from here -- workgroup b owns the frames
 * [b, b + 1) x wavesPerWg x *framesPerWave -- in ONE round: inside a range no wave owns a share, the waves claim runs of frames
 * from a counter in LDS, so that none of the twelve leaves its SIMD long before the others (profiles/r07_ab_headline.txt).  The
 * kernels of n_fft 512, 1024 and 4096 keep the fixed share per wave. */
static inline long long afx_frame_split(long long total, int cus, int wavesPerWg, int rounds, long long *framesPerWave) {
    *framesPerWave = 0;
    if (total <= 0) return 0;
    const long long oneRoundWaves = (long long)cus * wavesPerWg, waves = oneRoundWaves * rounds;
    long long fpw = (total + waves - 1) / waves;
    if (fpw < 16) {
        const long long oneRound = (total + oneRoundWaves - 1) / oneRoundWaves;
        fpw = oneRound < 16 ? oneRound : 16;
    }
    const long long usedWaves = (total + fpw - 1) / fpw;
    *framesPerWave = fpw;
    return (usedWaves + wavesPerWg - 1) / wavesPerWg;
}

/* ---- spectral descriptors (afx_descriptors.hip) ---------------------------- */
/* descriptor kinds in the order of AfxSpectralKind (include/afx_batch.h) */
enum {
    AFX_DESC_FLATNESS = 0, AFX_DESC_FLUX, AFX_DESC_ROLLOFF, AFX_DESC_CENTROID, AFX_DESC_SPREAD, AFX_DESC_SKEWNESS,
    AFX_DESC_KURTOSIS, AFX_DESC_ENTROPY, AFX_DESC_CREST, AFX_DESC_SLOPE, AFX_DESC_DECREASE, AFX_DESC_BANDWIDTH,
    AFX_DESC_RMS, AFX_DESC_ENERGY, AFX_DESC_HFC, AFX_DESC_SD, AFX_DESC_SF, AFX_DESC_MKL, AFX_DESC_PD, AFX_DESC_WPD,
    AFX_DESC_NWPD, AFX_DESC_CD, AFX_DESC_RCD, AFX_DESC_BROADBAND, AFX_DESC_NOVELTY, AFX_DESC_EEF, AFX_DESC_EER,
    AFX_DESC_MAX, AFX_DESC_MEAN, AFX_DESC_VAR, AFX_DESC_COUNT
};
/* one request: its parameters in the order of the reference prototype, and the first output slot it writes */
typedef struct {
    int kind;
    int iarg[4];
    float farg[2];
    int slot;
} AfxDescReq;

typedef struct {
    const float *spec;   /* device [rows, num]                                                        */
    const float *phase;  /* device [rows, num]; pd / wpd / nwpd / cd / rcd only                       */
    float *out;          /* device: request r writes out[(slot + k) * outStride + row]                */
    long long rows, outStride;
    int framesPerClip;   /* > 0: frame-difference descriptors restart every framesPerClip rows        */
    int num;             /* row pitch                                                                 */
    int start, len;      /* the edge: bins start .. start + len - 1, or idx[0 .. len - 1]             */
    const int *idx;      /* device index table (any order, repeats allowed), NULL for a range         */
    int idx0;            /* first bin of the edge (idx[0] or start)                                   */
    const float *fre;    /* device [num]                                                              */
    /* per-edge constants, summed on the host in the reference's order (spectral_algorithm.c:1100-1140,
     * :1040-1075, flux_spectral.c:353-360): mean of fre over the edge, sum (fre - mean)^2, that / (len - 1) */
    float meanFre, slopeDen, varFre;
    int isPower;         /* AFX_DESC_ENERGY: the rows are power already (spectrogram object, dataType Power) */
    const AfxDescReq *req; /* host; at most one request per kind in a launch */
    int count;
} AfxDescArgs;
/* Row-local kinds in one launch that fetches every row once (rows up to 1024 edge bins stay in registers, longer ones are
 * read a second time while they sit in L2), frame-difference kinds in a second launch on the same stream.  AFX_ERR_ARG
 * for a bad kind, two requests of one kind, or a phase kind without `phase`. */
int afxk_descriptors(const AfxDescArgs *a, void *stream);
/* out[r, j] = in[r, j] / value, halved at j == 0 and j == halfBin (spectrogram_algorithm.c:2080-2120); in == out allowed */
int afxk_desc_preprocess(const float *in, float *out, long long rows, int num, float value, int halfBin, void *stream);

/* ---- harmonic / percussive separation (afx_hpss.hip) ----------------------- */
typedef struct {
    const float *re, *im;  /* device half spectrum [rows, pitch]: bins 0 .. cols - 1 of every frame               */
    long long rows;        /* clips * framesPerClip (the last clip may be shorter)                                */
    int framesPerClip;     /* > 0: a median along time never reads across a clip boundary                         */
    int cols, pitch;       /* bins per frame (fftLength / 2 + 1 when spectra are stored), floats between rows     */
    int hOrder, pOrder;    /* odd, 1 ... 63: window along time / along frequency; zeros outside the clip's plane  */
    int fftLength;
    float *hRe, *hIm;      /* device [rows, fftLength] or NULL: the harmonic spectrum with its Hermitian mirror   */
    float *pRe, *pIm;      /* the percussive one                                                                  */
    float *hMag, *pMag;    /* device [rows, cols] or NULL: the masked magnitudes                                  */
} AfxHpssArgs;
/* mag = sqrtf(re^2 + im^2); h, p = medians of mag along time / frequency; H = h^2 / max(h^2 + p^2, 1e-16) mag, P likewise;
 * spectra = H, P times the unit phase (re, im) / max(mag, 1e-16) (hpss_algorithm.c:168-300).  One launch, nothing but the
 * requested outputs is written.  AFX_ERR_UNSUPPORTED for an order it does not cover. */
int afxk_hpss_mask(const AfxHpssArgs *a, void *stream);
/* out[r, c] = median of the odd `order` values of in [rows, cols] around (r, c) along axis 0 (rows, inside the clip of
 * framesPerClip rows; 0: one clip) or axis 1, zeros outside; exact selection.  Orders up to AFX_MEDIAN_FAST_ORDER keep the
 * window sorted in registers, up to AFX_MEDIAN_MAX_ORDER a rank-counting kernel runs; beyond: AFX_ERR_UNSUPPORTED */
#define AFX_MEDIAN_FAST_ORDER 63
#define AFX_MEDIAN_MAX_ORDER 255
int afxk_median_filter(const float *in, long long rows, int cols, int framesPerClip, int axis, int order, float *out, void *stream);

/* ---- YIN pitch tracking (afx_pitch_yin.hip) -------------------------------- */
typedef struct {
    const float *x;        /* device, clip b starts at x + b * clipStride                                         */
    long long clipStride;  /* in samples                                                                          */
    int batch, dataLength; /* clips, samples per clip                                                             */
    int timeLength;        /* frames per clip: (dataLength - fftLength) / hop + 1 > 0                             */
    int radix2Exp, hop;    /* fftLength = 2^radix2Exp, 6 ... 13; hop > 0 (may exceed fftLength)                   */
    int autoLength;        /* 0 ... fftLength - 1: the correlation sums autoLength + 1 products                   */
    int minIndex, maxIndex; /* lags of the curve: 1 <= minIndex, minIndex + 2 <= maxIndex <= fftLength - autoLength - 1 */
    int samplate;
    float thresh;
    const float *twiddle;  /* device float2 (cos, -sin)(2 pi m / fftLength), m < fftLength / 2                    */
    float *fre, *trough, *minv; /* device [b * outStride + t] or NULL: 0 in fre / trough where no trough qualifies */
    long long outStride;
    float *candFre, *candVal; /* device [row * candPitch + i], row = b * timeLength + t, or NULL (both or none)    */
    int *candLen;          /* device [row]: all qualifying troughs of the frame; the first candPitch are stored    */
    int candPitch;
    float *curve;          /* device [row * yinLength + k], yinLength = maxIndex - minIndex + 1, or NULL           */
} AfxPitchYinArgs;
/* One launch from samples to results (_pitch_yin.c:352-603): difference function by an FFT autocorrelation, cumulative-mean
 * normalisation, first trough below thresh with its parabolic offset, min of the curve; optionally the candidate lists and
 * the curve.  One workgroup per frame, everything between the samples and the outputs stays in LDS and registers.
 * AFX_ERR_ARG for a plan outside the limits above, AFX_ERR_UNSUPPORTED beyond 2^31 - 1 frames in a launch. */
int afxk_pitch_yin(const AfxPitchYinArgs *a, void *stream);

/* ---- non-stationary Gabor transform (afx_nsgt.hip) ------------------------- */
#define AFX_NSGT_TILE 512  /* spectrum values (and twiddles) of a band one wave keeps in LDS; longer bands tile k */
#define AFX_NSGT_BLOCK 256 /* outputs n of one work item: 4 accumulators per lane */
typedef struct {
    int len;      /* L: window length = length of the band's inverse DFT = its cells                  */
    int offset;   /* first spectrum bin under the window (reads are clamped to 0 ... N - 1)           */
    int cell;     /* start of the band's cells in [totalLength]; its windows start there too          */
    int twiddle;  /* start (in float2) of the length's table T_L[m] = (cos, sin)(2 pi m / L), m < L   */
    int cellCol;  /* start of the band's L + 1 entries in cellCol: entry n = first matrix column whose
                   * cell index is >= n (entry L = maxLength)                                          */
} AfxNsgtBand;
typedef struct {
    int r1, r2;              /* N = 2^(r1 + r2); frequency k of chunk c at Xt[c][k & (2^r1 - 1)][k >> r1]  */
    int num, maxLength, totalLength;
    const AfxNsgtBand *bands;   /* device [num]                                                            */
    const int *items;        /* device [nItems][2]: (band, first output n of the block), long bands first  */
    int nItems;
    const float *window;     /* device [totalLength]                                                       */
    const float *twiddle;    /* device float2 tables, one per distinct length                              */
    const int *colMap;       /* device [num][maxLength]: cell index (0 ... L - 1) each matrix column holds  */
    const int *cellCol;      /* device: see AfxNsgtBand                                                    */
    const float *Xt;         /* device [chunks][N] complex: afxk_nsgt_spectrum's result                    */
    int chunks;              /* <= 65535 per launch                                                        */
    float *outRe, *outIm;    /* device [chunks][num][maxLength]: every element is written                   */
    float *cellRe, *cellIm;  /* device [chunks][totalLength], or both NULL: not stored                      */
} AfxNsgtArgs;
/* `chunks` real signals of N = 2^(r1 + r2) samples, chunk c at x + c xStride -> their full complex spectra
 * Xt[c][k1][k2] (TRANSPOSED layout: frequency k1 + 2^r1 k2 at [k1][k2]); scratchA: chunks * N complex.  The forward pass
 * of the CWT (afxk_cwt_forward, pad 0) under a name of its own.  d: r1, r2, dataLength = N, pad 0, tileCols. */
int afxk_nsgt_spectrum(const AfxCwtPlanDims *d, const float *tw, const float *x, long long xStride, int chunks,
                       float *scratchA, float *Xt, void *stream);
/* per band and chunk: window multiply on the spectrum slice, rotation by L - L / 2, inverse DFT of the band's own length
 * L (any L >= 1), 1 / L, cell store, and the sample-and-hold gather into the matrix row -- one launch, one wave per
 * (band, chunk, block of AFX_NSGT_BLOCK outputs).  AFX_ERR_ARG for a NULL plan / output, AFX_ERR_UNSUPPORTED beyond the
 * launch limits (chunks > 65535). */
int afxk_nsgt_bands(const AfxNsgtArgs *a, void *stream);

/* ---- harmonic product / log-harmonic sum pitch tracking (afx_pitch_hs.hip) -- */
#define AFX_PITCH_HPS 0 /* curve[j] = prod_k |X[j (k + 1)]|     */
#define AFX_PITCH_LHS 1 /* curve[j] = sum_k log |X[j (k + 1)]| */
#define AFX_PITCH_HS_LDS_BUDGET (160 * 1024) /* LDS one workgroup may declare on gfx950 */
#define AFX_PITCH_HS_SCRATCH_GROUPS 1024     /* workgroups of a launch whose spectrum slice lives in device scratch */
/* floats of a spectrum slice that holds bins 0 ... lastBin: one float of padding per 32 keeps the stride M / fftLength of
 * a residue's bins off a single LDS bank */
static inline long long afx_pitch_hs_slice_floats(long long lastBin) { return lastBin + (lastBin >> 5) + 1; }
/* LDS bytes of a workgroup without the slice: cross-wave exchange, transform buffer (afx_ldsfft.h padding), windowed frame */
static inline long long afx_pitch_hs_lds_fixed(int radix2Exp) {
    const long long n = 1LL << radix2Exp;
    return 128 + 8 * (n + (n >> 5) + 1) + 4 * n;
}
typedef struct {
    const float *x;        /* device, clip b starts at x + b * clipStride                                         */
    long long clipStride;  /* in samples                                                                          */
    int batch, dataLength; /* clips, samples per clip                                                             */
    int timeLength;        /* frames per clip: (dataLength - fftLength) / hop + 1 > 0                             */
    int kind;              /* AFX_PITCH_HPS / AFX_PITCH_LHS                                                       */
    int radix2Exp, hop;    /* fftLength = 2^radix2Exp, 6 ... 13; hop > 0 (may exceed fftLength)                   */
    int interpExp;         /* M = 2^interpExp >= fftLength: the zero-padded transform length                      */
    int minIndex, maxIndex; /* candidates: 0 <= minIndex <= maxIndex                                              */
    int harmonicCount;     /* >= 1, maxIndex * harmonicCount < M                                                  */
    double freStep;        /* 1.0 * samplate / M                                                                  */
    const float *window;   /* device [fftLength]                                                                  */
    const float *twiddle;  /* device float2 (cos, -sin)(2 pi m / fftLength), m < fftLength / 2                    */
    const float *roots;    /* device float2 (cos, -sin)(2 pi m / M), m < M                                        */
    float *slice;          /* device scratch [groups][afx_pitch_hs_slice_floats(maxIndex * harmonicCount)], or NULL:
                            * the slice lives in LDS                                                              */
    int groups;            /* workgroups of the launch when slice != NULL (<= AFX_PITCH_HS_SCRATCH_GROUPS)        */
    float *fre, *value;    /* device [b * outStride + t] or NULL                                                  */
    long long outStride;
    float *curve;          /* device [row * (maxIndex + 1) + j], row = b * timeLength + t, or NULL                */
} AfxPitchHsArgs;
/* One launch from samples to results (_pitch_hps.c:415-518, _pitch_lhs.c:416-532): window, the needed bins of the
 * M-point spectrum of the zero-padded frame as M / fftLength modulated fftLength-point transforms in LDS (half of them:
 * the frame is real), the harmonic product / log-sum over 0 ... maxIndex, the first argmax over minIndex ... maxIndex.
 * One workgroup per frame (a fixed number of workgroups striding over the frames when the slice lives in scratch).
 * AFX_ERR_ARG for a plan outside the limits above, AFX_ERR_UNSUPPORTED beyond 2^31 - 1 frames in a launch. */
int afxk_pitch_hs(const AfxPitchHsArgs *a, void *stream);

/* ---- pitch-estimation-filter tracking (afx_pitch_pef.hip) ------------------- */
#define AFX_PITCH_PEF_MIN_EXP 6
#define AFX_PITCH_PEF_MAX_EXP 12 /* 13: 167 KB of LDS for a plan that reads every bin, above the 160 KB of a gfx950 CU */
/* one entry of the log grid: y[m] = (index < 0 ? pw[N] : pw[index] + dx * (pw[index + 1] - pw[index]) / dl) * bw, the
 * operands of __vinterp_linear (flux_vectorOp.c:580-610) precomputed in float32 */
typedef struct __attribute__((aligned(16))) { /* one 16-byte load */
    int index;  /* 0 ... N - 1, or -1: past the last linear frequency */
    float dx;   /* lg[m] - lin[index]            */
    float dl;   /* lin[index + 1] - lin[index]   */
    float bw;   /* bandWidthArr[m]               */
} AfxPitchPefTap;
/* LDS bytes of a workgroup: cross-wave exchange, the 2N-point complex transform buffer (afx_ldsfft.h padding), and the
 * pwLength <= N + 1 bins of the power spectrum the log grid reads (rounded up to 16 bytes) */
static inline long long afx_pitch_pef_lds_bytes(int radix2Exp, int pwLength) {
    const long long n = 1LL << radix2Exp;
    return 128 + 8 * (2 * n + (2 * n >> 5) + 1) + 4 * (((long long)pwLength + 3) & ~3LL);
}
typedef struct {
    const float *x;        /* device, clip b starts at x + b * clipStride                                         */
    long long clipStride;  /* in samples                                                                          */
    int batch, dataLength; /* clips, samples per clip                                                             */
    int timeLength;        /* frames per clip: (dataLength - fftLength) / hop + 1 > 0                             */
    int radix2Exp, hop;    /* N = fftLength = 2^radix2Exp, 6 ... 12; hop > 0 (may exceed fftLength)               */
    int minIndex, maxIndex; /* candidates: 0 <= minIndex <= maxIndex < 2N                                         */
    int filterPadNum;      /* 0 ... N: zeros in front of the log spectrum                                         */
    int pwLength;          /* bins 0 ... pwLength - 1 of the power spectrum are kept: every taps[m].index + 2 <=
                            * pwLength <= N + 1, and N + 1 when an index is -1                                    */
    const float *window;   /* device [N]                                                                          */
    const float *twiddle;  /* device float2 (cos, -sin)(2 pi m / 4N), m < 2N                                      */
    const AfxPitchPefTap *taps; /* device [2N], 16-byte aligned                                                   */
    const float *filterSpec; /* device float2 [2N + 1]: conj of the 4N-point spectrum of h, bins 0 ... 2N, times 1 / 2N */
    const float *lg;       /* device [2N]: the log frequencies                                                    */
    float *fre, *value;    /* device [b * outStride + t] or NULL                                                  */
    long long outStride;
    float *curve;          /* device [row * (maxIndex + 1) + k], row = b * timeLength + t, or NULL                */
} AfxPitchPefArgs;
/* One launch from samples to results (_pitch_pef.c:258-426): window, power spectrum of the frame zero-padded to 2N points
 * (an N-point complex transform and the real split), interpolation onto the log grid, the correlation with the filter as
 * a 4N-point real one (two 2N-point complex transforms around a product with filterSpec), the first argmax over
 * minIndex ... maxIndex.  Workgroups stride over the (clip, frame) rows; everything between the samples and the outputs
 * stays in LDS and registers.  AFX_ERR_ARG for a plan outside the limits above, AFX_ERR_UNSUPPORTED beyond 2^31 - 1 frames
 * in a launch. */
int afxk_pitch_pef(const AfxPitchPefArgs *a, void *stream);

/* ---- lag-domain pitch tracking: NCF and cepstrum (afx_pitch_lag.hip) -------- */
#define AFX_PITCH_LAG_MIN_EXP 6
#define AFX_PITCH_LAG_MAX_EXP 12 /* 13: a 16384-point complex buffer, 128 KB of LDS, one workgroup per CU */
#define AFX_PITCH_LAG_NCF 0      /* curve from |X|^2: the normalised autocorrelation      */
#define AFX_PITCH_LAG_CEP 1      /* curve from ln |X|^2: the real cepstrum                 */
/* LDS bytes of a workgroup: cross-wave exchange and the 2N-point complex transform buffer (afx_ldsfft.h padding) */
static inline long long afx_pitch_lag_lds_bytes(int radix2Exp) {
    const long long n = 1LL << radix2Exp;
    return 256 + 8 * (2 * n + (2 * n >> 5) + 1);
}
typedef struct {
    const float *x;        /* device, clip b starts at x + b * clipStride                                         */
    long long clipStride;  /* in samples                                                                          */
    int batch, dataLength; /* clips, samples per clip                                                             */
    int timeLength;        /* frames per clip: (dataLength - fftLength) / hop + 1 > 0                             */
    int radix2Exp, hop;    /* N = fftLength = 2^radix2Exp, 6 ... 12; hop > 0 (may exceed fftLength)               */
    int mode;              /* AFX_PITCH_LAG_NCF / AFX_PITCH_LAG_CEP                                               */
    int samplate;          /* fre = samplate / (index + 1)                                                        */
    int minIndex, maxIndex; /* candidates: 1 (CEP: 0) <= minIndex <= maxIndex <= N - 1 (CEP: 2N - 1)              */
    const float *window;   /* device [N], or NULL: the rectangular window, no multiply                            */
    const float *twiddle;  /* device float2 (cos, -sin)(2 pi m / 2N), m < N                                       */
    float *fre, *value;    /* device [b * outStride + t] or NULL                                                  */
    long long outStride;
    float *curve;          /* device [row * (maxIndex + 1) + k], row = b * timeLength + t, or NULL                */
} AfxPitchLagArgs;
/* One launch from samples to results (_pitch_ncf.c:380-494, _pitch_cep.c:381-474): window, the 2N-point spectrum of the
 * frame zero-padded to 2N, |X|^2 or ln |X|^2 in place, the inverse as a forward transform of that real, even sequence,
 * NCF's normalisation by its own lag 0, the first argmax over minIndex ... maxIndex, fre = samplate / (index + 1).  One
 * workgroup per frame; everything between the samples and the outputs stays in LDS and registers.  AFX_ERR_ARG for a plan
 * outside the limits above, AFX_ERR_UNSUPPORTED beyond 2^31 - 1 frames in a launch. */
int afxk_pitch_lag(const AfxPitchLagArgs *a, void *stream);

/* ---- harmonic ratio (afx_harmonic_ratio.hip) -------------------------------- */
/* the window exponents are those of the lag kernel: the same L = 2N-point LDS transform, the same LDS bytes */
#define AFX_HARMONIC_RATIO_NONE (-1) /* frames[row]: the frame found no zero crossing of its own */
/* ints of the scratch a launch over `rows` frames needs: frames [rows], list [rows], count [1] */
static inline long long afx_harmonic_ratio_scratch_ints(long long rows) { return 2 * rows + 1; }
typedef struct {
    const float *x;        /* device, clip b starts at x + b * clipStride                                         */
    long long clipStride;  /* in samples                                                                          */
    int batch, dataLength; /* clips, samples per clip                                                             */
    int timeLength;        /* frames per clip: (dataLength - N) / hop + 1 > 0                                     */
    int radix2Exp, hop;    /* N = windowLength = 2^radix2Exp, 6 ... 12; hop > 0 (may exceed N)                    */
    int maxLength;         /* 2 <= maxLength <= N - 1: lags 1 ... maxLength - 1 are candidates                    */
    const float *window;   /* device [N]                                                                          */
    const float *twiddle;  /* device float2 (cos, -sin)(2 pi m / 2N), m < N                                       */
    int *scratch;          /* device [afx_harmonic_ratio_scratch_ints(batch * timeLength)]                        */
    float *value;          /* device [b * outStride + t] or NULL                                                  */
    int *lag, *first;      /* device [b * outStride + t] or NULL: the chosen lag (-1: none), the minIndex used    */
    long long outStride;
    float *curve;          /* device [row * maxLength + j], row = b * timeLength + t, or NULL                     */
} AfxHarmonicRatioArgs;
/* Samples to results (harmonicRatio_algorithm.c:172-287) in three stream-ordered launches: every frame with its own first
 * zero crossing (a frame without one assumes minIndex 0 and records NONE); per clip, the minIndex each such frame inherits
 * from the nearest earlier frame that found one, and the list of frames for which that is not 0; those frames again with
 * minIndex given.  One workgroup per frame in the first launch; everything between the samples and the outputs stays in
 * LDS and registers.  AFX_ERR_ARG for a plan outside the limits above, AFX_ERR_UNSUPPORTED beyond 2^31 - 1 frames. */
int afxk_harmonic_ratio(const AfxHarmonicRatioArgs *a, void *stream);

/* ---- onset detection (afx_onset.hip) ---------------------------------------- */
/* frames of one clip's envelope the picker keeps in LDS (32 KB: four workgroups of a CU keep theirs); a longer clip is
 * picked from global memory (the envelope the same workgroup wrote, or the caller's) */
#define AFX_ONSET_LDS_FRAMES 8192
/* floats of a tile of whole rows the max filter keeps in LDS; a longer row is filtered from global memory (its second
 * read finds it in L2) */
#define AFX_ONSET_FILTER_TILE 2048
/* out[r, j] = max of in[r, max(j - order / 2, 0) ... min(j - 1 + order - order / 2, cols - 1)] (__vmaxfilter,
 * flux_vector.c:3063-3081), order >= 1 (any size: the window is cut at the row's ends); in != out.  Exact. */
int afxk_max_filter(const float *in, long long rows, int cols, int order, float *out, void *stream);
typedef struct {
    const float *src;      /* device: clip b's values at src + b * srcStride                                      */
    long long srcStride;
    int batch, length;     /* clips, frames per clip (> 0)                                                        */
    int normalise;         /* 1: e = src - min(src), then e / max(e) when that is > 0 (onset_algorithm.c:379-385),
                            * stored to evn; 0: e = src                                                           */
    float *evn;            /* device [b * evnStride + t], normalise only                                          */
    long long evnStride;
    int preMax, postMax, preAvg, postAvg, wait; /* preMax, preAvg, wait >= 0; postMax, postAvg >= 1               */
    float delta;
    int *point;            /* device [b * pointStride + k] or NULL: the first pointStride points of a clip        */
    int *count;            /* device [b] or NULL: all points of the clip                                          */
    long long pointStride;
} AfxOnsetPickArgs;
/* One workgroup per clip, one launch: (min, max, normalise,) the candidates of __peakPick (onset_algorithm.c:423-460) --
 * e[i] == max of its window, e[i] >= float32 mean of its window summed in index order + delta -- per tile of frames in
 * parallel, compacted in order, and the wait rule over the candidates alone.  AFX_ERR_ARG outside the limits above. */
int afxk_onset_pick(const AfxOnsetPickArgs *a, void *stream);
/* out[b * stride + i] = max(10 log10f(in[b * stride + i] / max_i in[b * stride + i]), min), i < length
 * (util_powerToDB, flux_util.c:549-571; min as given: the caller applied the >= 0 -> -80 rule): partial maxima of every
 * clip (at most 32 per clip, in stream-ordered scratch that is released on the stream), then the map.  in == out
 * allowed. */
int afxk_power_to_db(const float *in, int batch, long long length, long long stride, float min, float *out, void *stream);

/* ---- fast S-transform (afx_fst.hip) ----------------------------------------- */
#define AFX_FST_MIN_EXP 4  /* the forward pass (afxk_nsgt_spectrum) starts at 2^4 */
#define AFX_FST_MAX_EXP 14 /* the longest band, 2^12 points, is 33 KB of LDS */
/* outputs of one launch above this many bytes are stored non-temporally: the L2 caches of the device hold 32 MB */
#define AFX_FST_STREAM_BYTES (32ll << 20)
typedef struct {
    int r1, r2;              /* N = 2^(r1 + r2); frequency k of chunk c at Xt[c][k & (2^r1 - 1)][k >> r1]  */
    const float *Xt;         /* device [chunks][N] complex: afxk_nsgt_spectrum's result                    */
    const float *twiddle;    /* device float2 (cos, -sin)(2 pi m / N), m < N / 2: the forward pass's table  */
    int chunks;              /* <= 65535 per launch                                                        */
    float scale[16];         /* entry b: 1 / sqrt(N 2^b), the net scale of the band of 2^b points (0: singles) */
    float *cellRe, *cellIm;  /* device [chunks][N / 2 + 1]: bin -1, DC, bin +1, band 2, band 4, ..., band N / 4 */
} AfxFstCellArgs;
/* the visible cells of every chunk: the three single bins as scaled copies, and per positive band of n = 2, 4, ..., N / 4
 * points (bins n ... 2n - 1) its n-point inverse transform in LDS, the (-1)^k sign of the shifted spectrum and both
 * half-rotations folded into the indices -- one launch, one workgroup per (band, chunk).  AFX_ERR_ARG for a NULL
 * pointer or N outside 2^AFX_FST_MIN_EXP ... 2^AFX_FST_MAX_EXP, AFX_ERR_UNSUPPORTED for chunks > 65535. */
int afxk_fst_cells(const AfxFstCellArgs *a, void *stream);
typedef struct {
    int radix2Exp;           /* N = 2^radix2Exp columns                                                    */
    int minIndex, rows;      /* output row k shows index minIndex + k; 0 <= minIndex, minIndex + rows <= N / 2 + 1 */
    int chunks;              /* <= 65535 per launch                                                        */
    const int *rowMap;       /* device [N / 2 + 1][2]: (first cell, shift) of an index: column l holds cell first + (l >> shift) */
    const float *cellRe, *cellIm; /* device [chunks][N / 2 + 1]                                            */
    float *outRe, *outIm;    /* device [chunks][rows][N], any 4-byte alignment: every element is written   */
} AfxFstExpandArgs;
/* the sample-and-hold of the cells onto the N-column grid: each lane stores 4 consecutive columns of both planes (one
 * value each: a cell repeats at least 4 times), 16 bytes a store where the plane is 16-byte aligned, dwords otherwise;
 * non-temporal above AFX_FST_STREAM_BYTES.  AFX_ERR_ARG outside the limits above, AFX_ERR_UNSUPPORTED for chunks > 65535. */
int afxk_fst_expand(const AfxFstExpandArgs *a, void *stream);

/* ---- S-transform (afx_st.hip); sizes and the streaming threshold are the FST's -- */
typedef struct {
    int r1, r2;              /* N = 2^(r1 + r2); frequency k of chunk c at Xt[c][k & (2^r1 - 1)][k >> r1]  */
    const float *Xt;         /* device [chunks][N] complex: afxk_nsgt_spectrum's result                    */
    const float *twiddle;    /* device float2 (cos, -sin)(2 pi m / N), m < N / 2: the forward pass's table  */
    const float *coef;       /* device [N / 2 + 1]: c_k = -factor 2 pi^2 / k^(2 norm) (entry 0 is not read) */
    const int *bins;         /* device [rows]: the bin k of every output row, each in 0 ... N / 2          */
    int rows;                /* 1 ... 2^31 - 1: one workgroup per (row, chunk)                              */
    int chunks;              /* <= 65535 per launch                                                        */
    float *outRe, *outIm;    /* device [chunks][rows][N], any 4-byte alignment: every element is written   */
} AfxStArgs;
/* row i of chunk c = ifft_j(X[(k + j) mod N] W_k[j]) with k = bins[i] and W_k[j] = expf(c_k j^2) + expf(c_k (j - N)^2)
 * evaluated in the kernel (float: j^2 rounded, one multiply, expf, one add -- the sequence of st_algorithm.c:227-243); k = 0:
 * Re X[0] / N in every column, zeros in the imaginary plane.  The N-point transform runs in LDS (afx_ldsfft.h, skewed:
 * 8 afx_lds_padded_size(N) bytes, 135 KB at 2^14); 16 bytes a store where both planes are 16-byte aligned, dwords otherwise;
 * non-temporal above AFX_FST_STREAM_BYTES.  AFX_ERR_ARG for a NULL pointer, rows <= 0 or N outside 2^AFX_FST_MIN_EXP ...
 * 2^AFX_FST_MAX_EXP, AFX_ERR_UNSUPPORTED for chunks > 65535. */
int afxk_st_rows(const AfxStArgs *a, void *stream);

/* ---- band-limited resampling (afx_resample.hip) ------------------------------ */
#define AFX_RESAMPLE_TILE 512                  /* outputs of one work item = threads of a workgroup: a lane owns one output */
#define AFX_RESAMPLE_GROUP 4                   /* clips of one work item at most: a weight is computed once for all of them */
#define AFX_RESAMPLE_LDS_BUDGET (160 * 1024)   /* LDS one workgroup may declare on gfx950 */
#define AFX_RESAMPLE_MAX_TABLE (1 << 24)       /* entries of the table a constructor accepts: 64 MB of device memory */
/* what output i reads (resample_algorithm.c:483-511): the sample n under it, and per side the first table entry and the
 * weight of the next one.  t is ONE float64 division rounded to float32, factor and scale - factor single float32
 * roundings (no fused multiply-add: the pragma); factor * bitLength is exact, so offset and delta are. */
typedef struct {
    int n;               /* floorf(t), t = (float)(i / ratio): may reach sourceLength and beyond when dataLength * ratio rounded up */
    int offL, offR;      /* first table entry of the left taps x[n - j] and of the right taps x[n + 1 + j] */
    float deltaL, deltaR;
} AfxResamplePhase;
AFX_HD static inline AfxResamplePhase afx_resample_phase(long long i, float ratio, float scale, int bitLength) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    AfxResamplePhase p;
    const float t = (float)((double)i / (double)ratio);
    const float fn = floorf(t);
    float factor = scale * (t - fn);
    float fv = factor * (float)bitLength;
    float fo = floorf(fv);
    p.n = (int)fn;
    p.offL = (int)fo;
    p.deltaL = fv - fo;
    factor = scale - factor;
    fv = factor * (float)bitLength;
    fo = floorf(fv);
    p.offR = (int)fo;
    p.deltaR = fv - fo;
    return p;
}
/* min(1, ratio) and floorf(scale * bitLength): the table entries between two taps (resample_algorithm.c:455-456) */
AFX_HD static inline float afx_resample_scale(float ratio) { return 1.0 > ratio ? ratio : 1.f; }
AFX_HD static inline int afx_resample_step(float ratio, int bitLength) { return (int)floorf(afx_resample_scale(ratio) * (float)bitLength); }
typedef struct {
    const float *x;        /* device, clip b starts at x + b * clipStride                                         */
    long long clipStride;  /* in samples, >= sourceLength when batch > 1                                          */
    int batch;
    int sourceLength;      /* samples per clip, > 0                                                               */
    int targetLength;      /* outputs per clip, > 0                                                               */
    float ratio;           /* targetRate / sourceRate as the object holds it; floorf(min(1, ratio) * bitLength) >= 1 */
    int bitLength;         /* table entries per zero crossing, a power of two                                     */
    int interpLength;      /* zeroNum * bitLength + 1                                                             */
    const float *table;    /* device [interpLength + 1]: the table (times ratio when that is < 1), its last entry
                            * repeated -- the difference table's last entry is 0 (resample_algorithm.c:543)       */
    float outScale;        /* every output is divided by it: sqrtf(ratio) with isScale, else 1                    */
    float *out;            /* device [b * outStride + i], i < targetLength: overwritten                           */
    long long outStride;   /* >= targetLength when batch > 1                                                      */
} AfxResampleArgs;
/* What the launcher decides from the ratio and the table's size, without a device: where the table lives, how many clips a
 * work item covers, how much of the input it stages. */
typedef struct {
    int tableInLds;       /* the table and its repeated last entry live in LDS                                    */
    int group;            /* 1, 2 or AFX_RESAMPLE_GROUP clips per work item                                       */
    int spanFloats;       /* staged input samples per clip (0: the taps read global memory)                       */
    long long ldsBytes;   /* of one workgroup                                                                     */
    int taps;             /* taps per side at most: interpLength / step                                           */
} AfxResampleLaunch;
static inline int afx_resample_launch_plan(int batch, float ratio, int bitLength, int interpLength, AfxResampleLaunch *l) {
    const int step = afx_resample_step(ratio, bitLength);
    if (step < 1 || interpLength < 2 || !(ratio > 0)) return AFX_ERR_ARG;
    l->taps = interpLength / step;
    const long long tabBytes = ((4ll * (interpLength + 1)) + 15) & ~15ll;
    /* samples under one tile of outputs, both sides' taps, and slack for the float32 rounding of t near the tile's ends */
    const double under = (double)(AFX_RESAMPLE_TILE - 1) / (double)ratio;
    const double span = under + 2.0 * l->taps + 8.0;
    l->tableInLds = tabBytes <= AFX_RESAMPLE_LDS_BUDGET;
    const long long left = AFX_RESAMPLE_LDS_BUDGET - (l->tableInLds ? tabBytes : 0);
    l->group = batch >= AFX_RESAMPLE_GROUP ? AFX_RESAMPLE_GROUP : (batch >= 2 ? 2 : 1);
    l->spanFloats = 0;
    if (4.0 * span <= (double)left) { /* one clip's span fits: as many clips as fit beside it */
        const long long s = (((long long)span) + 3) & ~3ll;
        while (l->group > 1 && 4 * s * l->group > left) l->group >>= 1;
        if (4 * s * l->group <= left) l->spanFloats = (int)s;
    }
    if (!l->spanFloats) l->group = 1;
    l->ldsBytes = (l->tableInLds ? tabBytes : 0) + 4ll * l->spanFloats * l->group;
    if (l->ldsBytes < 16) l->ldsBytes = 16;
    return AFX_OK;
}
/* Every output of every clip in one launch (resample_algorithm.c:430-521, the isScale division of :387-396 in the store):
 * out[i] = sum over the left taps j < min(n + 1, (interpLength - offL) / step) of w x[n - j], then the right taps
 * j < min(sourceLength - n - 1, (interpLength - offR) / step) of w x[n + 1 + j], with
 * w = table[o] + delta (table[o + 1] - table[o]), o = off + j step, summed in float32 in that order.  Samples at
 * n - j >= sourceLength count as 0 (the reference reads past its input there).  Persistent workgroups keep the table in
 * LDS when it fits, else read it from global memory; the input span under a tile of outputs is staged in LDS when it fits.
 * AFX_ERR_ARG for a NULL pointer, non-positive sizes, a stride below its row or a ratio with step < 1. */
int afxk_resample(const AfxResampleArgs *a, void *stream);

/* ---- phase vocoder (afx_phasevocoder.hip) ------------------------------------- */
/* Where output frame i sits between the input frames (phase_vocoder.c:36, :58-59): t = 0 + i * rate in float32 as
 * __varange states it (flux_vector.c:2186), k = floorf(t), alpha = t - floorf(t).  Stated once for the kernels, the host
 * plan and the tests. */
AFX_HD static inline int afx_pv_time(int i, float rate, float *alpha) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = 0.f + (float)i * rate;
    const float f = floorf(t);
    *alpha = t - f;
    return f < 2147483520.f ? (int)f : 2147483520; /* (beyond every frame count: a zero frame) */
}
/* output frames of T1 input frames: ceilf(T1 / rate) in float32 (phase_vocoder.c:35); 0: rate is not a positive finite
 * number, or the count is beyond AFX_PV_MAX_FRAMES */
#define AFX_PV_MAX_FRAMES (1 << 24)
static inline int afx_pv_frames(int T1, float rate) {
    if (T1 <= 0 || !(rate > 0.f) || !(rate <= 3.0e38f)) return 0;
    const float f = ceilf((float)T1 / rate);
    return f >= 1.f && f <= (float)AFX_PV_MAX_FRAMES ? (int)f : 0;
}
/* the expected phase advance of bin j per hop (phase_vocoder.c:38, __vlinspace flux_vector.c:2151-2158) */
AFX_HD static inline float afx_pv_phi_step(int hop, int F) {
    return ((float)(3.14159265358979323846 * hop) - 0.f) / (float)(F - 1 > 0 ? F - 1 : 1);
}
typedef struct {
    const float *re, *im;  /* device [batch * T1, inPitch]: bins 0 ... N / 2 of every input frame are read                */
    long long inPitch;     /* floats between input rows, >= N / 2 + 1                                                      */
    int batch, T1, T2;     /* clips, input frames and output frames (afx_pv_frames) per clip                                */
    int radix2Exp, hop;    /* N = 2^radix2Exp, 1 ... 14                                                                     */
    float rate;
    float *mag, *ang;      /* device scratch [batch * T1, N / 2 + 1] each; mag == re and ang == im (inPitch N / 2 + 1): in place */
    float *outRe, *outIm;  /* device [batch * T2, N]: every word is written (outRe holds the phases between two launches)   */
} AfxPhaseVocoderArgs;
/* phase_vocoder.c:19-120 in three launches.  polar: mag = sqrtf(re re + im im) (unfused), ang = atan2f(im, re) of every input
 * frame, once.  phase: one lane per (clip, bin j), serial over i < T2: phase[i][j] is stored to outRe[i][j], then advances by
 * phi_j + wrap((ang[k + 1] - ang[k]) - phi_j) in float32, the wrap through float64 as the reference writes it; frames at or
 * beyond T1 are zero frames (angle 0).  synthesis: (mag[k] (1 - alpha) + mag[k + 1] alpha) (cosf, sinf)(phase) over
 * (clip, i, j), bin j and its conjugate mirror N - j.  AFX_ERR_ARG for a NULL pointer or sizes outside the limits above. */
int afxk_phase_vocoder(const AfxPhaseVocoderArgs *a, void *stream);
/* dst[b * dstStride + i] = i < srcLength ? src[b * srcStride + i] : 0 for i < length, b < batch: rows cut or zero-tailed */
int afxk_rows_fit(const float *src, long long srcStride, int srcLength, float *dst, long long dstStride, int length, int batch,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AFX_DEVICE_H */
