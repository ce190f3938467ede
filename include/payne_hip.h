/* payne_hip.h -- C ABI of libpayne_hip.so: the MI355X (gfx950) implementation of
 * ThePayne's nested-sampling likelihood hot path, evaluated in batch.
 *
 * Each entry point names the reference interface (pacargile/ThePayne, paths relative
 * to the reference root) it stands in for.  The reference is pure Python with no FFI
 * of its own; this is the boundary a maintainer binds with ctypes.
 *
 * Conventions
 *  - plain C, no torch/HIP types in signatures (`stream` is a hipStream_t passed as
 *    void*; NULL = the default stream);
 *  - return 0 on success, a negative PAYNE_E_* code on failure; never throws;
 *    payne_last_error() gives the message;
 *  - pointers documented "device" are fp32/fp64 arrays in the memory of the context's
 *    GPU, owned by the caller and alive for as long as the context uses them (weights,
 *    theta, outputs); pointers documented "host" are read during the call only;
 *  - batch calls enqueue work on `stream` and do not synchronise; the caller
 *    synchronises the stream before reading an output buffer;
 *  - a context is bound to one device and is not thread-safe (the reference's callers,
 *    dynesty's sampling loop, are single-threaded: Payne/fitting/fitstar.py:309-338);
 *  - NaN in -> NaN out at the same places as the reference.
 */
#ifndef PAYNE_HIP_H
#define PAYNE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PAYNE_ABI_VERSION 2

#define PAYNE_OK 0
#define PAYNE_E_INVALID (-1)     /* bad argument / descriptor */
#define PAYNE_E_UNSUPPORTED (-2) /* valid in the reference, not (yet) by this library */
#define PAYNE_E_HIP (-3)         /* HIP runtime error */
#define PAYNE_E_BATCH (-4)       /* B exceeds opts.b_max */
#define PAYNE_E_SIGMA (-5)       /* payne_smooth_direct: target sigma below the input's (the reference raises ValueError) */

/* activation codes */
#define PAYNE_ACT_NONE 0
#define PAYNE_ACT_LRELU 1   /* z*(z>0) + 0.01*z*(z<0)  Payne/predict/ystpred.py:41-45 */
#define PAYNE_ACT_SIGMOID 2 /* torch.sigmoid            Payne/train/NNmodels.py:155-160 */

#define PAYNE_MAX_LAYERS 8
#define PAYNE_MAX_LABELS 5
#define PAYNE_MAX_POLY 12

/* One dense layer y = act(W x + b); W is [n_out][n_in] row-major fp32 exactly as the
 * reference stores it (w_array_k / model/linK.weight / model/features.K.weight). */
typedef struct payne_layer {
  const float* w; /* device [n_out*n_in] */
  const float* b; /* device [n_out] */
  int n_in, n_out;
  int act; /* activation applied to this layer's OUTPUT */
} payne_layer;

/* The spectral emulator: replaces ystpred.Net (Payne/predict/ystpred.py:18-58) and
 * predictspec.ANN + NNmodels.{LinNet,SMLP} (Payne/predict/predictspec.py:29-74,
 * Payne/train/NNmodels.py:92-168).  YST1: 3 layers lrelu,lrelu,none; SMLP: 4 layers
 * lrelu x3,none; LinNet: 6 layers sigmoid x5,none.  Input encoding for all of them:
 * (x - xmin)/(xmax - xmin) - 0.5. */
typedef struct payne_model_desc {
  int n_layers; /* >= 2 */
  payne_layer layers[PAYNE_MAX_LAYERS];
  int n_labels;             /* 4: Teff,logg,[Fe/H],[a/Fe]; 5: + vmic */
  const double* xmin;       /* host [n_labels] (Teff in K: apply ystpred.py:76-79 first) */
  const double* xmax;       /* host [n_labels] */
  int npix;                 /* == layers[n_layers-1].n_out */
  const double* wavelength; /* host [npix], strictly increasing, Angstrom */
  double resolution;        /* sigma-based R of the ANN (file key 'resolution') */
} payne_model_desc;

/* The observed spectrum: fitargs['obs_wave_fit','obs_flux_fit','obs_eflux_fit']
 * (Payne/fitting/fitstar.py:71-98).  flux/eflux may be NULL (predict-only context). */
typedef struct payne_obs_desc {
  int nobs;
  const double* wave;  /* host [nobs] */
  const double* flux;  /* host [nobs] or NULL */
  const double* eflux; /* host [nobs] or NULL */
} payne_obs_desc;

/* Photometric emulator: the stacked per-filter nets of photANN.fastANN
 * (Payne/predict/photANN.py:95-131) + highAv table (Payne/predict/highred.py:4-25)
 * + observed magnitudes fitargs['obs_phot'] (Payne/fitting/likelihood.py:109-112). */
typedef struct payne_phot_desc {
  int n_filters, hidden;
  const float* w1; /* device [F][H][6] */
  const float* b1; /* device [F][H]    */
  const float* w2; /* device [F][H][H] */
  const float* b2; /* device [F][H]    */
  const float* w3; /* device [F][H]    */
  const float* b3; /* device [F]       */
  const double* xmin;    /* host [6] */
  const double* xmax;    /* host [6] */
  const double* hiav;    /* host [F][5] = a1,b1,a2,b2,c2 (NaN rows allowed) or NULL */
  const double* obs_mag; /* host [F] or NULL */
  const double* obs_err; /* host [F] or NULL */
} payne_phot_desc;

typedef struct payne_opts {
  int b_max;     /* largest batch any call will pass (workspaces are sized for it) */
  int npoly;     /* Chebyshev blaze coefficients pc_0.. in theta (0 = modpoly off) */
  int photscale; /* 1: phot block carries log(A) (genphot_scaled); 0: log(R), Dist (genphot) */
  unsigned variant; /* 0 = the default kernels; PAYNE_V_* bits select the other code paths that ship */
} payne_opts;

/* Kernel variants (payne_opts.variant).  Every one computes the same results; they exist because the default of
 * each pair only covers some shapes (the other is what differently shaped nets / spectra run), and the parity
 * tests run the reference vectors through each of them. */
#define PAYNE_V_OUT_GENERIC 1u   /* output layer: register-staged GEMM (what nets with unequal hidden widths use) */
#define PAYNE_V_POST_GENERIC 2u  /* post kernel: runtime FFT geometry (what spectra other than 1k/2k/4k/8k use) */
#define PAYNE_V_TW_GLOBAL 4u     /* post kernel: twiddles read from L2 instead of LDS (what 8k spectra use) */
#define PAYNE_V_POST_FULL 8u     /* likelihood through the full post kernel instead of its likelihood-only build */
#define PAYNE_V_NO_PREP 16u      /* per-candidate records computed inside the post kernel (what 2-layer nets use) */
#define PAYNE_V_SELECT_MEDIAN 64u /* continuum / LSF medians by radix selection (what rows too long for an LDS sort use) */
#define PAYNE_V_NO_WALK_TAIL 512u /* the sampler's chain step as a launch of its own between two likelihood batches (what
                                  * contexts without a likelihood-only post kernel use) instead of at the post kernel's tail */
#define PAYNE_V_OUT_BK64 1024u   /* output layer: 64-deep stages (half as many barrier steps) when the padded width allows */
#define PAYNE_V_OUT_ROLLED 2048u /* output layer: the loop over k-steps as other hidden widths than 300 run it (not unrolled) */
#define PAYNE_V_OUT_F32 4096u    /* output layer: the fp32 matrix instruction (v_mfma_f32_32x32x2_f32) instead of six bf16 products of
                                  * operands split in three (fp32-accurate either way; what launches with several tiles per CU use) */
#define PAYNE_V_SED_OWN_LAUNCH 8192u /* joint likelihoods: the photometric nets as a launch of their own (one wave per candidate and
                                    * filter: what payne_sed_batch and nets wider than 64 use) instead of extra workgroups of the
                                    * hidden-layer launch */
#define PAYNE_V_OUT_SMALL_TILES 16384u /* output layer with many tiles per CU (C5): 64 x 128 tiles, two workgroups per CU (what batches that
                                       * are not whole 128 x 256 tiles use) instead of persistent workgroups on 128 x 256 tiles */
#define PAYNE_V_BIG_WORKSPACE 65536u /* 65 536-point spectra: both convolution stages through the global workspace (the four-step transform: what
                                      * other lengths above 16 384 use) instead of on the compute unit */
#define PAYNE_V_NO_WALK_SPEC 131072u /* the sampler's next proposal drawn at the post kernel's tail, after the likelihood it waits for (what fits
                                     * with more than 16 sampled dimensions or 32 theta columns use), instead of made ahead for both outcomes by
                                     * idle workgroups of the hidden-layer launch */
#define PAYNE_V_ROWS_PIXEL 262144u /* the output layer writes pixels and the post kernel transforms them itself (what runs with a continuum
                                    * network, with vsini maps that are not the identity, and for spectra other than 1k/2k/4k/8k);
                                    * default where it applies: the output layer's weights carry the first stage's forward transform */
#define PAYNE_V_OUT_PLANES 524288u /* output layer: the weights read as three bf16 planes split at payne_ctx_create (what nets of other widths than
                                    300 and batches with more tiles than compute units use) instead of fp32 weights split on their way into LDS */
#define PAYNE_V_OUT_BF16X3 1048576u /* output layer: operands split in three bf16 parts, six products (what batches with more tiles than
                                     compute units and nets whose last hidden layer could not be calibrated use) instead of two fp16 parts, three products */
#define PAYNE_V_HID_F32 2097152u  /* hidden layers: the fp32 matrix instruction for the second layer too (what later layers of deeper nets and
                                     widths other than 289..304 use) instead of products of fp16 pairs */
#define PAYNE_V_HID_CHAIN 4194304u /* deeper nets: the hidden layers past the second in ONE launch with hand-offs inside a 32-candidate row
                                      block (agent-scope release / acquire: measured 8 us a hop against 5.7 us a launch -- kept as a tested
                                      variant, not a default) */
#define PAYNE_V_HID_WAVES4 8388608u /* sigmoid nets: the first launch's tiles by four waves (what leaky-ReLU nets and launches that carry
                                      photometric tiles use) instead of eight */
#define PAYNE_V_OUT_WHOLE_TILE 16777216u /* output layer, one tile a compute unit: the tile's k-loop in one pass, all its rows stored at the end
                                           (what batches with more tiles than compute units use) instead of two halves, the first one's rows
                                           leaving under the second one's products */
#define PAYNE_V_LSF_GLOBAL 128u  /* LSF broadening with its buffers in global memory (what spectra > 8192 px use) */

typedef struct payne_ctx payne_ctx;

int payne_version(void);

/* Build a context on `device` (HIP ordinal).  model may be NULL for a photometry-only
 * fit, obs NULL if no observed grid is bound yet, phot NULL without photometry.
 * Replaces likelihood.__init__ -> GenMod._initspecnn/_initphotnn
 * (Payne/fitting/likelihood.py:7-40, Payne/fitting/genmod.py:15-43). */
int payne_ctx_create(const payne_model_desc* model, const payne_obs_desc* obs,
                     const payne_phot_desc* phot, const payne_opts* opts, int device,
                     payne_ctx** out);

/* Re-bind the observed grid (the `outwave` of getspec / a new spectrum). */
int payne_ctx_set_obs(payne_ctx* ctx, const payne_obs_desc* obs);

/* Bind (or, with NULL, remove) the continuum network of ystpred.PayneSpecPredict(Cnnpath=...)
 * (Payne/predict/ystpred.py:81-85): every spectrum the context produces from then on is the spectral
 * ANN's output times the continuum network's, converted F_nu -> F_lambda, normalised by its
 * NaN-ignoring median and interpolated onto the spectral ANN grid (NaN outside; ystpred.py:191-209).
 * Same descriptor as the spectral model (`resolution` unused); n_labels must match; any npix. */
int payne_ctx_set_continuum(payne_ctx* ctx, const payne_model_desc* cont);

/* LSF-vector instrumental broadening: getspec(inst_R=<array>, outwave=...) (Payne/predict/ystpred.py:248-269
 * -> smoothspec(smoothtype='lsf') -> smooth_lsf_fft, Payne/utils/smoothing.py:125-151, 482-586).
 * lsf: HOST fp64 [n], the Gaussian dispersion (same units as the wavelengths) at every pixel of the bound
 * observed grid (n must equal its length).  While a vector is set, theta's Inst_R column is ignored by
 * payne_lnlike_batch and stages 2/3 of payne_predict_batch; results are never NaN inside the model's range
 * (np.interp clamps).  NULL removes it; payne_ctx_set_obs removes it too.  Any spectrum length; the FFT length the
 * reference derives from the vector (smoothing.py:533-538) must not exceed the model's own (pow2ceil(npix)): NaN then. */
int payne_ctx_set_lsf(payne_ctx* ctx, const double* lsf, int n);
/* The same with the dispersion vector given on wavelengths of its own (HOST fp64 [n], strictly increasing) instead of on the
 * bound observed grid: smoothspec(wave, spec, resolution=<vector on wave>, outwave=<another grid>, smoothtype='lsf')
 * (Payne/utils/smoothing.py:125-151: the vector is a function of the INPUT wavelengths there; getspec interpolates it from the
 * output grid, ystpred.py:255-259).  The dispersion at a model pixel is np.interp of the vector (clamped outside). */
int payne_ctx_set_lsf_on(payne_ctx* ctx, const double* lsf_wave, const double* lsf, int n);

void payne_ctx_destroy(payne_ctx* ctx);

/* Message for the last failure on ctx (ctx == NULL: last create failure). */
const char* payne_last_error(const payne_ctx* ctx);

/* Number of fp64 columns of one theta row: 8 + npoly + 4.
 *   0 Teff  1 log(g)  2 [Fe/H]  3 [a/Fe]  4 Vrad  5 Vrot  6 Vmic  7 Inst_R
 *   8.. pc_0..pc_{npoly-1}
 *   then  log(A) | log(R),  Dist,  Av,  Rv
 * i.e. `specpars` followed by `photpars` of likelihood.lnlikefn
 * (Payne/fitting/likelihood.py:50-72); NaN = "absent" exactly as there. */
int payne_theta_cols(const payne_ctx* ctx);

/* lnL for B parameter vectors: likelihood.lnlike over a batch
 * (Payne/fitting/likelihood.py:84-117 -> genmod.py:58-108 -> ystpred.py:119-277).
 * Inst_R is the sampled FWHM-based value; the 2.355 factor of genmod.py:82-85 is
 * applied inside.  theta: device fp64 [B][payne_theta_cols]; lnl: device fp64 [B]. */
int payne_lnlike_batch(payne_ctx* ctx, const double* theta, int B, double* lnl, void* stream);

/* Model spectra for B parameter vectors.
 *   stage 0: raw ANN output on the ANN grid          (predictspec, ystpred.py:84-99)
 *   stage 1: after rotational broadening, ANN grid   (ystpred.py:211-224)
 *   stage 2: getspec on the bound observed grid      (ystpred.py:226-277)
 *   stage 3: genspec = stage 2 x Chebyshev blaze     (genmod.py:103-106)
 *   stage 4: the continuum network's own output      (predictcont, ystpred.py:101-117); ld_out >= its npix
 * With a continuum network bound (payne_ctx_set_continuum) stages 1-3 and the likelihood include the
 * normalised continuum (ystpred.py:191-209); stage 0 stays the spectral network's own output.
 * flags bit 0 (PAYNE_F_FWHM_R): theta[7] is FWHM-based (genspec semantics, x2.355);
 * otherwise it is the sigma-based R handed to getspec.
 * out: device fp32 [B][ld_out]; ld_out >= npix (stages 0,1) or nobs (stages 2,3). */
#define PAYNE_F_FWHM_R 1u
#define PAYNE_STAGE_CONT 4
int payne_predict_batch(payne_ctx* ctx, const double* theta, int B, int stage, unsigned flags,
                        float* out, int ld_out, void* stream);

/* The broadening stages on caller-supplied spectra: PayneSpecPredict.smoothspec (Payne/predict/ystpred.py:279-281 ->
 * Payne/utils/smoothing.py:19-169, the 'vsini' / 'vel' / 'R' / 'lsf' FFT branches).  spectra: device fp32
 * [B][ld_spec], full flux on the context's model wavelength grid; theta, stage (1..3), flags and out as for
 * payne_predict_batch -- the ANN forward pass is simply replaced by `spectra`.  Stage 4 (PAYNE_SMOOTH_VSINI_TO_OBS):
 * rotational broadening only, interpolated from the stage's own resampled grid onto the bound observed grid with NaN outside
 * (smoothspec(smoothtype='vsini', outwave=...), smoothing.py:293-312); out is [B][nobs]. */
#define PAYNE_SMOOTH_VSINI_TO_OBS 4
int payne_smooth_batch(payne_ctx* ctx, const float* spectra, int ld_spec, const double* theta, int B, int stage,
                       unsigned flags, float* out, int ld_out, void* stream);

/* smoothspec's branches that are not on the sampler's path, on caller-supplied HOST arrays, synchronous (no context: an
 * analysis helper of PayneSpecPredict.smoothspec, Payne/predict/ystpred.py:279-281 -> Payne/utils/smoothing.py):
 *   PAYNE_SMOOTH_VEL_DIRECT   smooth_vel       (smoothing.py:171-210)  fftsmooth=False, smoothtype 'vel' / 'R'
 *   PAYNE_SMOOTH_WAVE_DIRECT  smooth_wave      (:339-393)              fftsmooth=False, smoothtype 'lambda'; sigma scalar or [n]
 *   PAYNE_SMOOTH_LSF_DIRECT   smooth_lsf       (:435-480)              fftsmooth=False, smoothtype 'lsf'; sigma [nout] (or scalar)
 *   PAYNE_SMOOTH_WAVE_FFT     smooth_wave_fft  (:395-433)              fftsmooth=True,  smoothtype 'lambda'
 *   PAYNE_SMOOTH_INTERP       np.interp(outwave, wave, spec)           smooth_lsf with neither sigma nor lsf (:464-465)
 * wave, spec [n]: the input AFTER smoothspec's mask and nan_to_num (:131-138); sigma in the units the reference's function
 * takes (km/s for VEL_DIRECT, Angstrom otherwise); inres / in_vel / nsigma: its keywords (defaults 0 / 0 / 10).
 * Returns PAYNE_E_SIGMA where the reference raises ValueError (smooth_wave: target sigma below the input's, :381-383);
 * PAYNE_E_INVALID is a malformed call (null pointers, n < 2, a sigma vector of the wrong length). */
#define PAYNE_SMOOTH_VEL_DIRECT 0
#define PAYNE_SMOOTH_WAVE_DIRECT 1
#define PAYNE_SMOOTH_LSF_DIRECT 2
#define PAYNE_SMOOTH_WAVE_FFT 3
#define PAYNE_SMOOTH_INTERP 4
int payne_smooth_direct(int device, int kind, const double* wave, const double* spec, int n, const double* outwave, int nout,
                        const double* sigma, int nsig, double inres, int in_vel, double nsigma, double* out);

/* The velocity scan of RVcalc (Payne/fitting/fitutils.py:79-94, scanned by scipy.optimize.brute at :64-69) for G velocities
 * at once, on caller-supplied HOST arrays, synchronous, no context (like payne_smooth_direct):
 *   chisq[g] = sum_i (m_gi - flux_i)^2 / eflux_i^2,
 * m_gi = interp1d(modwave * (1 + rv_g / 299792.458), modflux, kind='linear', bounds_error=False, fill_value=1.0)(wave_i):
 * bracket by searchsorted (side left, clipped to [1, nm - 1]), both end points inside, 1.0 outside.  NaN in modflux or flux
 * makes chisq[g] NaN wherever it is reached (no pixel is skipped, as in the reference).  fp64 throughout; the sum is formed in
 * a fixed order, so the same call returns the same bits.
 * PAYNE_E_INVALID: null pointers, nm < 2, nobs < 1, G < 1, modwave not strictly increasing. */
int payne_rv_scan(int device, const double* modwave, const double* modflux, int nm, const double* wave, const double* flux,
                  const double* eflux, int nobs, const double* rv, int G, double* chisq);

/* The masked chi^2 that ends BROADcalc.chisq_broad (Payne/fitting/fitutils.py:148-154) for G rows: rows is device fp32
 * [G][ld] as payne_smooth_batch writes them, n valid pixels per row; flux, eflux: HOST fp64 [n]; chisq: HOST fp64 [G];
 * n_kept: HOST int32 [G].  The pixels with rows[g][i] < threshold are kept (NaN compares false), compacted in order; the j-th
 * kept model value is paired with the j-th kept flux and with eflux[j], the first n_kept entries of the UNMASKED error vector
 * -- the reference's line `eflux[cond]` discards its result and zip() truncates: its arithmetic is reproduced, not its intent.
 * The kernel is enqueued on `stream` (behind whatever wrote the rows there) and the call synchronises it before returning.
 * PAYNE_E_INVALID: null pointers, n < 1, n > ld, G < 1. */
int payne_chisq_below(int device, const float* rows, int ld, int n, int G, const double* flux, const double* eflux,
                      double threshold, double* chisq, int* n_kept, void* stream);

/* The medians TestSpec's report takes of its residual matrix (Payne/testing/testspec.py:94-108, :125-208, :227-361).  All
 * pointers are DEVICE pointers: pred fp32 [N][ld_pred], truth fp32 [N][ld_truth] (P valid pixels per row, the padding is never
 * read), groups uint8 [G][N] (non-zero = the row belongs to the set).  With r[i][j] = fabs((double)truth[i][j] -
 * (double)pred[i][j]), never stored:
 *   pix_med[g][j] = np.median of { r[i][j] : groups[g][i] != 0 }     fp64 [G][P]
 *   row_med[i]    = np.median of r[i][0..P-1]                        fp64 [N]; NULL: not computed
 * np.median: the elements of rank (m-1)>>1 and m>>1 averaged as 0.5 * (lo + hi); NaN if any member is NaN; NaN for an empty
 * set.  Found by radix selection on the integer image of r (csrc/mad_core.hpp): exact, and the same bits on every call.
 * G == 0 with row_med != NULL is valid (row medians only).  The kernels are enqueued on `stream` (behind whatever wrote the two
 * matrices there) and the call synchronises it before returning.
 * PAYNE_E_INVALID (nothing is written): null pred / truth / pix_med, N < 1, P < 1, ld_pred < P, ld_truth < P, G < 0,
 * groups == NULL with G > 0.  PAYNE_E_UNSUPPORTED: G > 65535. */
int payne_mad_stats(int device, const float* pred, int ld_pred, const float* truth, int ld_truth, int N, int P,
                    const unsigned char* groups, int G, double* pix_med, double* row_med, void* stream);

/* ---- photometric LayerNorm + SiLU networks: Payne/predict/photANN_new.py (MLP_v0 / MLP_v1 of Payne/train/NNmodels_new.py) ----
 * One network maps D_in labels to D_out bands through n_layers Linear layers; every layer but the last is followed by
 * nn.LayerNorm over its true width (mean, biased variance about that mean, eps = 1e-5, gain and bias per column) and SiLU,
 * z / (1 + exp(-z)).  All arithmetic of the network is fp32 (products on the fp32 matrix instruction, an fp32 fmaf chain per
 * output); one launch evaluates every layer for a tile of 64 rows (csrc/k_lnmlp.hip, csrc/lnmlp_core.hpp).
 * payne_lnmlp_create: every pointer of the descriptor is a HOST pointer; the arrays are copied (the weights re-ordered and
 * padded) to `device`.  layers[i].w is row-major fp32 [n_out][n_in] (torch's Linear.weight), b fp32 [n_out], ln_gain / ln_bias
 * fp32 [n_out] on every layer but the last, where both are NULL.  in_mid / in_std fp64 [D_in] (both or neither): the input is
 * (x - mid) / std in fp64, rounded once to fp32; without them x itself rounded to fp32.  out_mid / out_std fp64 [D_out] (both
 * or neither): the output is y * std + mid in fp64, rounded once to fp32.
 *   PAYNE_E_INVALID      null desc / out, a width < 1, n_in of a layer != n_out of the one before, null w / b, a hidden layer
 *                        without ln_gain / ln_bias, an output layer with them, one of a mid / std pair without the other
 *   PAYNE_E_UNSUPPORTED  n_layers outside 2..8, D_in > 32, a hidden width or D_out > 512
 * payne_lnmlp_eval: x_dev DEVICE fp64 [N][ld_x] (D_in columns read), y_dev DEVICE fp32 [N][ld_y] (D_out columns written;
 * nothing beyond them, nothing beyond N rows).  The launch is enqueued on `stream`; the call does not wait for it.  No
 * atomics, no order that depends on timing: the same input gives the same bits.  N == 0 succeeds and launches nothing.
 *   PAYNE_E_INVALID      null handle, N < 0, null x_dev / y_dev with N > 0, ld_x < D_in, ld_y < D_out */
#define PAYNE_LNMLP_MAX_LAYERS 8
#define PAYNE_LNMLP_MAX_IN 32
#define PAYNE_LNMLP_MAX_WIDTH 512

typedef struct payne_lnmlp_layer {
  int n_in, n_out;
  const float* w;
  const float* b;
  const float* ln_gain; /* NULL on the output layer */
  const float* ln_bias; /* NULL on the output layer */
} payne_lnmlp_layer;

typedef struct payne_lnmlp_desc {
  int n_layers;
  payne_lnmlp_layer layers[PAYNE_LNMLP_MAX_LAYERS];
  const double* in_mid;
  const double* in_std;
  const double* out_mid;
  const double* out_std;
} payne_lnmlp_desc;

typedef struct payne_lnmlp payne_lnmlp;

int payne_lnmlp_create(int device, const payne_lnmlp_desc* desc, payne_lnmlp** out);
int payne_lnmlp_eval(payne_lnmlp* h, const double* x_dev, int ld_x, int N, float* y_dev, int ld_y, void* stream);
void payne_lnmlp_destroy(payne_lnmlp* h);

/* ---- training those networks: Payne/train/trainphot.py (TrainMod.train_mod) on MLP_v0 / MLP_v1 of Payne/train/NNmodels_new.py ----
 * One step is trainphot.py:411-447: the forward in training mode (the dropout of NNmodels_new.py:21 / :48 from a counter-based
 * mask), MSELoss(reduction='mean') (:343), backward, torch.optim.RAdam(lr) with its defaults (:353).  All arithmetic of the
 * network, the backward and the update is fp32 (products on the fp32 matrix instruction); the loss is the fp32 residuals
 * squared and summed in fp64.  Three launches a step (csrc/k_lnmlp_train.hip, csrc/lnmlp_train_core.hpp), no atomics: the same
 * parameters, batch, seed and step counter give the same bits for loss, gradients and updated parameters.  With every
 * dropout_p = 0 the handle's forward returns payne_lnmlp_eval's bits on the same parameters.  A handle is used from one stream
 * at a time.
 * payne_lnmlp_train_create: `init` as for payne_lnmlp_create (HOST pointers, row-major weights) = the initial parameters, or a
 * restart file's (trainphot.py:278-292); opts: RAdam's lr, beta1, beta2, eps (torch's defaults: 1e-3, 0.9, 0.999, 1e-8),
 * dropout_p[i] the probability behind hidden block i (0 = none; MLP_v0: p[2] = 0.3, MLP_v1: p[1] = 0.01), the mask's seed, and
 * max_rows, the largest batch of a step; the workspace (activations and gradients of max_rows rows) is allocated here.
 *   PAYNE_E_INVALID      what payne_lnmlp_create rejects; in_mid / in_std / out_mid / out_std not NULL (training data arrive
 *                        normalised, as ReadPhot(norm=True) hands them over); null opts; a dropout_p outside [0, 1); max_rows < 1;
 *                        lr <= 0, a beta outside [0, 1), eps < 0
 *   PAYNE_E_UNSUPPORTED  n_layers outside 2..8, D_in > 32, a hidden width or D_out > 512
 * payne_lnmlp_train_step: one forward / backward / update on x_dev DEVICE fp32 [N][ld_x] (D_in columns read) and t_dev DEVICE
 * fp32 [N][ld_t] (D_out columns read), 1 <= N <= max_rows (trainphot.py:428-443).  loss_dev: DEVICE double, the loss before the
 * update (:431), or NULL.  Enqueued on `stream`; the call does not wait.  N == 0 succeeds and does nothing.
 *   PAYNE_E_INVALID      null handle, N < 0, N > max_rows, null x_dev / t_dev with N > 0, ld_x < D_in, ld_t < D_out
 * payne_lnmlp_train_loss: the loss in evaluation mode (trainphot.py:456-476): no dropout, no parameter, optimiser state or step
 * counter changes.  N may exceed max_rows (evaluated in chunks).  Enqueued; does not wait.  N == 0 succeeds, writes nothing.
 *   PAYNE_E_INVALID      as payne_lnmlp_train_step without the limit on N; null loss_dev with N > 0
 * payne_lnmlp_train_get: what = PAYNE_LNMLP_PARAMS (the current parameters, model.state_dict() of trainphot.py:511-519) or
 * PAYNE_LNMLP_GRADS (the gradients of the last step), copied row-major into the HOST arrays host_out's pointers name (same
 * widths as `init`; the norm pointers are ignored).  Waits for the work enqueued through the handle.
 *   PAYNE_E_INVALID      null handle / host_out, another `what`, n_layers or a width differing from the handle's, a null array
 * payne_lnmlp_train_steps: the number of steps taken (RAdam's t; the mask of the next step uses this value); -1 for NULL.
 * payne_lnmlp_train_destroy: NULL is allowed.
 * payne_lnmlp_dropout_mask: HOST only, no GPU work: out_host[r * n_cols + c] = 1 where column c of hidden block `layer` is kept
 * in row r of the batch of step `step` (0 = a handle's first), from the function the kernels use.  p == 0 keeps everything.
 *   PAYNE_E_INVALID      null out_host, negative n_rows / n_cols / layer, p outside [0, 1) */
#define PAYNE_LNMLP_PARAMS 0
#define PAYNE_LNMLP_GRADS 1

typedef struct payne_lnmlp_train_opts {
  double lr, beta1, beta2, eps;
  double dropout_p[PAYNE_LNMLP_MAX_LAYERS];
  unsigned long long seed;
  int max_rows;
} payne_lnmlp_train_opts;

typedef struct payne_lnmlp_train payne_lnmlp_train;

int payne_lnmlp_train_create(int device, const payne_lnmlp_desc* init, const payne_lnmlp_train_opts* opts, payne_lnmlp_train** out);
int payne_lnmlp_train_step(payne_lnmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N, double* loss_dev,
                           void* stream);
int payne_lnmlp_train_loss(payne_lnmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N, double* loss_dev,
                           void* stream);
int payne_lnmlp_train_get(payne_lnmlp_train* h, int what, payne_lnmlp_desc* host_out);
long long payne_lnmlp_train_steps(payne_lnmlp_train* h);
void payne_lnmlp_train_destroy(payne_lnmlp_train* h);
int payne_lnmlp_dropout_mask(unsigned long long seed, unsigned long long step, int layer, int n_rows, int n_cols, double p,
                             unsigned char* out_host);

/* ---- training the spectral networks: Payne/train/trainspec.py (TrainMod.train_mod) on SMLP / LinNet of Payne/train/NNmodels.py ----
 * The network maps D_in encoded labels to D_out pixels through n_layers Linear layers; every layer but the last is followed by
 * LeakyReLU(0.01) (PAYNE_SPECMLP_LEAKY: SMLP, three hidden layers) or a sigmoid (PAYNE_SPECMLP_SIGMOID: LinNet, five).  One step
 * is trainspec.py:422-444: forward, MSELoss(reduction='sum') (:319), backward, torch.optim.RAdam(lr) with its defaults (:328).
 * All arithmetic of the network, the backward and the update is fp32 (products on the fp32 matrix instruction); the loss is the
 * fp32 residuals squared and summed in fp64.  Five launches a step (csrc/k_specmlp_train.hip, csrc/specmlp_train_core.hpp), no
 * atomics: the same parameters, batch and step counter give the same bits for loss, gradients and updated parameters.  The rows
 * arrive encoded, (x - xmin) / (xmax - xmin) - 0.5 rounded to fp32 (NNmodels.py:109-113).  A handle is used from one stream at a
 * time.
 * payne_specmlp_train_create: every pointer of the descriptor is a HOST pointer: layers[i].w row-major fp32 [n_out][n_in]
 * (torch's Linear.weight), b fp32 [n_out]: the initial parameters, or a restart file's.  opts: RAdam's lr, beta1, beta2, eps
 * (the reference: 1e-4, 0.9, 0.999, 1e-8) and max_rows, the largest batch of a step; the workspace is allocated here.
 *   PAYNE_E_INVALID      null desc / opts / out, a width < 1, n_in of a layer != n_out of the one before, null w / b, an
 *                        activation kind other than the two, max_rows < 1, lr <= 0, a beta outside [0, 1), eps < 0
 *   PAYNE_E_UNSUPPORTED  n_layers outside 2..8, D_in > 32, a hidden width > 512, D_out > 65536
 * payne_specmlp_train_step: one forward / backward / update on x_dev DEVICE fp32 [N][ld_x] (D_in columns read) and t_dev DEVICE
 * fp32 [N][ld_t] (D_out columns read), 1 <= N <= max_rows.  loss_dev: DEVICE double, the batch's sum of squares before the
 * update, or NULL.  Enqueued on `stream`; the call does not wait.  N == 0 succeeds and does nothing.
 *   PAYNE_E_INVALID      null handle, N < 0, N > max_rows, null x_dev / t_dev with N > 0, ld_x < D_in, ld_t < D_out
 * payne_specmlp_train_loss: the forward and the sum of squares alone; no parameter, optimiser state or step counter changes.
 * N may exceed max_rows (evaluated in chunks).  N == 0 succeeds, writes nothing.
 *   PAYNE_E_INVALID      as payne_specmlp_train_step without the limit on N; null loss_dev with N > 0
 * payne_specmlp_train_predict: the forward alone, y_dev DEVICE fp32 [N][ld_y] (D_out columns written; nothing beyond them,
 * nothing beyond N rows).  N may exceed max_rows.
 *   PAYNE_E_INVALID      null handle, N < 0, null x_dev / y_dev with N > 0, ld_x < D_in, ld_y < D_out
 * payne_specmlp_train_set_lr: the learning rate of the steps that follow (trainspec.py:334,531 StepLR once an epoch).
 *   PAYNE_E_INVALID      null handle, lr <= 0 or not finite
 * payne_specmlp_train_get: what = PAYNE_SPECMLP_PARAMS or PAYNE_SPECMLP_GRADS (the gradients of the last step), copied row-major
 * into the HOST arrays host_out's pointers name (same widths as `init`).  Waits for the work enqueued through the handle.
 *   PAYNE_E_INVALID      null handle / host_out, another `what`, n_layers or a width differing from the handle's, a null array
 * payne_specmlp_train_steps: the number of steps taken (RAdam's t); -1 for NULL.
 * payne_specmlp_train_destroy: NULL is allowed. */
#define PAYNE_SPECMLP_LEAKY 0
#define PAYNE_SPECMLP_SIGMOID 1
#define PAYNE_SPECMLP_PARAMS 0
#define PAYNE_SPECMLP_GRADS 1
#define PAYNE_SPECMLP_MAX_OUT 65536

typedef struct payne_specmlp_layer {
  int n_in, n_out;
  const float* w;
  const float* b;
} payne_specmlp_layer;

typedef struct payne_specmlp_desc {
  int n_layers;
  int act;
  payne_specmlp_layer layers[PAYNE_LNMLP_MAX_LAYERS];
} payne_specmlp_desc;

typedef struct payne_specmlp_train_opts {
  double lr, beta1, beta2, eps;
  int max_rows;
} payne_specmlp_train_opts;

typedef struct payne_specmlp_train payne_specmlp_train;

int payne_specmlp_train_create(int device, const payne_specmlp_desc* init, const payne_specmlp_train_opts* opts, payne_specmlp_train** out);
int payne_specmlp_train_step(payne_specmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N, double* loss_dev,
                             void* stream);
int payne_specmlp_train_loss(payne_specmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N, double* loss_dev,
                             void* stream);
int payne_specmlp_train_predict(payne_specmlp_train* h, const float* x_dev, int ld_x, int N, float* y_dev, int ld_y, void* stream);
int payne_specmlp_train_set_lr(payne_specmlp_train* h, double lr);
int payne_specmlp_train_get(payne_specmlp_train* h, int what, payne_specmlp_desc* host_out);
long long payne_specmlp_train_steps(payne_specmlp_train* h);
void payne_specmlp_train_destroy(payne_specmlp_train* h);

/* ---- label gradients of the emulated spectrum and Fisher matrices ----
 * payne_specjac_*: the spectral networks as payne_specmlp_desc describes them (Net of Payne/predict/ystpred.py:18-58, SMLP / LinNet
 * of Payne/train/NNmodels.py:92-168) evaluated together with their Jacobian with respect to the labels, by a forward-mode pass
 * through the dense layers: for label k the tangent starts as column k of the first weight matrix, is multiplied by act'(z) behind
 * every hidden layer and by the next weight matrix (no bias), and leaves the output layer as dy/de_k, e the encoded labels
 * (x - xmin) / (xmax - xmin) - 0.5 (ystpred.py:47-50, NNmodels.py:109-113; formed in fp64, rounded once to fp32).  dy/dx_k is that
 * times (float)(1 / (xmax_k - xmin_k)).  act' of LeakyReLU(0.01) is 1 for z > 0 and 0.01 otherwise (torch's rule at z == 0; the
 * reference's numpy leaky_relu, ystpred.py:41-45, is 0 there: a set of measure zero); the sigmoid's is s (1 - s) from the primal's
 * fp32 s.  Everything after the network in getspec (ystpred.py:211-277: rotational broadening with its edge rule, the Doppler
 * shift, instrumental broadening, resampling) is linear in the flux, so the Jacobian of the broadened spectrum is
 * payne_smooth_batch applied to these rows.  All arithmetic is fp32 with the products on the fp32 matrix instruction; two launches
 * (csrc/k_specjac.hip, csrc/specjac_core.hpp), no atomics: the same inputs give the same bits.  A handle is used from one stream at
 * a time.
 * payne_specjac_create: every pointer is a HOST pointer: the descriptor's layers[i].w row-major fp32 [n_out][n_in], b fp32 [n_out];
 * xmin, xmax fp64 [D_in].  max_rows: the stars of one pass; the workspace is allocated here.
 *   PAYNE_E_INVALID      null net / xmin / xmax / out, a width < 1, n_in of a layer != n_out of the one before, null w / b, an
 *                        activation kind other than the two, max_rows < 1, an xmin or xmax that is not finite, xmin == xmax
 *   PAYNE_E_UNSUPPORTED  n_layers outside 2..8, D_in > 8, a hidden width > 512, D_out > PAYNE_SPECMLP_MAX_OUT (within these the
 *                        workgroup's image is at most 132 KB of the 160 KB of LDS)
 * payne_specjac_eval: labels_dev DEVICE fp64 [N][ld_x], the raw labels (Teff in K; D_in columns read).  y_dev DEVICE fp32 [N][ld_y],
 * the network's output, or NULL; jac_dev DEVICE fp32 [N][D_in][ld_j], row [i][k] = dy_i / dx_k, or dy_i / de_k with
 * PAYNE_JAC_ENCODED in flags.  D_out columns and N rows are written, nothing beyond them.  N may exceed max_rows (evaluated in
 * chunks, the same bits).  N == 0 succeeds and does nothing.  Enqueued on `stream`; the call does not wait.
 *   PAYNE_E_INVALID      null handle, N < 0, a flag other than PAYNE_JAC_ENCODED, ld_x < D_in, ld_j < D_out, ld_y < D_out with
 *                        y_dev, null labels_dev / jac_dev with N > 0
 * payne_specjac_destroy: NULL is allowed.
 * payne_fisher_batch: F[b][i][j] = sum_p rows[b][i][p] rows[b][j][p] w[p] for B stars and K rows of n pixels each: with rows the
 * derivatives of the model spectrum and w = 1 / sigma^2 the Fisher matrix of the star's parameters.  rows_dev DEVICE fp32
 * [B][K][ld]; w_dev DEVICE fp64 [n], one vector for all stars; F_dev DEVICE fp64 [B][K][K].  Products and sums in fp64, the pixels
 * in index order, no atomics; F[i][j] and F[j][i] are the same bits.  A pixel with w[p] == 0 is skipped whatever the rows hold
 * there (getspec is NaN outside the model's range); any other NaN propagates.  B == 0 succeeds and does nothing.  Enqueued on
 * `stream`; the call does not wait.
 *   PAYNE_E_INVALID      K < 1, n < 1, B < 0, ld < n, null rows_dev / w_dev / F_dev with B > 0
 *   PAYNE_E_UNSUPPORTED  K > 16 */
#define PAYNE_JAC_ENCODED 1u

typedef struct payne_specjac payne_specjac;

int payne_specjac_create(int device, const payne_specmlp_desc* net, const double* xmin, const double* xmax, int max_rows, payne_specjac** out);
int payne_specjac_eval(payne_specjac* h, const double* labels_dev, int ld_x, int N, float* y_dev, int ld_y, float* jac_dev, int ld_j,
                       unsigned flags, void* stream);
void payne_specjac_destroy(payne_specjac* h);
int payne_fisher_batch(int device, const float* rows_dev, int ld, int K, int n, int B, const double* w_dev, double* F_dev, void* stream);

/* ---- batched Levenberg-Marquardt: least-squares fits of K parameters for many stars at once ----
 * payne_lmfit_*: the state of B independent fits and the step that advances all of them, one launch an iteration.  The caller
 * evaluates the model and its derivatives at the handle's trial points (payne_specjac_eval + payne_smooth_batch, say) and hands the
 * rows to payne_lmfit_update; nothing else is needed between two iterations and nothing waits.  Per star, with R the [K+1][n] matrix
 * of the K derivative rows and the residual row flux - model, both in fp64, G = R diag(w) R^T holds the normal matrix A = J^T W J
 * (G[i][j], i, j < K), the gradient g = J^T W r (G[k][K]) and chi^2 (G[K][K]).  G is one accumulator tile of the fp64 matrix
 * instruction, four pixels an instruction; each of the workgroup's four waves sums a contiguous stripe of pixels and the four
 * partial tiles are added in wave order: no atomics, the same inputs give the same bits, and a star's bits do not depend on the
 * batch it is in.  A pixel with w == 0 contributes nothing whatever the rows or the flux hold there (getspec is NaN outside the
 * model's range); any other NaN reaches chi^2.  Then one thread per star (csrc/lmfit_core.hpp, fp64):
 *   decide   the trial is accepted at the star's first evaluation, or when its chi^2 is finite and <= the best so far.  Accepted:
 *            x_best = x_trial, G becomes the stored matrix, lambda = max(lambda / down, lambda_min).  Rejected: the stored matrix
 *            stays, lambda = min(lambda * up, lambda_max).  chi^2 not finite at the first evaluation: PAYNE_LMFIT_NAN.
 *   solve    S = diag(A_kk^-1/2); (S A S + lambda I) u = S g by Cholesky; delta = S u.  An A_kk that is not positive and finite, a
 *            pivot that is not positive or a delta that is not finite: PAYNE_LMFIT_SINGULAR.
 *   trial    x_trial = clip(x_best + delta, lo, hi); bit k of at_bound says that parameter k was clipped.
 *   stop     with the step actually taken, dx = x_trial - x_best: after an acceptance with max_k |dx_k| sqrt(A_kk) < xtol
 *            PAYNE_LMFIT_CONVERGED; after a rejection of a trial made with lambda == lambda_max PAYNE_LMFIT_STALLED; after
 *            `maxiter` evaluations PAYNE_LMFIT_MAXITER (in this order).
 * A star that is no longer PAYNE_LMFIT_RUNNING is skipped by every later update and its x_trial equals its x_best.
 * payne_lmfit_create: K parameters, room for max_stars stars.  opts NULL: the defaults (lambda0 1e-3, down 10, up 10, lambda_min
 * 1e-12, lambda_max 1e8, xtol 1e-3, maxiter 50).  lambda0 == 0 with lambda_min == 0 is plain Gauss-Newton.
 *   PAYNE_E_INVALID      null out, K < 1, max_stars < 1, an option that is not finite, lambda0 < 0, lambda_min < 0, lambda_max <
 *                        lambda_min, lambda0 outside [lambda_min, lambda_max], down < 1, up < 1, xtol < 0, maxiter < 1
 *   PAYNE_E_UNSUPPORTED  K > 15
 * payne_lmfit_begin: x0_dev DEVICE fp64 [B][K]; lo, hi HOST fp64 [K], the box.  Every star becomes RUNNING with lambda0, no
 * evaluation behind it and x_trial = clip(x0) (at_bound says where).  B stays the handle's batch until the next begin.
 *   PAYNE_E_INVALID      null handle / lo / hi, B outside 0 .. max_stars, null x0_dev with B > 0, lo >= hi or not finite
 * payne_lmfit_trial: the DEVICE pointer of x_trial, fp64 [B][K] (NULL for a null handle); it stays valid for the handle's life.
 * payne_lmfit_update: rows_dev DEVICE fp32 [B][1 + K][ld], row 0 the model at the star's x_trial and row 1 + k its derivative with
 * respect to parameter k; flux_dev DEVICE fp32 [B][ld_f]; w_dev DEVICE fp64 [B][ld_f], the star's own 1 / sigma^2; n pixels.
 * Rows and flux are read 16 bytes a lane where ld and ld_f are multiples of four and the pointers 16-byte aligned, element by
 * element otherwise (the same bits).
 *   PAYNE_E_INVALID      null handle, n < 1, ld < n, ld_f < n, null rows_dev / flux_dev / w_dev with B > 0
 * payne_lmfit_update_poly: the update for a model multiplied by a continuum polynomial that is fitted with it.  The handle's K
 * parameters are Km = K - P of the caller's model m (Km >= 0) and then P Chebyshev coefficients c of p(x) = sum_j c_j T_j(x), in
 * polycalc's basis on payne_contfit_batch's abscissa x_dev, DEVICE fp64 [n], shared by all stars.  rows_dev is [B][1 + Km][ld], the
 * un-normalised model and its Km derivatives as payne_lmfit_update takes them; the coefficients are read from the star's x_trial.
 * The K + 1 rows of R are formed in registers and never stored: p dm/dtheta_i (i < Km), m T_j(x) (i = Km + j) and flux - m p
 * (i = K), p and T_j in fp64 by the recurrence T_k = fma(2 x, T_k-1, -T_k-2), p = fma(c_k, T_k, p) with k ascending.  Pixel order,
 * operand map, the handling of w == 0, NaN and pixels beyond n, both load forms (x_dev 16-byte aligned too for the first) and the
 * step that follows are payne_lmfit_update's, over all K parameters; a star's bits do not depend on its batch.  |x| <= 1 is assumed.
 *   PAYNE_E_INVALID      as payne_lmfit_update, and P < 1, P > K, null x_dev with B > 0
 * payne_lmfit_update_phot: the update for a spectrum and magnitudes fitted together, Gaussian priors included.  The handle's K
 * parameters are, in this order, Km of the spectral model (rows_dev [B][1 + Km][ld] as above), Kp that only the photometry sees (no
 * row: rows Km .. Km + Kp - 1 of the spectral tile are none of R's and stay zero) and P >= 0 Chebyshev coefficients (P == 0: the
 * plain model, x_dev is not read and may be NULL).  The spectral tile is otherwise payne_lmfit_update_poly's (payne_lmfit_update's
 * for P == 0).  The photometric block is what payne_sedfit_jac wrote at the trial point: mags_dev DEVICE fp64 [B][F], dmags_dev
 * DEVICE fp64 [B][F][ncol], ncol 7 or 6; obs_dev, pw_dev DEVICE fp64 [B][F], the observed magnitudes and 1 / sigma^2 (pw == 0: the
 * filter does not count whatever the four arrays hold there, NaN included); sed_col HOST int [K], the column of dmags that parameter
 * k is or -1 for none (Vrad, Vmic, the coefficients).  With R_k = dmags[f][sed_col[k]] (0 for -1) and R_K = obs_f - mag_f, element
 * (i, j), i <= j <= K, of the block is g = 0, then g = fma(R_i pw_f, R_j, g) over the counting filters in ascending order;
 * prior_mu_dev, prior_sigma_dev DEVICE fp64 [B][K] or both NULL add to it as in payne_sedfit_run, at the star's x_trial (a sigma that
 * is not finite and positive: none); then tile[i][j] = tile[i][j] + g, one addition, and the step is payne_lmfit_update's
 * (csrc/lmfit_phot_core.hpp).  No atomics, every sum has a fixed order; a star's bits depend on nothing but its own inputs.
 *   PAYNE_E_INVALID      as payne_lmfit_update; P < 0, Kp < 0, Km < 0, Km + Kp + P != K; null x_dev with P > 0 and B > 0; F < 0, a
 *                        null photometric array with F > 0 and B > 0; ncol other than 6 / 7; null sed_col, an entry outside
 *                        [-1, ncol), -1 for one of the Kp parameters, another than -1 for a coefficient; only one of prior_mu_dev /
 *                        prior_sigma_dev; the box (payne_lmfit_begin's) of the parameter mapped to column ncol - 1, Av, with hi >= 5
 *                        (the model jumps there)
 *   PAYNE_E_UNSUPPORTED  F > 64 (a star's filters are staged in LDS)
 * payne_lmfit_update_pair: the update for a spectrum of two components A and B with a light ratio q, times a continuum polynomial:
 * model = p(x) [(1 - q) m_A + q m_B].  The handle's K parameters are, in this order, Kl that the components see, q, and P >= 0
 * Chebyshev coefficients (P == 0: p == 1, x_dev is not read and may be NULL), K = Kl + 1 + P.  rows_a_dev is DEVICE fp32
 * [B][1 + Ka][ld] and rows_b_dev [B][1 + Kb][ld]: row 0 a component's model at the star's x_trial, row 1 + k its k-th derivative.
 * ia, ib HOST int [Kl]: parameter k is derivative ia[k] of A's block and ib[k] of B's, -1 where the component does not see it; both
 * >= 0 for a parameter the two share.  q and the coefficients are read from the star's x_trial.  The K + 1 rows of R are formed in
 * registers and never stored (csrc/lmfit_pair_core.hpp states every product and fma): p [(1 - q) dm_A[ia] + q dm_B[ib]] (i < Kl),
 * p (m_B - m_A) (i = Kl), [(1 - q) m_A + q m_B] T_j(x) (i = Kl + 1 + j) and flux - p [(1 - q) m_A + q m_B] (i = K), 1 - q rounded once
 * a star.  Pixel order, operand map, the handling of w == 0, NaN and pixels beyond n, both load forms (both row blocks and x_dev
 * 16-byte aligned for the first) and the step that follows are payne_lmfit_update's; a star's bits do not depend on its batch.
 *   PAYNE_E_INVALID      as payne_lmfit_update (either row block); Kl < 0, P < 0, Kl + 1 + P != K, Ka < 0, Kb < 0; null ia / ib with
 *                        Kl > 0, an entry outside [-1, Ka) / [-1, Kb), both -1 for one parameter; null x_dev with P > 0 and B > 0
 * A call that is refused leaves the state untouched.
 * payne_lmfit_result: DEVICE pointers, any may be NULL: x_best fp64 [B][K], chisq fp64 [B] (of x_best), A fp64 [B][K][K] and g fp64
 * [B][K] (at x_best), lambda fp64 [B], status int [B], niter int [B] (evaluations), at_bound unsigned [B].  Copies on `stream`.
 *   PAYNE_E_INVALID      null handle
 * B == 0 succeeds and does nothing; every call is enqueued on `stream` and does not wait.  payne_lmfit_destroy: NULL is allowed. */
#define PAYNE_LMFIT_RUNNING 0
#define PAYNE_LMFIT_CONVERGED 1
#define PAYNE_LMFIT_STALLED 2
#define PAYNE_LMFIT_MAXITER 3
#define PAYNE_LMFIT_SINGULAR 4
#define PAYNE_LMFIT_NAN 5
#define PAYNE_LMFIT_MAX_K 15

typedef struct payne_lmfit_opts {
  double lambda0, down, up, lambda_min, lambda_max, xtol;
  int maxiter;
} payne_lmfit_opts;

typedef struct payne_lmfit payne_lmfit;

int payne_lmfit_create(int device, int K, int max_stars, const payne_lmfit_opts* opts, payne_lmfit** out);
int payne_lmfit_begin(payne_lmfit* h, const double* x0_dev, const double* lo, const double* hi, int B, void* stream);
double* payne_lmfit_trial(payne_lmfit* h);
int payne_lmfit_update(payne_lmfit* h, const float* rows_dev, int ld, const float* flux_dev, const double* w_dev, int ld_f, int n,
                       void* stream);
int payne_lmfit_update_poly(payne_lmfit* h, int P, const float* rows_dev, int ld, const float* flux_dev, const double* w_dev, int ld_f,
                            const double* x_dev, int n, void* stream);
int payne_lmfit_update_phot(payne_lmfit* h, int Km, int Kp, int P, const float* rows_dev, int ld, const float* flux_dev,
                            const double* w_dev, int ld_f, const double* x_dev, int n, int F, int ncol, const int* sed_col,
                            const double* mags_dev, const double* dmags_dev, const double* obs_dev, const double* pw_dev,
                            const double* prior_mu_dev, const double* prior_sigma_dev, void* stream);
int payne_lmfit_update_pair(payne_lmfit* h, int Kl, int P, const int* ia, const int* ib, const float* rows_a_dev, int Ka,
                            const float* rows_b_dev, int Kb, int ld, const float* flux_dev, const double* w_dev, int ld_f,
                            const double* x_dev, int n, void* stream);
int payne_lmfit_result(payne_lmfit* h, double* x_best, double* chisq, double* A, double* g, double* lambda, int* status, int* niter,
                       unsigned* at_bound, void* stream);
void payne_lmfit_destroy(payne_lmfit* h);

/* ---- SED fits for many stars: the magnitudes' derivatives and a whole Levenberg-Marquardt fit in one launch ----
 * payne_sedfit_*: a handle of its own on the per-filter photometric nets (6 -> H -> H -> 1, sigmoids, fp64 arithmetic on fp32
 * weights).  The magnitudes are the likelihood's (GenMod.genphot / genphot_scaled: Rv = 3.1, at Av >= 5 the nets at Av = 0 and the
 * high-Av table), in its own parameters: a row is [Teff, logg, FeH, aFe, logR, Dist, Av] (photscale 0, 7 values) or
 * [Teff, logg, FeH, aFe, logA, Av] (photscale 1, 6 values).  csrc/sedfit_core.hpp holds the arithmetic; in short:
 *   net      forward mode through one filter's net: next to a star's row of activations run the tangents of the network inputs
 *            among Teff, logg, FeH, aFe, Av that are asked for.  A workgroup takes one filter for a block of stars: the rows of its
 *            48-row tile are (star, tangent), 48 / (1 + Kn) stars for Kn tangents; both hidden layers' products run on the fp64
 *            matrix instruction, s(z) and s'(z) = a (1 - a) are applied in LDS, layer 3 and the chain rule are fp64 fma.  The
 *            width is padded to a multiple of 16 with zero weights, which is exact.
 *   chain    d m / d Teff = -dBC/dTeff - 10 / (Teff ln 10); d m / d (logg, FeH, aFe, Av) = -dBC/d(the label); d m / d logR = -5;
 *            d m / d Dist = 5 / (Dist ln 10); d m / d logA = 5.  At Av >= 5, dBC/dAv = -c1 (c2 + c3 Rv + c4 Rv^2) of the table.
 *            Where a magnitude is NaN (a NaN label, no table row at Av >= 5) so are its derivatives.
 *   fit      per star R = [d m / d theta_free ; obs - m] and G = R diag(w) R^T summed over the filters in ascending order, one fma
 *            an element and filter, no atomics; a filter with w == 0 is ignored whatever obs or the model hold there.  A Gaussian
 *            prior on free parameter k adds 1 / sigma_k^2 to A_kk, (mu_k - theta_k) / sigma_k^2 to g_k and its term to chi^2.
 *            The step behind G is payne_lmfit_update's, with its rules and statuses (decide, solve, trial, stop above).
 * A star's bits depend neither on its place in a tile nor on the batch; the same inputs give the same bits.
 * payne_sedfit_create: HOST arrays in fastANN's stacking, w1 [F][H][6], b1 [F][H], w2 [F][H][H], b2 [F][H], w3 [F][H], b3 [F], fp32;
 * xmin, xmax fp64 [6]; hiav fp64 [F][5] or NULL (then a magnitude at Av >= 5 is NaN).  The handle uploads copies of its own.
 *   PAYNE_E_INVALID      null out or array (but hiav), F < 1, H < 1, an xmin / xmax that is not finite or xmax <= xmin
 *   PAYNE_E_UNSUPPORTED  H > 64
 * payne_sedfit_jac: one launch, workgroups over (filter, block of 8 stars).  pars_dev DEVICE fp64 [B][7 | 6]; mags_dev DEVICE fp64
 * [B][F]; dmags_dev DEVICE fp64 [B][F][7 | 6], the derivative with respect to every parameter of the row.
 *   PAYNE_E_INVALID      null handle, B < 0, photscale other than 0 / 1, null pars_dev / mags_dev / dmags_dev with B > 0
 * payne_sedfit_run: the whole fit in one launch.  A workgroup owns 48 / (1 + Kn) stars (Kn: the free parameters among Teff, logg,
 * FeH, aFe, Av) from their first evaluation to their last: it loops over at most opts.maxiter evaluations, in each over the
 * filters, whose weights it streams into LDS, and ends early when none of its stars is RUNNING.  free_mask: bit p set = parameter p
 * of the row is fitted, K of them, in ascending order wherever an array has K entries; the others are read from start_dev and
 * passed through.  start_dev DEVICE fp64 [B][7 | 6]; obs_dev, w_dev DEVICE fp64 [B][F], the magnitudes and 1 / sigma^2; lo, hi HOST
 * fp64 [K], the box (the start is clipped into it); prior_mu_dev, prior_sigma_dev DEVICE fp64 [B][K] or both NULL, a sigma that is
 * not finite and positive meaning no prior on that parameter; opts NULL: payne_lmfit_create's defaults.  Outputs, DEVICE: pars_dev
 * fp64 [B][7 | 6] (x_best), status_dev int [B]; and, each may be NULL, chisq_dev fp64 [B] (priors included), A_dev fp64 [B][K][K]
 * (the normal matrix at x_best, priors included), niter_dev int [B] (evaluations), at_bound_dev unsigned [B] (bit k: free parameter k),
 * nfilt_dev int [B] (filters with w != 0).  A star whose counting filters plus priors are fewer than K is PAYNE_SEDFIT_TOO_FEW: no
 * evaluation, pars the clipped start, chi^2 NaN, A zero.  A NaN in the start or in obs at a counting filter: PAYNE_LMFIT_NAN.
 *   PAYNE_E_INVALID      null handle, B < 0, photscale other than 0 / 1, free_mask 0 or with a bit beyond the row, null lo / hi, lo >=
 *                        hi or not finite, Av free with hi >= 5 (the model jumps there), an option payne_lmfit_create rejects, only
 *                        one of prior_mu_dev / prior_sigma_dev, null start_dev / obs_dev / w_dev / pars_dev / status_dev with B > 0
 * B == 0 succeeds and does nothing; both calls are enqueued on `stream` and do not wait.  payne_sedfit_destroy: NULL is allowed. */
#define PAYNE_SEDFIT_TOO_FEW 6
#define PAYNE_SEDFIT_MAX_K 7

typedef struct payne_sedfit payne_sedfit;

int payne_sedfit_create(int device, int F, int H, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                        const float* b3, const double* xmin, const double* xmax, const double* hiav, payne_sedfit** out);
int payne_sedfit_jac(payne_sedfit* h, const double* pars_dev, int B, int photscale, double* mags_dev, double* dmags_dev, void* stream);
int payne_sedfit_run(payne_sedfit* h, int photscale, unsigned free_mask, const double* start_dev, const double* obs_dev,
                     const double* w_dev, int B, const double* lo, const double* hi, const double* prior_mu_dev,
                     const double* prior_sigma_dev, const payne_lmfit_opts* opts, double* pars_dev, double* chisq_dev, double* A_dev,
                     int* status_dev, int* niter_dev, unsigned* at_bound_dev, int* nfilt_dev, void* stream);
void payne_sedfit_destroy(payne_sedfit* h);

/* ---- template-bank chi^2 search: every star against every template, the best few per star ----
 * payne_tmatch_*: chi^2[s][t] = sum_p w[s][p] (flux[s][p] - m[t][p])^2 for N stars and M templates on one pixel grid, expanded into
 * one N x M matrix product over 2 n terms on the fp64 matrix instruction, and per star the topk smallest (starting points for
 * payne_lmfit_*).  csrc/tmatch_core.hpp holds the arithmetic and its order; in short:
 *   value    chi^2 = c0[s] + sum_p (a1 (-2 m) + a2 m^2) with a1 = w f (rounded once), a2 = w, c0 = sum_p a1 f, everything fp64; m is
 *            widened first, so -2 m and m^2 are exact.  The error against the direct sum is at most (2 n + 4) 2^-53 (sum w f^2 +
 *            2 sum |w f m| + sum w m^2): the expansion cancels, but in fp64.
 *   pixels   a pixel with w == 0, or beyond n, contributes nothing whatever the flux or the templates hold there (NaN, 1e30): both
 *            operands are replaced by zero by a select.  A flux, weight or template value that is not finite at a pixel with w != 0
 *            makes that chi^2 NaN (for a template value: of that (star, template) pair only).  ld - n padding is never read.
 *   lists    per star the topk smallest chi^2 ascending, equal values in ascending template index; NaN never enters; a slot that
 *            cannot be filled (topk > M, or fewer templates that are not NaN) has idx = -1 and chisq = +inf.
 *   order    the grid is (tiles of 64 stars) x (chunks of payne_tmatch_chunk() templates); a workgroup leaves its chunk's list in the
 *            handle's workspace and a second small launch merges a star's chunks in chunk order.  No atomics: the same inputs give
 *            the same bytes, with or without all_dev, and a star's bytes do not depend on the other stars of the call.
 * payne_tmatch_create: room for max_stars stars and max_templates templates a call; the handle owns only the workspace
 * (ceil(max_templates / chunk) * max_stars * 8 entries of 12 bytes).
 *   PAYNE_E_INVALID      null out, max_stars < 1, max_templates < 1
 * payne_tmatch_match: templates_dev DEVICE fp32 [M][ld_t]; flux_dev DEVICE fp32 [N][ld_f]; w_dev DEVICE fp64 [N][ld_f], each star's
 * own 1 / sigma^2; n pixels; idx_dev DEVICE int32 [N][topk], chisq_dev DEVICE fp64 [N][topk]; all_dev DEVICE fp64 [N][ld_a], every
 * chi^2, or NULL.  Checked before anything reaches the device:
 *   PAYNE_E_INVALID      null handle, topk outside 1 .. PAYNE_TMATCH_MAX_TOPK, N outside 0 .. max_stars, M outside 0 .. max_templates,
 *                        n < 1, ld_t < n, ld_f < n; with N > 0 and M > 0: a null templates_dev / flux_dev / w_dev / idx_dev /
 *                        chisq_dev, ld_a < M with all_dev
 *   PAYNE_E_UNSUPPORTED  more than 65535 chunks of templates (M > 65535 * payne_tmatch_chunk())
 * N == 0 or M == 0 succeeds and does nothing; the call is enqueued on `stream` and does not wait; payne_last_error(NULL) has the
 * message of a failure.  Two calls on one handle share its workspace, so they belong on one stream.  payne_tmatch_destroy: NULL is
 * allowed. */
#define PAYNE_TMATCH_MAX_TOPK 8

typedef struct payne_tmatch payne_tmatch;

int payne_tmatch_create(int device, int max_stars, int max_templates, payne_tmatch** out);
int payne_tmatch_match(payne_tmatch* h, const float* templates_dev, int ld_t, int M, const float* flux_dev, const double* w_dev, int ld_f,
                       int N, int n, int topk, int* idx_dev, double* chisq_dev, double* all_dev, long long ld_a, void* stream);
int payne_tmatch_chunk(void);
void payne_tmatch_destroy(payne_tmatch* h);

/* The search with a free continuum polynomial per (star, template) pair:
 *   chi^2[s][t] = min_c sum_p w[s][p] (flux[s][p] - m[t][p] sum_j c_j T_j(x[p]))^2, c the P <= PAYNE_TMATCH_MAX_POLY Chebyshev
 * coefficients in payne_contfit_batch's basis and abscissa x (|x| <= 1) -- the chi^2 that payne_contfit_batch and
 * payne_lmfit_update_poly minimise.  3 P - 1 matrix products over n on the fp64 matrix instruction (b_j = sum (w f T_j) m,
 * S_q = sum (w T_q) m^2, q <= 2 P - 2), A_jk = (S_{j+k} + S_{|j-k|}) / 2, A c = b by the scaled Cholesky solve, and
 * chi^2 = c0 + c^T A c - 2 c^T b; csrc/tmatch_poly_core.hpp holds the arithmetic and its order.  The rules are payne_tmatch_match's
 * except:
 *   NaN      a pair is also NaN when the star has fewer than P pixels with w != 0 or when the solve refuses (a template that is zero
 *            at every such pixel).  So a star without a weighted pixel lists nothing (idx -1, chisq +inf), where
 *            payne_tmatch_match lists chi^2 = 0 for it.
 *   lists    every entry carries its coefficients: coef_dev DEVICE fp64 [N][topk][P] (NaN where idx is -1) and flags_dev DEVICE
 *            int32 [N][topk]: bit 0 is set when the polynomial is > 0 at every pixel of the star with w != 0.  A template whose
 *            polynomial turns negative stays listed.
 *   order    the grid is (tiles of payne_tmatch_poly_stars() stars) x (chunks of payne_tmatch_poly_chunk() templates).
 * payne_tmatch_create_poly: payne_tmatch_create plus the workspace of match_poly for P <= max_poly; payne_tmatch_match works on
 * such a handle as on any other.  PAYNE_E_INVALID as payne_tmatch_create, and max_poly outside 1 .. PAYNE_TMATCH_MAX_POLY.
 * payne_tmatch_match_poly: x_dev DEVICE fp64 [n]; the other arrays as payne_tmatch_match's.  PAYNE_E_INVALID as payne_tmatch_match,
 * and P outside 1 .. the handle's max_poly (a handle of payne_tmatch_create has max_poly = 0), a null x_dev / coef_dev / flags_dev.
 * Nothing is touched on a refusal; N == 0 or M == 0 succeeds and does nothing. */
#define PAYNE_TMATCH_MAX_POLY 8

int payne_tmatch_create_poly(int device, int max_stars, int max_templates, int max_poly, payne_tmatch** out);
int payne_tmatch_match_poly(payne_tmatch* h, const float* templates_dev, int ld_t, int M, const float* flux_dev, const double* w_dev,
                            int ld_f, int N, int n, const double* x_dev, int P, int topk, int* idx_dev, double* chisq_dev,
                            double* coef_dev, int* flags_dev, double* all_dev, long long ld_a, void* stream);
int payne_tmatch_poly_stars(void);
int payne_tmatch_poly_chunk(void);

/* The search against PAIRS of templates with both amplitudes free, the starting points of payne_lmfit_update_pair's fit:
 *   chi^2[s][a][b] = min over (alpha, beta) of sum_p w[s][p] (flux[s][p] - alpha m[a][p] - beta m[b][p])^2;
 * alpha + beta is the two-component fit's scale and beta / (alpha + beta) its light ratio.  The primary a runs over the kA <=
 * PAYNE_TMATCH_MAX_PRIMARIES templates that cand_dev names per star, the secondary b over the whole bank.  Three enqueued launches:
 * the moments B[s][t] = sum (w f) m_t, S[s][t] = sum w m_t^2 and c0[s] (N x M, the plain search's tile with its two products kept
 * apart); the cross term X = sum (w m_a) m_b as one (N kA) x M matrix product over n (row s kA + j is star s with primary
 * cand[s][j]), the 2 x 2 solve and the rows' lists per chunk; the merge.  csrc/tmatch_pair_core.hpp holds the arithmetic and its
 * order.  D = fma(-X, X, Sa Sb), alpha = (Ba Sb - Bb X) / D, beta = (Bb Sa - Ba X) / D and
 * chi^2 = c0 + alpha^2 Sa + 2 alpha beta X + beta^2 Sb - 2 (alpha Ba + beta Bb), within (2 n + 16) 2^-53 of the terms' magnitudes.
 * The rules are payne_tmatch_match's except:
 *   NaN      a pair is NaN and never listed when a == b; when cand[s][j] lies outside 0 .. M - 1 (-1 marks an unused slot); when
 *            either template is not finite at a pixel of the star with w != 0; when Sa or Sb is not > 0 (so a star without a
 *            weighted pixel lists nothing); when the pair is collinear, not (D > 2^-20 Sa Sb); when alpha or beta is not > 0 (one
 *            template with a scale fits as well: payne_tmatch_match_poly with P = 1); when b is one of the star's primaries in an
 *            earlier slot j' < j (that pair is (j', a): an unordered pair is listed once).
 *   lists    ascending in (chi^2, slot j, b).  idx_a_dev and idx_b_dev DEVICE int32 [N][topk] hold TEMPLATE indices (not slots), -1
 *            in an empty slot; chisq_dev DEVICE fp64 [N][topk], +inf there; amp_dev DEVICE fp64 [N][topk][2] holds (alpha, beta),
 *            NaN there.  all_dev DEVICE fp64 [N kA][ld_a], every chi^2 of every row, or NULL.
 *   order    the cross launch's grid is (tiles of payne_tmatch_pair_rows() rows) x (chunks of payne_tmatch_pair_chunk() templates);
 *            the merge walks a star's rows in j order and each row's chunks in chunk order.  No atomics: the same inputs give the
 *            same bytes, with or without all_dev, and a star's bytes do not depend on the other stars of the call.
 *   cand     a primary named twice for one star is the caller's error: its pairs are listed twice.
 * payne_tmatch_create_pairs: payne_tmatch_create plus the workspace of match_pairs: the moments (2 max_stars max_templates + max_stars
 * doubles) and the lists of max_stars * max_primaries rows (ceil(max_templates / chunk) * rows * 8 entries of 28 bytes).
 * payne_tmatch_match works on such a handle as on any other.  PAYNE_E_INVALID as payne_tmatch_create, and max_primaries outside
 * 1 .. PAYNE_TMATCH_MAX_PRIMARIES.
 * payne_tmatch_match_pairs: cand_dev DEVICE int32 [N][kA]; the other inputs as payne_tmatch_match's.  PAYNE_E_INVALID as
 * payne_tmatch_match, and kA outside 1 .. the handle's max_primaries (a handle of payne_tmatch_create has 0), a null cand_dev /
 * idx_a_dev / idx_b_dev / amp_dev.  Nothing is touched on a refusal; N == 0 or M == 0 succeeds and does nothing. */
#define PAYNE_TMATCH_MAX_PRIMARIES 16

int payne_tmatch_create_pairs(int device, int max_stars, int max_templates, int max_primaries, payne_tmatch** out);
int payne_tmatch_match_pairs(payne_tmatch* h, const float* templates_dev, int ld_t, int M, const float* flux_dev, const double* w_dev,
                             int ld_f, int N, int n, const int* cand_dev, int kA, int topk, int* idx_a_dev, int* idx_b_dev,
                             double* chisq_dev, double* amp_dev, double* all_dev, long long ld_a, void* stream);
int payne_tmatch_pair_rows(void);
int payne_tmatch_pair_chunk(void);

/* ---- continuum polynomials: the blaze's Chebyshev coefficients for many stars against a given model row each ----
 * payne_contfit_batch: per star the c [P] that minimise chi^2 = sum_p w_p (f_p - m_p sum_j c_j T_j(x_p))^2, the likelihood's own
 * objective in its pc_* parameters (modpoly: model x polycalc) for a fixed model, which is linear least squares; optional
 * kappa-sigma clipping; and the spectrum divided by the polynomial with its weights carried along, sum w (f - m p)^2 =
 * sum (w p^2) (f / p - m)^2.  One stateless call, one 256-thread workgroup a star, enqueued on `stream`; nothing waits.
 * csrc/contfit_core.hpp holds the arithmetic and its order; in short, per star:
 *   pixels   a pixel counts if w != 0.  One with w == 0 is ignored whatever flux and model hold there (NaN, 1e30), by a select, as
 *            in payne_lmfit_update and payne_tmatch_match.  A counting pixel whose flux, model or weight is not finite: status NAN.
 *            A model_index outside [0, n_models): BAD_MODEL, and nothing is read through it.
 *   sums     R [P + 1][n]: R_j = m T_j(x) (T by the three-term recurrence in fp64), R_P = f.  G = R diag(w_kept) R^T on the fp64
 *            matrix instruction with payne_lmfit_update's operand map and pixel order; four partial tiles added in wave order, no
 *            atomics.  G holds the normal matrix, the right-hand side G[j][P] and sum w f^2 = G[P][P].
 *   solve    one thread: the matrix scaled to a unit diagonal, Cholesky, c; chi^2 = e^T G e with e = (c, -1), that is
 *            G[P][P] - 2 c.b + c^T A c (no second pass over the residuals: without clipping every pixel is read once for the fit).
 *            A diagonal entry or pivot that is not positive, or a c or chi^2 that is not finite: SINGULAR.  Fewer kept pixels than
 *            P: TOO_FEW.
 *   clipping nclip > 0: z_p = sqrt(w_p) (f_p - m_p p(x_p)) over every counting pixel (a pixel may come back); s = 1 or, with
 *            `rescale`, sqrt(max(chi^2, 0) / max(1, kept - P)); kept iff -kappa_lo s <= z_p <= kappa_hi s.  The fit is repeated on
 *            the kept pixels until the mask does not change, at most nclip times.  rounds = the solves that succeeded; npix = the
 *            kept pixels of the last solve (of the attempt that failed, for TOO_FEW / SINGULAR / NAN; 0 for BAD_MODEL), chisq is
 *            over them.
 *   outputs  flux_out = f / p rounded to fp32 (for every pixel: NaN where the flux is NaN), w_out = (w p) p; w_out = 0 for a pixel
 *            that does not count and, with drop_clipped, for a pixel the last solve did not keep.  Where p <= 0 or is not finite
 *            w_out = 0 and flux_out = 0; on a counting pixel that makes the status NONPOSITIVE (whether or not output rows were
 *            asked for), and the coefficients are still reported.  NAN, SINGULAR, TOO_FEW, BAD_MODEL: coefficients and chi^2 are
 *            NaN, w_out = 0 and flux_out = the input flux.  Nothing is written beyond column n of a row or beyond [N][P].
 * The same inputs give the same bytes, and a star's bytes do not depend on the batch it is in.  Rows are read (and written) 16
 * bytes a lane where ld_f, ld_m, ld_o are multiples of four and every pointer is 16-byte aligned, element by element otherwise
 * (the same bytes).
 * flux_dev DEVICE fp32 [N][ld_f], w_dev DEVICE fp64 [N][ld_f]; model_dev DEVICE fp32 [n_models][ld_m]; model_index_dev DEVICE int
 * [N], or NULL: star s uses row s; x_dev DEVICE fp64 [n], polycalc's abscissa in [-1, 1]; coef_dev fp64 [N][P], chisq_dev fp64 [N],
 * npix_dev, status_dev, rounds_dev int [N]; flux_out_dev fp32 [N][ld_o] and w_out_dev fp64 [N][ld_o], each may be NULL.
 *   PAYNE_E_INVALID      null opts, P outside 1 .. PAYNE_CONTFIT_MAX_P, nclip outside 0 .. PAYNE_CONTFIT_MAX_NCLIP, a kappa that is
 *                        not positive, N < 0, n < 1, ld_f < n, ld_m < n, n_models < 1, n_models < N without model_index_dev, ld_o < n
 *                        with an output row; with N > 0 a null flux_dev / w_dev / model_dev / x_dev / coef_dev / chisq_dev /
 *                        npix_dev / status_dev / rounds_dev
 *   PAYNE_E_UNSUPPORTED  n > PAYNE_CONTFIT_MAX_N (the clipping mask is a bit set in LDS)
 * N == 0 succeeds and does nothing; payne_last_error(NULL) has the message of a failure. */
#define PAYNE_CONTFIT_OK 0
#define PAYNE_CONTFIT_NONPOSITIVE 1
#define PAYNE_CONTFIT_TOO_FEW 2
#define PAYNE_CONTFIT_SINGULAR 3
#define PAYNE_CONTFIT_NAN 4
#define PAYNE_CONTFIT_BAD_MODEL 5
#define PAYNE_CONTFIT_MAX_P 15
#define PAYNE_CONTFIT_MAX_NCLIP 16
#define PAYNE_CONTFIT_MAX_N 262144

typedef struct payne_contfit_opts {
  int P, nclip, rescale, drop_clipped;
  double kappa_lo, kappa_hi;
} payne_contfit_opts;

int payne_contfit_batch(int device, const float* flux_dev, const double* w_dev, long long ld_f, const float* model_dev, long long ld_m,
                        int n_models, const int* model_index_dev, const double* x_dev, int N, int n, const payne_contfit_opts* opts,
                        double* coef_dev, double* chisq_dev, int* npix_dev, int* status_dev, int* rounds_dev, float* flux_out_dev,
                        double* w_out_dev, long long ld_o, void* stream);

/* Magnitudes for B parameter vectors: FastPayneSEDPredict.sed
 * (Payne/predict/predictsed.py:75-103).  pars: device fp64 [B][9] =
 * logt, logg, feh, afe, av, rv, logl, dist, logA  (NaN = kwarg absent; the
 * (logl, dist) form wins over logA as in the reference).  mags: device fp64 [B][F]. */
int payne_sed_batch(payne_ctx* ctx, const double* pars, int B, double* mags, void* stream);

/* Bolometric corrections for B label vectors: fastANN.eval
 * (Payne/predict/photANN.py:125-131).  x: device fp64 [B][6] = Teff, logg, feh, afe,
 * av, rv; bc: device fp64 [B][F]. */
int payne_bc_batch(payne_ctx* ctx, const double* x, int B, double* bc, void* stream);

/* ---- device-side sampler step ------------------------------------
 * The reference evaluates prior.priortrans(u) and lnprobfn(v) one vector at a time on the host
 * (Payne/fitting/prior.py:126-272, Payne/fitting/fitstar.py:647-659; 334 us per priortrans call).
 * A batched sampler would be host-bound by that, so the unit-cube -> parameter transform, the
 * additive ln-priors, the assembly of theta rows and the random-walk proposal loop run on the
 * GPU; the host only launches and reads back the survivors. */
#define PAYNE_MAX_DIM 24
#define PAYNE_MAX_FIXED 16
#define PAYNE_PRIOR_UNIFORM 0    /* p = lo, hi                 (max-min)*u+min          prior.py:153-157 */
#define PAYNE_PRIOR_GAUSSIAN 1   /* p = mu, sigma              norm.ppf                 prior.py:158-159 */
#define PAYNE_PRIOR_TGAUSSIAN 2  /* p = lo, hi, mu, sigma      truncnorm.ppf, inf -> hi prior.py:161-166 */
#define PAYNE_PRIOR_EXP 3        /* p = loc, scale             expon.ppf                prior.py:167-168 */
#define PAYNE_PRIOR_TEXP 4       /* p = lo, hi, scale          truncexpon.ppf, inf -> hi prior.py:169-174 */
#define PAYNE_PRIOR_LOGUNIFORM 5 /* p = lo, hi */
#define PAYNE_PRIOR_TABLE 6      /* p[0] * np.interp(u, adv.tab_cdf, adv.tab_val): Dist under a GAL prior = 1000 * gal_ppf(u)
                                  * (prior.py:231-234 -> advancedpriors.py:665-670); one such dimension per sampler */

typedef struct payne_prior_dim {
  int kind;      /* PAYNE_PRIOR_* */
  int theta_col; /* column of the theta row this sampled dimension fills (payne_theta_cols layout) */
  double p[4];
  int has_gauss; /* additive ln-prior -0.5((v-mu)/sigma)^2      prior.py:388-390 */
  int has_box;   /* -inf outside [box_lo, box_hi]               prior.py:391-394 */
  double g_mu, g_sigma, box_lo, box_hi;
} payne_prior_dim;

/* The priors on DERIVED quantities prior.lnpriorfn adds (Payne/fitting/prior.py:286-336, :425-465 via
 * Payne/fitting/advancedpriors.py:93-137, :691-733): everything below is off when zero-initialised.
 * A parameter they need is named by the sampled dimension that carries it (dim_* >= 0) or, when it is fixed or absent
 * (dim_* < 0), by its value (NaN = absent). */
typedef struct payne_adv_priors {
  int imf;   /* + imf_lnprior(mass), Kroupa (alpha 1.3 / 2.3, break 0.5, -inf at <= 0.08), mass = 10^(logg + 2 logR - 4.437) */
  int vrot;  /* + vrot_lnprior(Vrot, mass, eep = 350, logg); mass = 10^(logg + 2 logR) when both are finite and
              * vrot_mass_one == 0, else 1 (prior.py:320-334: a photscale fit has no radius) */
  int vrot_mass_one;
  int dim_logg, dim_logr, dim_vrot;
  double val_logg, val_logr, val_vrot;
  int plx_dim;          /* dimension holding Dist for the derived 'Parallax' = 1000 / Dist (prior.py:449-451); < 0: none */
  int plx_has_gauss, plx_has_box;
  double plx_mu, plx_sigma, plx_lo, plx_hi;
  const double* tab_cdf; /* HOST [tab_n], non-decreasing in [0, 1]: abscissae of PAYNE_PRIOR_TABLE (copied at create) */
  const double* tab_val; /* HOST [tab_n] */
  int tab_n;
} payne_adv_priors;

typedef struct payne_sampler_desc {
  int ndim; /* <= PAYNE_MAX_DIM */
  payne_prior_dim dims[PAYNE_MAX_DIM];
  int n_fixed; /* 'fixed' parameters merged into every theta row (likelihood.py:47-48) */
  int fixed_col[PAYNE_MAX_FIXED];
  double fixed_val[PAYNE_MAX_FIXED];
  payne_adv_priors adv;
} payne_sampler_desc;

typedef struct payne_sampler payne_sampler;

int payne_sampler_create(payne_ctx* ctx, const payne_sampler_desc* desc, int k_max, payne_sampler** out);
void payne_sampler_destroy(payne_sampler* s);

/* v = priortrans(u) for K unit-cube vectors.  u, v: device fp64 [K][ndim]. */
int payne_prior_transform_batch(payne_sampler* s, const double* u, int K, double* v, void* stream);

/* v = priortrans(u); lnprob = lnprior(v) + lnlike(v)  (lnprobfn over a batch).
 * u, v: device fp64 [K][ndim]; lnprob: device fp64 [K]. */
int payne_lnprob_u_batch(payne_sampler* s, const double* u, int K, double* v, double* lnprob, void* stream);

/* `walks` Metropolis steps for K lock-step chains under the constraint lnprob > loglstar
 * (the 'rwalk' proposal of the nested sampler): u' = u + scale * (axes . z), z uniform in the
 * unit ball; a step is accepted iff u' is inside the unit cube and lnprob(u') > loglstar.
 * u, v: device fp64 [K][ndim] in/out (chain positions); lnprob: device fp64 [K] in/out;
 * axes: HOST fp64 [ndim][ndim] row-major; nacc, ncall: device int32 [K] (accepted steps,
 * likelihood calls) overwritten (zeroed by the walk's first step).  One small kernel + one payne_lnlike_batch for the first
 * step; the steps after it ride in the likelihood batch's own launches (payne_sampler_counters). */
int payne_rwalk_batch(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes,
                      double scale, double loglstar, int walks, unsigned long long seed, int* nacc, int* ncall,
                      void* stream);

/* ---- host-side nested-sampling bookkeeping (no GPU work) ---------------------------------
 * Replaces the per-iteration body of dynesty's sampling loop as the reference drives it
 * (Payne/fitting/fitstar.py:332-338: one 15-tuple per dead point) for a QUEUE of proposals
 * evaluated in one GPU batch: worst live point, trapezoid evidence update, replacement by the
 * next queued proposal with lnprob > threshold.  All arrays are the caller's. */
typedef struct payne_ns_state {
  int nlive, ndim;
  long long it;            /* iteration number of the next dead point (starts at 1) */
  long long pending_nc;    /* likelihood calls spent since the last accepted replacement */
  double logz, logzvar, h, logvol, loglstar;   /* start: -1e300, 0, 0, 0, -1e300 */
} payne_ns_state;

typedef struct payne_ns_dead {          /* one row per dead point, capacity `cap` rows */
  int* worst;       double* u;          /* [cap], [cap][ndim] */
  double* v;        double* logl;       /* [cap][ndim], [cap] */
  double* logvol;   double* logwt;
  double* logz;     double* logzvar;
  double* h;        int* nc;
  int* worst_it;    double* delta_logz;
} payne_ns_dead;

#define PAYNE_NS_QUEUE_EMPTY 0   /* every queued proposal was used or rejected */
#define PAYNE_NS_CONVERGED   1   /* ln(1 + L_max X / Z) < dlogz */
#define PAYNE_NS_LIMIT       2   /* max_emit or the record capacity reached */
#define PAYNE_NS_LOGL_MAX    3   /* worst live lnprob >= logl_max */

/* live_*: [nlive][ndim] / [nlive], updated in place.  q*: the proposal queue in order
 * ([nq][ndim], [nq]; qnc = likelihood calls behind each proposal).  Returns the number of dead
 * points written to `out` (>= 0) or a negative error code; *consumed = queue entries used up,
 * *stop = one of PAYNE_NS_*. */
int payne_ns_consume(payne_ns_state* s, double* live_u, double* live_v, double* live_logl, int* live_it,
                     const double* qu, const double* qv, const double* ql, const int* qnc, int nq,
                     double dlogz, long long max_emit, double logl_max, payne_ns_dead* out, int cap,
                     int* consumed, int* stop);

/* The live set and the threshold as payne_ns_consume WILL leave them once it has walked the whole queue (replacements only:
 * no evidence arithmetic, no records, no stop condition but the queue's end), into copies out_* of the live arrays;
 * *loglstar is written only when *n_dead > 0.  The batched sampler starts its next queue of proposals from this state and
 * consumes the current one while the GPU walks (no reference counterpart: dynesty proposes one point at a time). */
int payne_ns_peek(int nlive, int ndim, const double* live_u, const double* live_v, const double* live_logl, const double* qu,
                  const double* qv, const double* ql, int nq, double* out_u, double* out_v, double* out_logl, double* loglstar,
                  int* n_dead);

/* Bounding ellipsoid(s) of n live points u[n][ndim] (unit cube): dynesty's bound='single' (multi = 0) or
 * 'multi' (recursive 2-means split while the children hold less than half the parent's volume, at most
 * max_ell <= PAYNE_MAX_ELL pieces).  Outputs, one entry per ellipsoid {ctr + axes z, |z| <= 1}: ctr [.][ndim],
 * axes / axes_unit (the cluster's Cholesky factor scaled to hold its points, resp. by sqrt(ndim+2)) / ainv
 * (inverse of axes) [.][ndim][ndim] row-major, logvol [.] (up to the unit ball's volume); *n_ell = count. */
int payne_ns_bound(const double* u, int n, int ndim, double enlarge, int multi, int max_ell, double* ctr,
                   double* axes, double* axes_unit, double* ainv, double* logvol, int* n_ell);

/* Text rows of the output table (fitstar.py:345-371: "Iter <pars> log(lk) log(vol) log(wt) h nc log(z)
 * delta(log(z))", every value as Python's str() writes it): vals host fp64 [m][ncol], is_int[c] marks integer
 * columns; each value is followed by a blank, each row by a newline.  Returns bytes written (< 0: error; 48
 * bytes per value always suffice). */
long long payne_format_rows(const double* vals, int m, int ncol, const int* is_int, char* out, long long cap);

/* payne_rwalk_batch in two parts: `begin` takes the same arguments and enqueues the set-up, `step(s, w)` for
 * w = 0 .. walks enqueues one step (settle proposal w-1, draw and evaluate proposal w; the last only settles).
 * A caller driving several samplers (one context and one stream each) interleaves their steps from one host
 * thread to keep two independent batches in flight. */
int payne_rwalk_begin(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes,
                      double scale, double loglstar, int walks, unsigned long long seed, int* nacc, int* ncall,
                      void* stream);
int payne_rwalk_step(payne_sampler* s, int w);

/* `begin` for a multi-ellipsoid bound (dynesty bound='multi' as fitstar.py:314 passes it): axes is HOST fp64
 * [n_ell][ndim][ndim], ell is HOST int32 [K] naming the ellipsoid whose axes shape chain k's steps (NULL with
 * n_ell == 1 is payne_rwalk_begin). */
#define PAYNE_MAX_ELL 32
int payne_rwalk_begin_ell(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes,
                          int n_ell, const int* ell, double scale, double loglstar, int walks,
                          unsigned long long seed, int* nacc, int* ncall, void* stream);

/* One queue of random-walk proposals of the batched static sampler, start to finish (the body of the sampler's "fill the
 * queue" step: what dynesty does per proposal in sample_rwalk + the pool's queue, Payne/fitting/fitstar.py:309-338): K
 * chains start from live points drawn at random (splitmix of `seed`); with n_ell > 1 each steps in the metric of an
 * ellipsoid that holds its start point (ctr [n_ell][ndim] / ainv [n_ell][ndim][ndim] of payne_ns_bound; else the nearest);
 * upload, `walks` Metropolis steps under lnprob > loglstar on the device (payne_rwalk_begin_ell / _step; a proposal that
 * leaves the unit cube is redrawn without a likelihood call, as dynesty does), download, and the chains that moved at
 * least once become the queue: qu, qv [nq][ndim], ql [nq] (NaN -> -inf), qnc [nq] (likelihood calls behind each), HOST
 * arrays of capacity K owned by the caller.  stats[0..3] = accepted steps, likelihood calls, redrawn proposals, calls of the
 * chains that never moved.  live_*: HOST; axes_unit: HOST [n_ell][ndim][ndim].  Synchronises `stream`. */
int payne_ns_rwalk_queue(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl, int nlive,
                         int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv, double scale,
                         double loglstar, int walks, unsigned long long seed, double* qu, double* qv, double* ql, int* qnc,
                         int* nq, long long* stats, void* stream);

/* The same in two parts: _begin returns when everything is enqueued on `stream` (nothing of its host arguments is read
 * afterwards), _end waits for the stream and writes the queue.  Between the two the host is free: the batched sampler computes
 * the bounding ellipsoids of its NEXT update there (thepayne_amd/sampler/nested.py, overlap_bound). */
int payne_ns_rwalk_queue_begin(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl, int nlive,
                               int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv, double scale,
                               double loglstar, int walks, unsigned long long seed, void* stream);
int payne_ns_rwalk_queue_end(payne_sampler* s, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats);

/* One turn of a loop that keeps a queue in flight: _end of the queue in flight (-> qu .. stats), the step scale adapted to its
 * acceptance (*scale in/out: scale * exp((acc / (calls + redrawn) - 0.5) / ndim / 0.5), clamped to [1e-4, 4]), payne_ns_peek of
 * that queue against the live arrays (*loglstar in: the current threshold; out: the one the queue's consumption will leave;
 * *n_dead: the dead points it will give), and _begin of the next queue from the predicted state, on the stream of the queue
 * collected.  The caller consumes the collected queue (payne_ns_consume) while the GPU walks. */
int payne_ns_rwalk_queue_turn(payne_sampler* s, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats,
                              const double* live_u, const double* live_v, const double* live_logl, int nlive, int K,
                              const double* axes_unit, int n_ell, const double* ctr, const double* ainv, double* scale,
                              double* loglstar, int walks, unsigned long long seed, int* n_dead);

/* How the chain steps of this sampler ran so far: out[0] at the tail of the likelihood-only post kernel (the workgroup of
 * candidate k settles chain k's proposal as soon as it has the likelihood and takes the next one from the two that idle workgroups
 * of the batch's hidden-layer launch made ahead, one per outcome -- or draws it there: PAYNE_V_NO_WALK_SPEC), out[1] as launches of
 * their own (the first step of every walk; every step under PAYNE_V_NO_WALK_TAIL, with an LSF, or when the spectrum length
 * has no likelihood-only kernel; every round of a slice walk).  Measurement / test aid, no reference counterpart. */
int payne_sampler_counters(const payne_sampler* s, long long out[2]);

/* Slice sampling ('slice' / 'rslice' of Payne/fitting/fitstar.py:292-295, samplemethod / slices=) for K lock-step chains under
 * lnprob > loglstar, the chain on the device.  dynesty proposes one point at a time; here every chain is a state machine that
 * asks for one likelihood per ROUND -- an end of its window while it steps out, a point of the window while it shrinks --, a
 * round is one small kernel and one likelihood batch, and the host enqueues rounds without looking at the chains.  Per
 * direction: the window left = u - r axis, right = u + (1 - r) axis (r uniform), stepped out by one axis length while an end
 * beats the threshold, then sampled uniformly and shrunk towards u until a point beats it (given up after 200 shrinks: the point
 * stays).  A point outside the open unit cube is -inf without a likelihood call.  Directions: random_dirs = 0 ('slice') `slices`
 * sweeps over the ndim columns of the chain's ellipsoid matrix, each sweep in an order of its own; random_dirs = 1 ('rslice')
 * `slices` directions axes . z with z a random unit vector; all scaled by `scale`.  Draws are counter-based on (seed, chain,
 * direction, draw), so a chain does not depend on how its rounds are grouped into calls.
 * u, v: device fp64 [K][ndim] in/out; lnprob: device fp64 [K] in/out; axes: HOST fp64 [n_ell][ndim][ndim] row-major, COLUMNS =
 * axes; ell: HOST int32 [K] naming each chain's matrix (NULL with n_ell == 1); ncall, nexpand, ncontract: device int32 [K]
 * (values asked for -- in the cube or not --, of which window ends, of which points of the window), overwritten: the walk's
 * first round starts them at zero.  `begin` enqueues the uploads only; it fails with PAYNE_E_INVALID while a random walk or a
 * queue is open on the sampler (the two share the pending proposal's buffers), as payne_rwalk_begin does while a slice walk is. */
int payne_slice_begin(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes, int n_ell,
                      const int* ell, double scale, double loglstar, int slices, int random_dirs, unsigned long long seed,
                      int* ncall, int* nexpand, int* ncontract, void* stream);

/* n >= 1 rounds of the walk begun (fitstar.py:292-295; dynesty proposes one point at a time, a round is one point for EVERY
 * chain), then one closing launch that settles what is pending, then a wait for the stream: *n_active = the chains that have not
 * finished -- the one word the host reads.  A later call continues the same walk; it is closed when *n_active == 0 (or by the
 * next payne_slice_begin).  An unfinished chain's point is its start point or a point that beat the threshold. */
int payne_slice_rounds(payne_sampler* s, int n, int* n_active);

/* begin + rounds(chunk) until no chain is active or max_rounds rounds are spent (fitstar.py:292-295 as above; dynesty proposes
 * one point at a time): PAYNE_OK with *n_active > 0 in the second case, the walk closed either way.  `chunk` trades rounds run
 * with every chain finished (at most chunk - 1) for host turns. */
int payne_slice_batch(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes, int n_ell,
                      const int* ell, double scale, double loglstar, int slices, int random_dirs, unsigned long long seed,
                      int* ncall, int* nexpand, int* ncontract, void* stream, int chunk, int max_rounds, int* n_active);

/* The proposal queue's TURN on the device.  payne_ns_rwalk_queue_turn collects a queue, adapts the scale, predicts the live set and
 * launches the next queue from the host -- the GPU idles meanwhile (~100 us of a 1 ms cycle at C2).  Here the live set lives on the
 * device: one workgroup merges the finished queue's proposals into it (the nlive largest of live points and proposals: what consuming
 * them in order leaves, thresholds only rise), adapts the scale by dynesty's rule, takes the new threshold and draws every chain's
 * start point, and the next queue is ENQUEUED before the current one has finished.  The host consumes each queue (payne_ns_consume) for
 * the evidence in its own time; its live SET is the device's, its slot order is not (start points differ from the host-turn loop's:
 * the same sampler statistically, not to the bit).  dynesty has no counterpart (one proposal at a time).
 *   _init    uploads the live set and the scale / threshold to start from (no queue may be in flight);
 *   _launch  enqueues [new bound, if one is given] + turn (merge = 0: start from the uploaded set as it is) + walks + 1 steps + the
 *            results' transfer; at most two queues in flight; axes_unit = NULL keeps the bound already on the device;
 *   _collect waits for the OLDEST queue in flight and returns it as payne_ns_rwalk_queue_end does, with the scale and threshold
 *            it ran under in dyn_used[2]. */
int payne_ns_queue_dev_init(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl, int nlive,
                            double scale, double loglstar);
int payne_ns_queue_dev_launch(payne_sampler* s, int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv,
                              int walks, unsigned long long seed, int merge, void* stream);
int payne_ns_queue_dev_collect(payne_sampler* s, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats,
                               double* dyn_used);

/* Kernel family names (for profiler filters): 0 dense layer, 1 post, 2 sed. */
const char* payne_kernel_name(int which);

/* The kernel (with its template arguments) the context's last batch call launched for one kind -- 0 output dense layer,
 * 1 post kernel, 2 sed kernel, 3 hidden dense layers (the last launch of that kind in the call) --, "" if none yet: which
 * code path a net of a given depth / a spectrum of a given length takes.  kind 4: "frequency" when the output layer handed the
 * post kernel rows already transformed (its weights restated once at payne_ctx_create: 1k/2k/4k/8k spectra on a geometric grid,
 * no continuum network, not PAYNE_V_ROWS_PIXEL), "pixels" otherwise.  Test and measurement aid, no reference counterpart. */
const char* payne_last_kernel(const payne_ctx* ctx, int kind);

/* out[i] = the activation `act` (PAYNE_ACT_*) of z[i], computed by the function the dense layers' epilogues call (device pointers,
 * n values, enqueued on `stream`).  Test aid, no reference counterpart: the sigmoid of NNmodels.py:92-121 is not the library's
 * expf + quotient here (dense_kernels.hpp sigmoid_f32), and its accuracy over the whole fp32 range is checked through this. */
int payne_activation_batch(const float* z, int n, int act, float* out, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream around every kernel
 * the batch calls enqueue (measurement aid for bench.py; no reference counterpart).
 * payne_profile(ctx, 1) clears the totals and starts recording, (ctx, 0) stops.
 * payne_profile_read waits for the recorded events and returns the accumulated
 * device time and launch count of one kind:
 *   0 output dense layer | 1 post kernel | 2 sed kernel | 3 hidden dense layers. */
int payne_profile(payne_ctx* ctx, int enable);
int payne_profile_read(payne_ctx* ctx, int kind, double* total_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* PAYNE_HIP_H */
