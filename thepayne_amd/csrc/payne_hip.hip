// payne_hip.hip -- the C ABI of include/payne_hip.h: contexts, launches, entry points.  One translation
// unit; the device code is included from dense_kernels.hpp (ANN layers), post_kernels.hpp + post_core.hpp +
// post_seq.hpp (spectrum pipeline), sed_kernel.hpp (photometry), the host-only part from host_tables.hpp
// (theta-independent tables).  The sampler's entry points are sampler_api.hip; what they ask of a context is ctx_api.hpp.
//
// Kernels (all hand-written for CDNA4, wave64):
//   payne_dense_kernel  fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32 fma chain) dense layer
//                       Y = act(X W^T + b) over the batch of candidates; LDS-tiled 64xBNx32,
//                       register-prefetch double buffering, XCD-aware tile order.  With FUSE_L0
//                       the A operand is produced on the fly from theta: label encoding
//                       (ystpred.py:47-50) + first layer + activation, so a YST1 forward pass
//                       (ystpred.py:52-58) is two launches.
//   payne_post_kernel   one 256-thread workgroup per candidate; the spectrum lives in LDS from
//                       the ANN output to chi^2: vsini FFT stage, Doppler, masked pow-2
//                       resample, Gaussian FFT stage, interpolation to the observed grid,
//                       blaze, chi^2 (phases in post_core.hpp, order in post_seq.hpp).
//   payne_sed_kernel    one wave per (candidate, filter): the stacked photometric nets of
//                       photANN.fastANN + highAv + the magnitude formulae of predictsed.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/payne_hip.h"
#include "host_tables.hpp"
#include "post_seq.hpp"
#include "ctx_api.hpp"

using namespace payne;

#include "dense_kernels.hpp"

#include "post_kernels.hpp"

#include "sed_kernel.hpp"
#include "select.hpp"

// photometry-only fits: lnL = -0.5 chi2_sed
__global__ void payne_photonly_kernel(const double* mags, const double* obs, const double* err, int F, int B, double* lnl) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) lnl[b] = -0.5 * sed_chi2(mags + (size_t)b * F, obs, err, F);
}

// ============================================================================
// context
// ============================================================================
static std::string g_create_error;

struct payne_ctx {
  int device = 0;
  payne_opts opts{};
  std::string err;
  std::vector<void*> owned;       // freed at destroy
  std::vector<void*> obs_owned;   // freed when the observed grid is re-bound
  // spectral model
  bool has_model = false;
  int n_layers = 0;
  payne_layer layers[PAYNE_MAX_LAYERS];
  int n_labels = 0;
  double xmin[PAYNE_MAX_LABELS], xden[PAYNE_MAX_LABELS];
  HostTables H;
  PostTables T{};
  float* hid[2] = {nullptr, nullptr};
  int ld_hid = 0;
  float* raw = nullptr;
  // The output layer's operand set: one for pixel rows, one for the same layer restated for rows in the frequency domain
  // (host_tables.hpp freq_rows: what the likelihood and the predictions past stage 0 run when the post kernel can start from the
  // transform, freq_ok).  pad: fp32 [rows][w_out_kp], k zero-padded to a multiple of 32 (the LDS-DMA kernels; payne_dense_dma3f_kernel
  // splits it on the way into LDS); p3: three bf16 planes [3][rows][w_out_kp]; h2: two fp16 planes [2][rows][w_out_kp] with row n
  // scaled by 2^e[n], rscale[n] = 2^-e[n] / act_scale; bias with bias_shift subtracted (the pixel rows are kept shifted by -1).
  struct OutOperands { const float* pad = nullptr; unsigned short* p3 = nullptr; unsigned short* h2 = nullptr; const float* rscale = nullptr;
                       const float* bias = nullptr; float bias_shift = 0.f; int rows = 0; };
  OutOperands out_pix, out_frq;
  bool freq_ok = false;
  int w_out_kp = 0;
  const float* w_hid_pad[PAYNE_MAX_LAYERS] = {};   // hidden layers: [N][ld_hid] copies, zero beyond K (hk_tile's LDS-DMA staging)
  bool dma_ok = false;                  // hidden buffers are zero beyond the last hidden width
  // the last hidden layer's output as the output layer's operand planes [3][b_max][ld_hid] (written by the hidden-layer kernel's
  // epilogue; zero beyond the hidden width); act_scale: the power of two it is written with as fp16 pairs (calibrated on the label
  // box; 0 = not available)
  unsigned short* hid_p3 = nullptr;
  float act_scale = 0.f;
  // Hidden layer l = 1 .. n - 2 on fp16 pairs (hk_tile_h2, hk_tile_h2x): its weights as two fp16 planes [2][n_out][304], rows scaled;
  // rs = 2^-e / in_scale; in_scale: the power of two its input activations are written with.  Layer 1 alone has them for a net with
  // two hidden layers; hid_pairs_deep: every hidden layer has, and hid_h2 (the activations between two such layers as planes
  // [2][b_max][304], two buffers taking turns) and chain_flags exist.
  struct HidPairs { unsigned short* planes = nullptr; const float* rs = nullptr; float in_scale = 0.f; };
  HidPairs hid_pairs[PAYNE_MAX_LAYERS];
  bool hid_pairs_deep = false;
  unsigned short* hid_h2[2] = {nullptr, nullptr};
  // payne_dense_chain_kernel: the row blocks' hop counters [ceil(b_max / 32)][kChainMax] (never reset) and the calls made so far
  unsigned long long* chain_flags = nullptr; unsigned long long chain_calls = 0;
  // freq_rs: the restated layer is that of the RESAMPLED spectrum (model grids that are not a power of two long: n1 rows of n1
  // values); a batch with a candidate that does not rotate falls back to pixels ON THE DEVICE (rot_flag: a word the records'
  // writers set to rot_seq, read by the output layer and the post kernel of the same batch; rot_seq: the last number issued)
  bool freq_rs = false; unsigned long long* rot_flag = nullptr; unsigned long long rot_seq = 0;
  size_t post_lds = 0;
  void (*post_fn_lean)(PAYNE_POST_SIG) = nullptr;   // likelihood-only instantiation (same LDS)
  bool post_tw_lds = false;
  int n_cu = 256;                       // compute units of the device (MI355X: 256)
  bool lean_available = false;          // a likelihood-only instantiation exists for this spectrum length (it can carry a walk's tail)
  PostTables* d_T = nullptr;          // device copy of T
  post_kernel_fn post_fn = nullptr;
  float* big_ws = nullptr;            // global spectrum buffers of payne_post_big_kernel (n1 > 16384)
  int big_grid = 0;
  bool big_tiled = false;             // ... with the four-step transform (LDS tile attribute set at create)
  bool big_chip = false;              // ... or with the convolution stages on the compute unit (65 536 points: payne_post_chip_kernel)
  bool big_chip2 = false;             // ... 32 768 points, two candidates at a time (payne_post_chip2_kernel)
  // optional continuum network (payne_ctx_set_continuum; ystpred.py:81-85, 191-209)
  bool has_cont = false;
  int cn_layers = 0, cn_npix = 0, cn_ld_hid = 0;
  payne_layer clayers[PAYNE_MAX_LAYERS];
  double cxmin[PAYNE_MAX_LABELS], cxden[PAYNE_MAX_LABELS];
  float* chid[2] = {nullptr, nullptr};
  float* cont_raw = nullptr;            // [b_max][cn_npix] continuum ANN output (F_nu)
  const double* cont_scale = nullptr;   // [cn_npix] (lam_ref / lam_c)^2 : F_nu -> F_lambda up to a constant the median removes
  const int* cont_idx = nullptr;        // [npix] np.interp(modwave, modcontwave, .) map: left pixel (-1: outside -> NaN)
  const double* cont_frac = nullptr;    // [npix] weight of the right pixel
  std::vector<void*> cont_owned;
  // optional LSF vector (payne_ctx_set_lsf): dispersion in AA per bound observed pixel; replaces Inst_R
  bool has_lsf = false;
  const double* d_obs_wave = nullptr;   // [nobs] (obs_owned)
  const double* lsf = nullptr;          // [n_lsf] dispersions ...
  const double* lsf_wave = nullptr;     // ... at these wavelengths (the observed grid itself for payne_ctx_set_lsf)
  int n_lsf = 0;
  float* lsf_spec = nullptr;            // [lsf_chunk][npix] spectra after vsini, shifted
  double* lsf_ws = nullptr;             // [lsf_chunk][2 npix + n1]
  float* lsf_fws = nullptr;             // global form: [lsf_chunk][2 fft_buf_floats(n1)] FFT buffers
  bool lsf_global = false;              // spectra too long for LDS (n1 > 8192): buffers in global memory, median by selection
  int lsf_chunk = 0;                    // candidates per launch (the global form walks the batch in chunks: bounded workspace)
  std::vector<void*> lsf_owned;
  bool obs_bound = false;
  CandState* prep = nullptr;      // [b_max] per-candidate records of the post kernel (written by the first dense launch)
  // photometry
  bool has_phot = false, has_obs_phot = false;
  PhotTables P{};
  double* mags_ws = nullptr;
  double *obs_mag = nullptr, *obs_err = nullptr;
  int ncols = 0;
  // optional per-kernel HIP-event timing (payne_profile): kinds 0 output dense layer,
  // 1 post, 2 sed, 3 hidden dense layers
  bool prof = false;
  struct ProfRec { hipEvent_t e0, e1; int kind; };
  std::vector<ProfRec> prof_pool;
  size_t prof_used = 0;
  double prof_ms[4] = {0, 0, 0, 0};
  long long prof_n[4] = {0, 0, 0, 0};
  const char* last_kernel[4] = {"", "", "", ""};   // what the last call launched, per kind (payne_last_kernel)
  bool last_rows_freq = false;                     // ... and whether its post kernel was handed rows in the frequency domain (kind 4)
};

// RAII bracket of one timed launch.  The event pair is handed to the launch itself (hipExtLaunchKernelGGL:
// start/stop are the kernel's own dispatch timestamps -- what rocprofv3 reports); events recorded AROUND a
// launch on the stream read ~2 us more (their own packets).  A scope that sees no PAYNE_LAUNCH gives its
// record back; a scope with several launches times the first.
struct ProfScope;
static thread_local ProfScope* g_prof_scope = nullptr;
struct ProfScope {
  payne_ctx* c; hipStream_t s; payne_ctx::ProfRec* r = nullptr; bool used = false; ProfScope* outer = nullptr; int kind;
  ProfScope(payne_ctx* c_, hipStream_t s_, int kind_) : c(c_), s(s_), kind(kind_) {
    outer = g_prof_scope; g_prof_scope = this;
    if (!c->prof) return;
    if (c->prof_used == c->prof_pool.size()) {
      payne_ctx::ProfRec n{};
      if (hipEventCreate(&n.e0) != hipSuccess || hipEventCreate(&n.e1) != hipSuccess) return;
      c->prof_pool.push_back(n);
    }
    r = &c->prof_pool[c->prof_used++];
    r->kind = kind;
  }
  ~ProfScope() {
    g_prof_scope = outer;
    if (r && !used) --c->prof_used;                      // nothing was launched under this scope
  }
};
#include <hip/hip_ext.h>
#define PAYNE_LAUNCH(kernel, grid, block, lds, stream, ...) PAYNE_LAUNCH_AS(#kernel, kernel, grid, block, lds, stream, __VA_ARGS__)
// (a dense kernel: its dynamic LDS is the one the list in dense_kernels.hpp gives it)
#define PAYNE_LAUNCH_DENSE(kernel, grid, block, stream, ...) PAYNE_LAUNCH_AS(#kernel, kernel, grid, block, DenseLds<kernel>::value, stream, __VA_ARGS__)
#define PAYNE_LAUNCH_AS(name, kernel, grid, block, lds, stream, ...)                                      \
  do {                                                                                                    \
    ProfScope* ps_ = g_prof_scope;                                                                        \
    if (ps_) ps_->c->last_kernel[ps_->kind] = name;                                                       \
    if (ps_ && ps_->r && !ps_->used) {                                                                    \
      ps_->used = true;                                                                                   \
      hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)(lds), stream, ps_->r->e0, ps_->r->e1, 0, __VA_ARGS__); \
    } else {                                                                                              \
      hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                  \
    }                                                                                                     \
  } while (0)

#define HIPCHK(ctx, call)                                                                 \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
      return PAYNE_E_HIP;                                                                 \
    }                                                                                     \
  } while (0)

template <class V>
static int upload(payne_ctx* c, const std::vector<V>& v, const V** out, std::vector<void*>& bag) {
  void* d = nullptr;
  size_t bytes = v.size() * sizeof(V);
  if (bytes == 0) { *out = nullptr; return PAYNE_OK; }
  HIPCHK(c, hipMalloc(&d, bytes));
  bag.push_back(d);
  HIPCHK(c, hipMemcpy(d, v.data(), bytes, hipMemcpyHostToDevice));
  *out = reinterpret_cast<const V*>(d);
  return PAYNE_OK;
}
template <class V>
static int dev_alloc(payne_ctx* c, size_t n, V** out, std::vector<void*>& bag, bool zero = true) {
  void* d = nullptr;
  HIPCHK(c, hipMalloc(&d, n * sizeof(V)));
  bag.push_back(d);
  if (zero) HIPCHK(c, hipMemset(d, 0, n * sizeof(V)));
  *out = reinterpret_cast<V*>(d);
  return PAYNE_OK;
}

void payne::set_create_error(const std::string& msg) { g_create_error = msg; }
static int fail(payne_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg; else set_create_error(msg);
  return code;
}

// the calls of an entry point go to the context's device (a failing hipSetDevice: the device has already failed)
static int on_device(payne_ctx* c) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != c->device) {
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  return PAYNE_OK;
}

// ctx_api.hpp: the same two and the three numbers a sampler reads, for the library's other units (ctx_lnlike: further down)
int payne::ctx_fail(payne_ctx* c, int code, const std::string& msg) { return fail(c, code, msg); }
int payne::ctx_on_device(payne_ctx* c) { return on_device(c); }
CtxView payne::ctx_view(const payne_ctx* c) { return CtxView{c->device, c->ncols, c->opts.b_max}; }

// A context being reconfigured: on its own device, with nothing in flight (no kernel may still read what is about to be freed or
// re-bound); the caller's device again on the way out.
struct DeviceScope {
  int prev = 0, dev;
  explicit DeviceScope(const payne_ctx* c) : dev(c->device) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); (void)hipDeviceSynchronize(); }
  ~DeviceScope() { if (prev != dev) (void)hipSetDevice(prev); }
};

// A network's layers into the context's own list `dst`: shapes checked (`who`: what the messages call the network), weights whose K
// is no multiple of 4 replaced by a zero-padded copy in `bag` (float4 tile loads).  *maxh: the widest hidden layer.
static int adopt_layers(payne_ctx* c, const payne_model_desc* m, payne_layer* dst, std::vector<void*>& bag, const std::string& who, int* maxh) {
  *maxh = 0;
  for (int l = 0; l < m->n_layers; ++l) {
    const payne_layer& L = m->layers[l];
    if (!L.w || !L.b || L.n_in <= 0 || L.n_out <= 0) return fail(c, PAYNE_E_INVALID, who + "layer with null weights or bad shape");
    if (l > 0 && L.n_in != m->layers[l - 1].n_out) return fail(c, PAYNE_E_INVALID, who + "layer shapes do not chain");
    dst[l] = L;
    if (l > 0 && (L.n_in & 3)) {
      const int Kp = (L.n_in + 3) & ~3;
      float* wp = nullptr;
      if (int rc = dev_alloc(c, (size_t)L.n_out * Kp, &wp, bag)) return rc;
      const hipError_t he = hipMemcpy2D(wp, (size_t)Kp * 4, L.w, (size_t)L.n_in * 4, (size_t)L.n_in * 4, L.n_out, hipMemcpyDeviceToDevice);
      if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy2D: ") + hipGetErrorString(he));
      dst[l].w = wp;
      dst[l].n_in = Kp;             // padded K (extra columns are zero)
    }
    if (l + 1 < m->n_layers) *maxh = std::max(*maxh, L.n_out);
  }
  return PAYNE_OK;
}

static int sync_tables(payne_ctx* c) {
  if (!c->d_T) return PAYNE_OK;
  HIPCHK(c, hipMemcpy(c->d_T, &c->T, sizeof(PostTables), hipMemcpyHostToDevice));
  return PAYNE_OK;
}

static int bind_obs(payne_ctx* c, const payne_obs_desc* obs) {
  for (void* p : c->obs_owned) (void)hipFree(p);
  c->obs_owned.clear();
  c->obs_bound = false;
  for (void* p : c->lsf_owned) (void)hipFree(p);      // an LSF vector belongs to the grid it was given on
  c->lsf_owned.clear(); c->has_lsf = false; c->d_obs_wave = nullptr;
  c->T.obs_sorted = 0;
  c->T.nobs = 0; c->T.lnobs = nullptr; c->T.obs_rec = nullptr; c->T.xcheb = nullptr; c->T.obs_f1 = nullptr; c->T.obs_ivar = nullptr;
  if (!obs || obs->nobs <= 0) return sync_tables(c);
  if (!obs->wave) return fail(c, PAYNE_E_INVALID, "obs.wave is NULL");
  if ((obs->flux == nullptr) != (obs->eflux == nullptr)) return fail(c, PAYNE_E_INVALID, "obs.flux and obs.eflux must both be given or both NULL");
  build_obs_tables(obs->wave, obs->flux, obs->eflux, obs->nobs, c->H);
  int rc;
  if ((rc = upload(c, c->H.lnobs, &c->T.lnobs, c->obs_owned))) return rc;
  if ((rc = upload(c, c->H.obs_rec, &c->T.obs_rec, c->obs_owned))) return rc;
  if ((rc = upload(c, c->H.obs_wave, &c->d_obs_wave, c->obs_owned))) return rc;
  if ((rc = upload(c, c->H.xcheb, &c->T.xcheb, c->obs_owned))) return rc;
  if (c->H.has_flux) {
    if ((rc = upload(c, c->H.obs_f1, &c->T.obs_f1, c->obs_owned))) return rc;
    if ((rc = upload(c, c->H.obs_ivar, &c->T.obs_ivar, c->obs_owned))) return rc;
  }
  c->T.nobs = obs->nobs;
  c->T.obs_min = c->H.obs_min;
  c->T.obs_max = c->H.obs_max;
  c->T.ln_obs_min = std::log(c->H.obs_min); c->T.ln_obs_max = std::log(c->H.obs_max);
  c->T.obs_sorted = 1;
  for (int i = 1; i < obs->nobs; ++i) if (!(obs->wave[i] >= obs->wave[i - 1])) { c->T.obs_sorted = 0; break; }
  c->obs_bound = true;
  return sync_tables(c);
}

extern "C" int payne_version(void) { return PAYNE_ABI_VERSION; }

extern "C" const char* payne_last_error(const payne_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

extern "C" int payne_theta_cols(const payne_ctx* ctx) { return ctx ? ctx->ncols : PAYNE_E_INVALID; }

extern "C" const char* payne_kernel_name(int which) {
  switch (which) {
    case 0: return "payne_dense_kernel";
    case 1: return "payne_post_kernel";
    case 2: return "payne_sed_kernel";
    default: return "";
  }
}

__global__ void payne_activation_kernel(const float* __restrict__ z, int n, int act, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = act_apply(z[i], act);
}
extern "C" int payne_activation_batch(const float* z, int n, int act, float* out, void* stream) {
  if (!z || !out || n < 0 || act < PAYNE_ACT_NONE || act > PAYNE_ACT_SIGMOID) return PAYNE_E_INVALID;
  if (n == 0) return PAYNE_OK;
  hipLaunchKernelGGL(payne_activation_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z, n, act, out);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}
extern "C" const char* payne_last_kernel(const payne_ctx* c, int kind) {
  if (c && kind == 4) return c->last_rows_freq ? "frequency" : "pixels";        // what the output layer handed to the post kernel
  return (c && kind >= 0 && kind < 4) ? c->last_kernel[kind] : "";
}

extern "C" void payne_ctx_destroy(payne_ctx* c) {
  if (!c) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(c->device);
  for (void* p : c->owned) (void)hipFree(p);
  for (void* p : c->obs_owned) (void)hipFree(p);
  for (void* p : c->cont_owned) (void)hipFree(p);
  for (void* p : c->lsf_owned) (void)hipFree(p);
  for (auto& r : c->prof_pool) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  (void)hipSetDevice(prev);
  delete c;
}

static hipError_t set_dense_attributes();
// ---- two fp16 planes an operand (dense_kernels.hpp split2h) -----------------------------------------------------------
// The largest |activation| of the last hidden layer over the label box (corners, centre, 64 points of a fixed sequence, 20 % beyond
// the box on every side), evaluated on the host in fp64 from the layers as the context holds them.  0 when the net has no hidden
// layer or produces something that is not finite.
static double hidden_amax(const payne_model_desc* m, std::string& why, double* per_layer = nullptr) {      // (per_layer[l]: the same for layer l's output, l < n_layers - 1)
  const int nl = m->n_layers, D = m->n_labels;
  if (nl < 3) { why = "no hidden layer pair"; return 0.0; }
  std::vector<std::vector<float>> W(nl - 1), b(nl - 1);
  for (int l = 0; l + 1 < nl; ++l) {
    const payne_layer& L = m->layers[l];
    W[l].resize((size_t)L.n_out * L.n_in); b[l].resize((size_t)L.n_out);
    if (hipMemcpy(W[l].data(), L.w, W[l].size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(b[l].data(), L.b, b[l].size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { why = "hipMemcpy"; return 0.0; }
  }
  auto act = [](double z, int a) { return a == PAYNE_ACT_LRELU ? (z > 0 ? z : 0.01 * z) : (a == PAYNE_ACT_SIGMOID ? 1.0 / (1.0 + std::exp(-z)) : z); };
  std::vector<std::vector<double>> pts;
  for (int cidx = 0; cidx < (1 << D); ++cidx) { std::vector<double> x(D); for (int d = 0; d < D; ++d) x[d] = ((cidx >> d) & 1) ? 0.6 : -0.6; pts.push_back(x); }
  pts.push_back(std::vector<double>(D, 0.0));
  unsigned long long st = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 64; ++i) {
    std::vector<double> x(D);
    for (int d = 0; d < D; ++d) { st = st * 6364136223846793005ull + 1442695040888963407ull; x[d] = ((double)(st >> 11) / 9007199254740992.0 - 0.5) * 1.2; }
    pts.push_back(x);
  }
  double amax = 0.0;
  std::vector<double> a, y;
  for (const auto& x : pts) {
    a = x;
    for (int l = 0; l + 1 < nl; ++l) {
      const payne_layer& L = m->layers[l];
      y.assign((size_t)L.n_out, 0.0);
      for (int o = 0; o < L.n_out; ++o) {
        double z = b[l][o];
        const float* w = &W[l][(size_t)o * L.n_in];
        for (int k = 0; k < L.n_in; ++k) z += (double)w[k] * a[k];
        y[o] = act(z, L.act);
      }
      a.swap(y);
      if (per_layer) for (double v : a) { if (std::isfinite(v)) per_layer[l] = std::max(per_layer[l], std::fabs(v)); else per_layer[l] = 1e300; }
    }
    for (double v : a) { if (!std::isfinite(v)) { why = "non-finite activation"; return 0.0; } amax = std::max(amax, std::fabs(v)); }
  }
  return amax;
}
// per-row power-of-two scales of a padded weight matrix [n][kp] (host copy) and its two fp16 planes on the device
static int make_h2_planes(payne_ctx* c, const float* d_w, const std::vector<float>& h_w, int n, int kp, float act_scale,
                          unsigned short** planes, const float** rscale) {
  std::vector<float> sc((size_t)n), rs((size_t)n);
  for (int i = 0; i < n; ++i) {
    float mx = 0.f;
    for (int k = 0; k < kp; ++k) mx = std::max(mx, std::fabs(h_w[(size_t)i * kp + k]));
    int e = 0;
    if (mx > 0.f && std::isfinite(mx)) e = (int)std::floor(std::log2(16384.0 / (double)mx));
    e = std::max(-100, std::min(100, e));
    sc[i] = (float)std::ldexp(1.0, e);
    rs[i] = (float)(std::ldexp(1.0, -e) / (double)act_scale);
  }
  const float* d_sc = nullptr;
  std::vector<void*> tmp;
  int rc = upload(c, sc, &d_sc, tmp);
  if (!rc) rc = upload(c, rs, rscale, c->owned);
  const size_t nw = (size_t)n * kp;
  if (!rc) rc = dev_alloc(c, 2 * nw, planes, c->owned);
  hipError_t he = hipSuccess;
  if (!rc) {
    hipLaunchKernelGGL(payne_split2h_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, nullptr, d_w, n, kp, d_sc, *planes, nw);
    he = hipDeviceSynchronize();
  }
  for (void* q : tmp) (void)hipFree(q);
  if (rc) return rc;
  if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("weight split (fp16 planes): ") + hipGetErrorString(he));
  return PAYNE_OK;
}

// The power of two a layer's activations are written with as fp16 pairs: their largest magnitude on the label box lands in
// [2048, 4096] (a factor of 8 to spare below fp16's range); 0 where the calibration found nothing usable.
static float h2_act_scale(double amax) {
  if (!(amax > 0.0 && amax < 1e30)) return 0.f;
  return (float)std::ldexp(1.0, std::max(-60, std::min(60, (int)std::floor(std::log2(4096.0 / amax)))));
}
// A layer's weights (device, [n][k]) as fp16-pair planes [n][kp], rows zero-padded to kp columns, for activations written at `scale`.
static int layer_h2_planes(payne_ctx* c, const float* d_w, int n, int k, int kp, float scale, const char* what,
                           unsigned short** planes, const float** rscale) {
  std::vector<float> h((size_t)n * k);
  const hipError_t he = hipMemcpy(h.data(), d_w, h.size() * 4, hipMemcpyDeviceToHost);
  if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy(") + what + "): " + hipGetErrorString(he));
  if (k == kp) return make_h2_planes(c, d_w, h, n, kp, scale, planes, rscale);          // (padded on the device already)
  std::vector<float> hp((size_t)n * kp, 0.f);
  for (int i = 0; i < n; ++i) std::copy(h.begin() + (size_t)i * k, h.begin() + (size_t)(i + 1) * k, hp.begin() + (size_t)i * kp);
  const float* d_hp = nullptr;
  std::vector<void*> tmp;
  int rc = upload(c, hp, &d_hp, tmp);
  if (!rc) rc = make_h2_planes(c, d_hp, hp, n, kp, scale, planes, rscale);
  for (void* q : tmp) (void)hipFree(q);
  return rc;
}

// An output layer's operand planes from its padded fp32 weights o.pad [o.rows][w_out_kp]: the three bf16 planes (OutForm::Bf16x3) unless
// they exist, and with h2_scale > 0 the two fp16 planes and rscale (OutForm::H2) for activations written at that scale.  h_w: the
// weights' host copy (null: fetched).  Both sets come here twice: what is allocated between the two calls keeps its place.
static int build_out_planes(payne_ctx* c, payne_ctx::OutOperands& o, const std::vector<float>* h_w, float h2_scale) {
  const int kp = c->w_out_kp;
  const size_t nw = (size_t)o.rows * kp;
  if (!o.p3) {
    if (int rc = dev_alloc(c, 3 * nw, &o.p3, c->owned)) return rc;
    hipLaunchKernelGGL(payne_split3_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, nullptr, o.pad, nw, o.p3, nw);
    const hipError_t he = hipDeviceSynchronize();
    if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("weight split: ") + hipGetErrorString(he));
  }
  if (!(h2_scale > 0.f)) return PAYNE_OK;
  if (h_w) return make_h2_planes(c, o.pad, *h_w, o.rows, kp, h2_scale, &o.h2, &o.rscale);
  return layer_h2_planes(c, o.pad, o.rows, kp, kp, h2_scale, "output layer", &o.h2, &o.rscale);
}

// payne_ctx_create, step by step: each returns a PAYNE_E_* code with c->err set.
// The dense kernels' operand copies of the spectral net (c->layers is filled in; maxh: the widest hidden layer).
static int create_dense_operands(payne_ctx* c, const payne_model_desc* model, const payne_opts* opts, int maxh) {
  int rc = PAYNE_OK;
  hipError_t he = hipSuccess;
  // k-padded copy of the output layer's weights for the LDS-DMA kernel (operands cannot be masked on the way)
  const payne_layer& L = c->layers[model->n_layers - 1];
  const int Kp = (L.n_in + 31) & ~31;
  float* wp = nullptr;
  if ((rc = dev_alloc(c, (size_t)L.n_out * Kp, &wp, c->owned))) return rc;
  he = hipMemcpy2D(wp, (size_t)Kp * 4, L.w, (size_t)L.n_in * 4, (size_t)L.n_in * 4, L.n_out, hipMemcpyDeviceToDevice);
  if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy2D: ") + hipGetErrorString(he));
  c->w_out_kp = Kp;
  c->out_pix.pad = wp; c->out_pix.bias = L.b; c->out_pix.bias_shift = kBase; c->out_pix.rows = L.n_out;
  // the activations' pad columns are zero only if no wider layer ever wrote them: all hidden widths equal
  bool same = model->n_layers >= 3;
  for (int l = 1; l + 1 < model->n_layers; ++l) same = same && model->layers[l].n_out == model->layers[0].n_out;
  c->dma_ok = same;
  if (!same) return PAYNE_OK;
  // hidden layers past the second (launch_hidden<false>): operand tiles straight into LDS need rows >= HK_PITCH floats apart that
  // may be read to their end -- the activations' buffers are (pitch ld_hid, pad columns zero while all widths are equal); the
  // weights get a copy with the same pitch
  const int ldh = (maxh + 31) & ~31;
  if (ldh >= HK_PITCH) {
    for (int l = 1; l + 1 < model->n_layers; ++l) {
      const payne_layer& Lh = c->layers[l];
      if (Lh.n_in > HK_KC) continue;
      float* wh = nullptr;
      if ((rc = dev_alloc(c, (size_t)Lh.n_out * ldh, &wh, c->owned))) return rc;
      he = hipMemcpy2D(wh, (size_t)ldh * 4, Lh.w, (size_t)Lh.n_in * 4, (size_t)Lh.n_in * 4, Lh.n_out, hipMemcpyDeviceToDevice);
      if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy2D: ") + hipGetErrorString(he));
      c->w_hid_pad[l] = wh;
    }
  }
  // the output layer's weights as three bf16 planes (OutForm::Bf16x3) ...
  if ((rc = build_out_planes(c, c->out_pix, nullptr, 0.f))) return rc;
  // ... and as two fp16 planes (OutForm::H2), the activations' scale calibrated on the label box.  The hidden layers' fp16 planes
  // need the same calibration: it is made unless neither form is asked for.
  const bool out_h2 = wanted_out_form(opts->variant) == OutForm::H2, hid_h2 = !(opts->variant & PAYNE_V_HID_F32);
  std::string why;
  double amaxl[PAYNE_MAX_LAYERS] = {};
  const double amax = (out_h2 || hid_h2) ? hidden_amax(model, why, amaxl) : 0.0;
  // the second layer's weights for hk_tile_h2: widths whose padded K is the tile's 304 columns
  const payne_layer& L1 = model->layers[1];
  if (h2_act_scale(amaxl[0]) > 0.f && L1.n_in > 288 && L1.n_in <= 304 && c->w_hid_pad[1] && hid_h2) {
    payne_ctx::HidPairs* hp = c->hid_pairs;
    hp[1].in_scale = h2_act_scale(amaxl[0]);
    if ((rc = layer_h2_planes(c, L1.w, L1.n_out, L1.n_in, 304, hp[1].in_scale, "second layer", &hp[1].planes, &hp[1].rs))) return rc;
    // deeper nets (LinNet: five hidden layers): the layers past the second the same way, their activations handed on as planes
    bool deep = model->n_layers > 3;
    for (int l = 1; l + 1 < model->n_layers; ++l) deep = deep && h2_act_scale(amaxl[l]) > 0.f && model->layers[l].n_out == L1.n_out;
    if (deep) {
      for (int l = 2; l + 1 < model->n_layers; ++l) {
        const payne_layer& Ll = model->layers[l];
        hp[l].in_scale = h2_act_scale(amaxl[l - 1]);
        if ((rc = layer_h2_planes(c, Ll.w, Ll.n_out, Ll.n_in, 304, hp[l].in_scale, "hidden layer", &hp[l].planes, &hp[l].rs))) return rc;
      }
      for (int q = 0; q < 2; ++q)
        if ((rc = dev_alloc(c, (size_t)2 * opts->b_max * 304, &c->hid_h2[q], c->owned))) return rc;
      if ((rc = dev_alloc(c, (size_t)((opts->b_max + 31) / 32) * kChainMax, &c->chain_flags, c->owned))) return rc;
      c->hid_pairs_deep = true;
    }
  }
  if (h2_act_scale(amax) > 0.f && out_h2) {
    c->act_scale = h2_act_scale(amax);
    if ((rc = build_out_planes(c, c->out_pix, nullptr, c->act_scale))) return rc;
  }
  return PAYNE_OK;
}
// The first convolution stage's forward transform is linear and the same for every candidate: with identity vsini maps and a
// compile-time geometry the output layer writes the rows already transformed (weights = the transform of each hidden unit's
// pixel vector, computed here once in fp64), and the post kernel starts at the taper.
static int create_freq_rows(payne_ctx* c, const payne_model_desc* model, const payne_opts* opts, int geom_n1) {
  int rc = PAYNE_OK;
  hipError_t he = hipSuccess;
  const PostTables& T = c->T;
  const bool fixed = geom_n1 != 0 && ((c->post_tw_lds && (T.n1 == 1024 || T.n1 == 2048 || T.n1 == 4096)) || (!c->post_tw_lds && T.n1 == 8192));
  // (65 536 / 32 768 points with the stages on the compute unit: the rows in the order those kernels' registers hold the transform)
  // (a model grid of any other length -- what a trained network has: readc3k.py:441-447 -- is resampled by the rotation stage first,
  //  a static linear map as well: the LDS kernels' lengths take rows of the RESAMPLED spectrum's transform, freq_rs)
  const bool ident = T.rot_identity && T.n1 == model->npix;
  if (((fixed || c->big_chip || c->big_chip2) && ident || (fixed && !ident)) && c->out_pix.p3 && c->hid_p3 && !(opts->variant & PAYNE_V_ROWS_PIXEL)) {
    const payne_layer& L = model->layers[model->n_layers - 1];
    const int K = L.n_in, Kp = c->w_out_kp, n = ident ? L.n_out : T.n1;
    std::vector<float> W((size_t)L.n_out * K), b((size_t)L.n_out), Wz, bz;
    he = hipMemcpy(W.data(), L.w, W.size() * 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(b.data(), L.b, b.size() * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy(output layer): ") + hipGetErrorString(he));
    if (ident) freq_rows(W.data(), b.data(), -(double)kBase, n, K, Wz, bz, c->big_chip ? 1 : (c->big_chip2 ? 2 : 0));   // (rows are kept shifted by -1, as the pixel rows are)
    else {
      freq_rows(W.data(), b.data(), -(double)kBase, n, K, Wz, bz, 0, c->H.rs1_idx.data(), c->H.rs1_frac.data(), L.n_out);
      c->freq_rs = true;
      if ((rc = dev_alloc(c, (size_t)1, &c->rot_flag, c->owned))) return rc;            // (zeroed; sequence numbers start at 1)
    }
    std::vector<float> Wp((size_t)n * Kp, 0.f);
    for (int i = 0; i < n; ++i) std::copy(Wz.begin() + (size_t)i * K, Wz.begin() + (size_t)(i + 1) * K, Wp.begin() + (size_t)i * Kp);
    payne_ctx::OutOperands& o = c->out_frq;
    o.rows = n; o.bias_shift = 0.f;                             // (the shift is in the restated bias)
    if ((rc = upload(c, Wp, &o.pad, c->owned))) return rc;      // (kept: the fp32 form is what the one-tile-per-CU kernel reads)
    if ((rc = build_out_planes(c, o, &Wp, 0.f))) return rc;
    if ((rc = upload(c, bz, &o.bias, c->owned))) return rc;
    if (c->out_pix.h2 && (rc = build_out_planes(c, o, &Wp, c->act_scale))) return rc;
    c->freq_ok = true;
  }
  return PAYNE_OK;
}
// The photometric nets.
static int create_phot(payne_ctx* c, const payne_phot_desc* phot, const payne_opts* opts) {
  int rc = PAYNE_OK;
  hipError_t he = hipSuccess;
  if (phot->n_filters <= 0 || phot->hidden <= 0 || phot->hidden > 2048) return fail(c, PAYNE_E_INVALID, "phot.n_filters/hidden out of range");
  if (!phot->w1 || !phot->b1 || !phot->w2 || !phot->b2 || !phot->w3 || !phot->b3 || !phot->xmin || !phot->xmax)
    return fail(c, PAYNE_E_INVALID, "phot descriptor has NULL members");
  PhotTables& P = c->P;
  const int F = phot->n_filters, H = phot->hidden;
  P.F = F; P.H = H;
  P.w1 = phot->w1; P.b1 = phot->b1; P.b2 = phot->b2; P.w3 = phot->w3; P.b3 = phot->b3;
  for (int d = 0; d < 6; ++d) { P.xmin[d] = phot->xmin[d]; P.xden[d] = phot->xmax[d] - phot->xmin[d]; }
  {   // w2 -> [F][k][h] so that lanes (h) read consecutive addresses
    std::vector<float> w2((size_t)F * H * H), w2t((size_t)F * H * H);
    he = hipMemcpy(w2.data(), phot->w2, w2.size() * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy(w2): ") + hipGetErrorString(he));
    sed_transpose_w2(F, H, H, w2.data(), w2t.data());
    if ((rc = upload(c, w2t, &P.w2t, c->owned))) return rc;
  }
  if (phot->hiav) {
    std::vector<double> hv(phot->hiav, phot->hiav + (size_t)F * 5);
    if ((rc = upload(c, hv, &P.hiav, c->owned))) return rc;
  }
  if (phot->obs_mag && phot->obs_err) {
    std::vector<double> m(phot->obs_mag, phot->obs_mag + F), e(phot->obs_err, phot->obs_err + F);
    const double *dm, *de;
    if ((rc = upload(c, m, &dm, c->owned))) return rc;
    if ((rc = upload(c, e, &de, c->owned))) return rc;
    c->obs_mag = const_cast<double*>(dm); c->obs_err = const_cast<double*>(de);
    c->has_obs_phot = true;
  }
  if ((rc = dev_alloc(c, (size_t)opts->b_max * F, &c->mags_ws, c->owned))) return rc;
  if ((size_t)H * 16 > 48 * 1024) {
    he = hipFuncSetAttribute(reinterpret_cast<const void*>(payne_sed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, H * 16);
    if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute(sed): ") + hipGetErrorString(he));
  }
  c->has_phot = true;
  return PAYNE_OK;
}

extern "C" int payne_ctx_create(const payne_model_desc* model, const payne_obs_desc* obs, const payne_phot_desc* phot,
                                const payne_opts* opts, int device, payne_ctx** out) {
  if (!out) return fail(nullptr, PAYNE_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!opts || opts->b_max <= 0) return fail(nullptr, PAYNE_E_INVALID, "opts.b_max must be > 0");
  if (opts->npoly < 0 || opts->npoly > PAYNE_MAX_POLY) return fail(nullptr, PAYNE_E_INVALID, "opts.npoly out of range");
  if (!model && !phot) return fail(nullptr, PAYNE_E_INVALID, "need a spectral model and/or a photometric model");
  hipError_t he = hipSetDevice(device);
  if (he != hipSuccess) return fail(nullptr, PAYNE_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
  payne_ctx* c = new payne_ctx();
  c->device = device;
  { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->n_cu = ncu; }
  c->opts = *opts;
  c->ncols = 8 + opts->npoly + 4;
  int rc = PAYNE_OK;
  auto bail = [&](int code) { g_create_error = c->err; payne_ctx_destroy(c); return code; };
  he = set_dense_attributes();
  if (he != hipSuccess) return bail(fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute(dense): ") + hipGetErrorString(he)));

  if (model) {
    if (model->n_layers < 2 || model->n_layers > PAYNE_MAX_LAYERS) return bail(fail(c, PAYNE_E_INVALID, "model.n_layers must be 2..8"));
    if (model->n_labels < 1 || model->n_labels > PAYNE_MAX_LABELS) return bail(fail(c, PAYNE_E_INVALID, "model.n_labels must be 1..5"));
    if (!model->xmin || !model->xmax || !model->wavelength) return bail(fail(c, PAYNE_E_INVALID, "model.xmin/xmax/wavelength missing"));
    if (model->layers[0].n_in != model->n_labels) return bail(fail(c, PAYNE_E_INVALID, "first layer n_in != n_labels"));
    if (model->layers[model->n_layers - 1].n_out != model->npix) return bail(fail(c, PAYNE_E_INVALID, "last layer n_out != npix"));
    int maxh = 0;
    if ((rc = adopt_layers(c, model, c->layers, c->owned, "", &maxh))) return bail(rc);
    if ((rc = create_dense_operands(c, model, opts, maxh))) return bail(rc);
    c->n_layers = model->n_layers;
    c->n_labels = model->n_labels;
    for (int d = 0; d < model->n_labels; ++d) { c->xmin[d] = model->xmin[d]; c->xden[d] = model->xmax[d] - model->xmin[d]; }
    rc = build_model_tables(model->wavelength, model->npix, c->H);
    if (rc == -1) return bail(fail(c, PAYNE_E_INVALID, "model.npix must be >= 16"));
    if (rc == -2) return bail(fail(c, PAYNE_E_INVALID, "model.wavelength must be strictly increasing"));
    if (c->H.n1 > (1 << 20)) return bail(fail(c, PAYNE_E_UNSUPPORTED, "npix > 2^20"));
    PostTables& T = c->T;
    fill_model_scalars(c->H, T);
    T.r_ann = model->resolution; T.npoly = opts->npoly;
    if ((rc = upload(c, c->H.vs_tab32, &T.vs_tab, c->owned))) return bail(rc);
    T.vs_tab += 1;                                           // (the table's entry of u = 0: one mirror entry sits in front of it)
    if ((rc = dev_alloc(c, 1, &c->d_T, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.lnlam, &T.lnlam, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.lam, &T.lam, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.tw, &T.tw, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.twf, &T.twf, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.rs1_idx, &T.rs1_idx, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.rs1_frac, &T.rs1_frac, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.bk1_idx, &T.bk1_idx, c->owned))) return bail(rc);
    if ((rc = upload(c, c->H.bk1_frac, &T.bk1_frac, c->owned))) return bail(rc);
    c->ld_hid = (maxh + 31) & ~31;
    if (model->n_layers > 2) {
      if ((rc = dev_alloc(c, (size_t)opts->b_max * c->ld_hid, &c->hid[0], c->owned))) return bail(rc);
      if ((rc = dev_alloc(c, (size_t)opts->b_max * c->ld_hid, &c->hid[1], c->owned))) return bail(rc);
      if (c->out_pix.p3 && (rc = dev_alloc(c, (size_t)3 * opts->b_max * c->ld_hid, &c->hid_p3, c->owned))) return bail(rc);
    }
    if ((rc = dev_alloc(c, (size_t)opts->b_max * std::max(model->npix, T.n1 <= 16384 ? T.n1 : 0), &c->raw, c->owned, false))) return bail(rc);   // (rows of n1 values: freq_rs)
    if ((rc = dev_alloc(c, (size_t)opts->b_max, &c->prep, c->owned, false))) return bail(rc);
    if (T.n1 > 16384) {                // spectrum larger than LDS: global-workspace kernel
      c->big_grid = opts->b_max < 256 ? opts->b_max : 256;
      // 32 768-point spectra on a geometric grid: the on-chip stages for two candidates at a time (four buffers per workgroup)
      c->big_chip2 = T.n1 == kChip2N1 && c->H.geo && !(opts->variant & PAYNE_V_BIG_WORKSPACE);
      if ((rc = dev_alloc(c, (size_t)c->big_grid * (c->big_chip2 ? 4 : 2) * T.n1, &c->big_ws, c->owned, false))) return bail(rc);
      if (c->big_chip2) {
        he = hipFuncSetAttribute(reinterpret_cast<const void*>(payne_post_chip2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kChipLdsBytes);
        if (he != hipSuccess) return bail(fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute(chip2): ") + hipGetErrorString(he)));
      }
      c->big_tiled = true;                 // the four-step transform where the length allows it (fft_tiled_ok); plain radix-8 passes otherwise
      // 65 536-point spectra on a geometric grid: the convolution stages stay on the compute unit (payne_post_chip_kernel)
      c->big_chip = T.n1 == kChipN1 && c->H.geo && !(opts->variant & PAYNE_V_BIG_WORKSPACE);
      if (c->big_chip) {
        he = hipFuncSetAttribute(reinterpret_cast<const void*>(payne_post_chip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)kChipLdsBytes);
        if (he != hipSuccess) return bail(fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute(chip): ") + hipGetErrorString(he)));
      }
      if (c->big_tiled) {
        he = hipFuncSetAttribute(reinterpret_cast<const void*>(payne_post_big_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(2 * fft_tile_complex() * sizeof(c32)));
        if (he != hipSuccess) return bail(fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute(big): ") + hipGetErrorString(he)));
      }
    }
    c->post_lds = (size_t)(T.n1 > 16384 ? 64 : fft_buf_floats(T.n1)) * 8 + (size_t)scratch_doubles(kPostThreads) * 8 + ((sizeof(CandState) + 15) & ~(size_t)15) + 16;
    // twiddles in LDS while two workgroups still fit a CU (160 KiB); larger spectra read them from L2
    const size_t tw_bytes = c->H.twf.size() * sizeof(c32);         // ~0.75 n1 entries
    c->post_tw_lds = (c->post_lds + tw_bytes) <= 80 * 1024;
    if (opts->variant & PAYNE_V_TW_GLOBAL) c->post_tw_lds = false;
    if (c->post_tw_lds) c->post_lds += tw_bytes;
#ifdef PAYNE_STAMPS
    if (const char* e = getenv("PAYNE_DIAG_LDS")) c->post_lds = std::max(c->post_lds, (size_t)atoi(e));   // diagnostic build: one workgroup per CU
#endif
    const int geom_n1 = (opts->variant & PAYNE_V_POST_GENERIC) ? 0 : T.n1;
    c->post_fn = pick_post_kernel(geom_n1, c->post_tw_lds);
    c->post_fn_lean = (opts->variant & PAYNE_V_POST_FULL) ? c->post_fn : pick_post_kernel(geom_n1, c->post_tw_lds, true);
    c->lean_available = c->post_fn_lean != c->post_fn;
    he = hipFuncSetAttribute(reinterpret_cast<const void*>(c->post_fn_lean), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->post_lds);
    if (he != hipSuccess) return bail(fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(he)));
    he = hipFuncSetAttribute(reinterpret_cast<const void*>(c->post_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->post_lds);
    if (he != hipSuccess) return bail(fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(he)));
    if ((rc = create_freq_rows(c, model, opts, geom_n1))) return bail(rc);
    c->has_model = true;
    if ((rc = bind_obs(c, obs))) return bail(rc);
  }

  if (phot && (rc = create_phot(c, phot, opts))) return bail(rc);
  *out = c;
  return PAYNE_OK;
}

extern "C" int payne_ctx_set_obs(payne_ctx* c, const payne_obs_desc* obs) {
  if (!c) return PAYNE_E_INVALID;
  if (!c->has_model) return fail(c, PAYNE_E_INVALID, "context has no spectral model");
  DeviceScope ds(c);
  return bind_obs(c, obs);
}

// Continuum network (ystpred.PayneSpecPredict(Cnnpath=...)): weights as for the spectral model; the label
// set must be the spectral model's.  cont == NULL removes it.
extern "C" int payne_ctx_set_continuum(payne_ctx* c, const payne_model_desc* cont) {
  if (!c) return PAYNE_E_INVALID;
  if (!c->has_model) return fail(c, PAYNE_E_INVALID, "context has no spectral model");
  DeviceScope ds(c);
  for (void* p : c->cont_owned) (void)hipFree(p);
  c->cont_owned.clear();
  c->has_cont = false;
  if (!cont) return PAYNE_OK;
  if (cont->n_layers < 3 || cont->n_layers > PAYNE_MAX_LAYERS) return fail(c, PAYNE_E_INVALID, "continuum.n_layers must be 3..8");
  if (cont->n_labels != c->n_labels) return fail(c, PAYNE_E_INVALID, "continuum.n_labels != model.n_labels");
  if (!cont->xmin || !cont->xmax || !cont->wavelength || cont->npix < 2)
    return fail(c, PAYNE_E_INVALID, "continuum.xmin/xmax/wavelength missing or npix < 2");
  if (cont->layers[0].n_in != cont->n_labels || cont->layers[cont->n_layers - 1].n_out != cont->npix)
    return fail(c, PAYNE_E_INVALID, "continuum layer shapes do not match n_labels / npix");
  int rc = PAYNE_OK, maxh = 0;
  if ((rc = adopt_layers(c, cont, c->clayers, c->cont_owned, "continuum ", &maxh))) return rc;
  c->cn_layers = cont->n_layers; c->cn_npix = cont->npix; c->cn_ld_hid = (maxh + 31) & ~31;
  for (int d = 0; d < cont->n_labels; ++d) { c->cxmin[d] = cont->xmin[d]; c->cxden[d] = cont->xmax[d] - cont->xmin[d]; }
  if ((rc = dev_alloc(c, (size_t)c->opts.b_max * c->cn_ld_hid, &c->chid[0], c->cont_owned))) return rc;
  if ((rc = dev_alloc(c, (size_t)c->opts.b_max * c->cn_ld_hid, &c->chid[1], c->cont_owned))) return rc;
  if ((rc = dev_alloc(c, (size_t)c->opts.b_max * cont->npix, &c->cont_raw, c->cont_owned, false))) return rc;
  // host tables: F_nu -> F_lambda factor (constants cancel in the median normalisation) and the np.interp map
  const int npc = cont->npix, npix = c->T.npix;
  std::vector<double> scale(npc), frac(npix);
  std::vector<int> idx(npix);
  const double* wc = cont->wavelength;
  for (int i = 1; i < npc; ++i)
    if (!(wc[i] > wc[i - 1])) return fail(c, PAYNE_E_INVALID, "continuum.wavelength must be strictly increasing");
  const double lref = wc[npc / 2];
  for (int i = 0; i < npc; ++i) { const double r = lref / wc[i]; scale[i] = r * r; }
  for (int i = 0; i < npix; ++i) {
    const double x = c->H.lam[i];
    if (x < wc[0] || x > wc[npc - 1]) { idx[i] = -1; frac[i] = 0.0; continue; }   // left = right = NaN
    int k = (int)(std::upper_bound(wc, wc + npc, x) - wc) - 1;
    if (k > npc - 2) k = npc - 2;
    idx[i] = k;
    frac[i] = (x - wc[k]) / (wc[k + 1] - wc[k]);
  }
  if ((rc = upload(c, scale, &c->cont_scale, c->cont_owned))) return rc;
  if ((rc = upload(c, idx, &c->cont_idx, c->cont_owned))) return rc;
  if ((rc = upload(c, frac, &c->cont_frac, c->cont_owned))) return rc;
  c->has_cont = true;
  return PAYNE_OK;
}

// LSF vector for the instrumental broadening: `lsf[n]` = Gaussian dispersion (AA) at each pixel of the bound
// observed grid (getspec(inst_R=array, outwave=...), ystpred.py:248-269).  While set, theta's Inst_R column
// is ignored.  NULL removes it; re-binding the observed grid removes it too.
static int set_lsf_impl(payne_ctx* c, const double* lsf_wave, const double* lsf, int n) {
  if (!c) return PAYNE_E_INVALID;
  if (!c->has_model) return fail(c, PAYNE_E_INVALID, "context has no spectral model");
  DeviceScope ds(c);
  for (void* p : c->lsf_owned) (void)hipFree(p);
  c->lsf_owned.clear();
  c->has_lsf = false;
  if (!lsf) return PAYNE_OK;
  if (!c->obs_bound) return fail(c, PAYNE_E_INVALID, "bind the observed grid before its LSF vector");
  if (!lsf_wave && n != c->T.nobs) return fail(c, PAYNE_E_INVALID, "the LSF vector must have one entry per observed pixel");
  if (lsf_wave && n < 2) return fail(c, PAYNE_E_INVALID, "an LSF vector on its own wavelengths needs at least two entries");
  for (int i = 0; i < n; ++i)
    if (!(lsf[i] > 0.0)) return fail(c, PAYNE_E_INVALID, "LSF dispersions must be positive");
  if (lsf_wave)
    for (int i = 1; i < n; ++i)
      if (!(lsf_wave[i] > lsf_wave[i - 1])) return fail(c, PAYNE_E_INVALID, "the LSF vector's wavelengths must be strictly increasing");
  std::vector<double> v(lsf, lsf + n);
  int rc;
  if ((rc = upload(c, v, &c->lsf, c->lsf_owned))) return rc;
  c->n_lsf = n;
  c->lsf_wave = c->d_obs_wave;
  if (lsf_wave) {
    std::vector<double> w(lsf_wave, lsf_wave + n);
    if ((rc = upload(c, w, &c->lsf_wave, c->lsf_owned))) return rc;
  }
  c->lsf_global = c->T.n1 > 8192 || (c->opts.variant & PAYNE_V_LSF_GLOBAL);
  c->lsf_chunk = c->lsf_global ? std::min(c->opts.b_max, 256) : c->opts.b_max;
  if ((rc = dev_alloc(c, (size_t)c->lsf_chunk * c->T.npix, &c->lsf_spec, c->lsf_owned, false))) return rc;
  if ((rc = dev_alloc(c, (size_t)c->lsf_chunk * (2 * (size_t)c->T.npix + c->T.n1), &c->lsf_ws, c->lsf_owned, false))) return rc;
  if (c->lsf_global) {
    if ((rc = dev_alloc(c, (size_t)c->lsf_chunk * 2 * fft_buf_floats(c->T.n1), &c->lsf_fws, c->lsf_owned, false))) return rc;
  } else {
    const size_t lds = (size_t)c->T.n1 * 8 + 2 * (size_t)fft_buf_floats(c->T.n1) * 4 + (256 + 8) * 8;
    hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void*>(payne_lsf_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(he));
  }
  c->has_lsf = true;
  return PAYNE_OK;
}
extern "C" int payne_ctx_set_lsf(payne_ctx* c, const double* lsf, int n) { return set_lsf_impl(c, nullptr, lsf, n); }
extern "C" int payne_ctx_set_lsf_on(payne_ctx* c, const double* lsf_wave, const double* lsf, int n) {
  if (c && lsf && !lsf_wave) return fail(c, PAYNE_E_INVALID, "lsf_wave is NULL");
  return set_lsf_impl(c, lsf_wave, lsf, n);
}

// ---- launches --------------------------------------------------------------
// Dynamic-LDS limits of the dense kernels, set on the context's device when the context is created (the attribute belongs
// to the function ON A DEVICE: a flag shared by every context would leave a second device of the same process without it).
static hipError_t set_dense_attributes() {
  hipError_t e = hipSuccess;
  auto set = [&](const void* f, size_t lds) {
    const hipError_t r = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = r;
  };
#define PAYNE_SET_T(K, ARGS, ...) set(reinterpret_cast<const void*>(PAYNE_UNPAREN K), __VA_ARGS__);
#define PAYNE_SET_F(K, ...) set(reinterpret_cast<const void*>(K), __VA_ARGS__);
  PAYNE_DENSE_KERNELS(PAYNE_SET_T, PAYNE_SET_F)
  return e;
}

template <int BM, int BN, int BK, bool FUSE>
static void launch_dense(DenseParams& p, hipStream_t s) {
  p.grid_m = (p.B + BM - 1) / BM;
  p.grid_n = (p.N + BN - 1) / BN;
#ifdef PAYNE_STAMPS
  p.stamps = FUSE ? nullptr : g_dense_stamps;
#endif
  PAYNE_LAUNCH_DENSE((payne_dense_kernel<BM, BN, BK, FUSE>), dim3(p.grid_m * p.grid_n), dim3(256), s, p);
}

static const payne_ctx::OutOperands& out_ops(const payne_ctx* c, bool freq) { return freq ? c->out_frq : c->out_pix; }

// The output layer's launch: plan_out (out_plan.hpp) has named the kernel, nothing is decided here.  `p` arrives with the layer as
// run_net describes every layer (W, K, bias, Y, ...); the form's operands are filled in once, in front of the switch.
// F32Dma: 64 x 128 tiles, 512 threads, BK-deep stages (NK: k-steps fixed at compile time or 0; NS: ring; PIPE: schedule -- see the
// kernel).  Bf16x3 and H2: operand planes; Big3*: persistent workgroups, one a compute unit.
static void launch_out(payne_ctx* c, DenseParams& p, hipStream_t s, const OutPlan& plan, bool freq, unsigned long long rot_seq) {
  const payne_ctx::OutOperands& o = out_ops(c, freq);
  const bool h2 = plan.form == OutForm::H2;
  if (plan.form != OutForm::Generic) {
    p.k_real = p.K;                                          // the layer's own width: the padded tail is skipped
    p.K = c->w_out_kp;                                       // padded pitch; X's pitch (ld_hid) is a multiple of 32 too
    p.grid_m = plan.grid_m; p.grid_n = plan.grid_n;
  }
  if (plan.form == OutForm::F32Dma) p.W = o.pad;
  if (plan.form >= OutForm::Bf16x3) {
    if (plan.sel) {                                          // rows of the resampled grid; pixels if the batch's records say so
      const payne_ctx::OutOperands& alt = c->out_pix;
      p.sel = c->rot_flag; p.sel_seq = rot_seq;
      p.Wp_alt = h2 ? alt.h2 : alt.p3; p.plane_w_alt = (size_t)p.N * c->w_out_kp; p.bias_alt = alt.bias; p.bias_shift_alt = alt.bias_shift;
      if (h2) p.rscale_alt = alt.rscale;
      p.N_alt = p.N; p.ldy_alt = p.ldy;
      p.N = c->T.n1; p.ldy = c->T.n1;
    }
    p.Wp = h2 ? o.h2 : o.p3; p.plane_w = (size_t)p.N * c->w_out_kp;
    if (h2) p.rscale = o.rscale;
    p.bias = o.bias; p.bias_shift = o.bias_shift;
    p.Xp = c->hid_p3; p.plane_x = (size_t)c->opts.b_max * c->ld_hid; p.ldp = c->ld_hid;
    if (plan.kernel == OutKernel::Dma3f10) {                 // the fp32 weights go through Wp's port
      p.W_alt = c->out_pix.pad;
      p.Wp = reinterpret_cast<const unsigned short*>(o.pad);
    }
  }
#ifdef PAYNE_STAMPS
  if (plan.form != OutForm::Generic && plan.kernel != OutKernel::Big3H2) p.stamps = g_dense_stamps;
#endif
  const dim3 grid(p.grid_m * p.grid_n), block(512);
  // (the fp32 ring's instantiations report the name their launch had inside its template)
#define OUT_DMA(BK, NK, NS, PIPE)                                                                                                    \
  PAYNE_LAUNCH_AS("(payne_dense_dma_kernel<WN, BK, NK, NS, PIPE>)", (payne_dense_dma_kernel<4, BK, NK, NS, PIPE>), grid, block,       \
                  (DenseLds<(payne_dense_dma_kernel<4, BK, NK, NS, PIPE>)>::value), s, p)
#define OUT_PLANES(kernel) PAYNE_LAUNCH_DENSE(kernel, grid, block, s, PAYNE_D3_LEAD_ARGS(p), p)
  switch (plan.kernel) {
    case OutKernel::GenericFused: launch_dense<64, 64, 32, true>(p, s); break;
    case OutKernel::Generic:      launch_dense<64, 64, 32, false>(p, s); break;     // nets whose hidden widths differ, the continuum network
    case OutKernel::Dma32Nk10Ns4: OUT_DMA(32, 10, 4, true); break;
    case OutKernel::Dma32Ns4:     OUT_DMA(32, 0, 4, true); break;
    case OutKernel::Dma32Ns3:     OUT_DMA(32, 0, 3, false); break;
    case OutKernel::Dma64Nk5:     OUT_DMA(64, 5, 3, true); break;
    case OutKernel::Dma64:        OUT_DMA(64, 0, 3, true); break;
    case OutKernel::Big3H2:       PAYNE_LAUNCH_DENSE(payne_dense_big3_kernel<true>, dim3(c->n_cu), dim3(512), s, p); break;
    case OutKernel::Big3:         PAYNE_LAUNCH_DENSE(payne_dense_big3_kernel<false>, dim3(c->n_cu), block, s, p); break;
    case OutKernel::Dma2hh5:      OUT_PLANES((payne_dense_dma2hh_kernel<5>)); break;
    case OutKernel::Dma2h5x64:    OUT_PLANES((payne_dense_dma2h_kernel<5, 64>)); break;
    case OutKernel::Dma2h10x32:   OUT_PLANES((payne_dense_dma2h_kernel<10, 32>)); break;
    case OutKernel::Dma2h0x32:    OUT_PLANES((payne_dense_dma2h_kernel<0, 32>)); break;
    case OutKernel::Dma3f10:      OUT_PLANES((payne_dense_dma3f_kernel<10>)); break;
    case OutKernel::Dma3Nk10Ns4:  OUT_PLANES((payne_dense_dma3_kernel<10, 4, true>)); break;
    case OutKernel::Dma3Ns4:      OUT_PLANES((payne_dense_dma3_kernel<0, 4, true>)); break;
    case OutKernel::Dma3Ns2:      OUT_PLANES((payne_dense_dma3_kernel<0, 2, false>)); break;
  }
#undef OUT_DMA
#undef OUT_PLANES
}

// The hidden-layer kernel's leading arguments carry two 16-bit values a dword (n_prep: 15 bits): what does not fit is refused
// by run_net before anything is launched (post_lead_fits is the post kernel's counterpart).
static bool hk_lead_fits(int B, int N, int K, int K0, int ldx, int ldwd, int ld_theta, int spec_K) {
  const long long n_gemm = (long long)((B + 31) / 32) * ((N + 31) / 32);
  return n_gemm <= 0xffff && (N + 31) / 32 <= 0xffff && (B + 255) / 256 <= 0x7fff && K <= 0xffff && K0 <= 0xffff && ldx <= 0xffff &&
         ldwd <= 0xffff && ld_theta <= 0xffff && (spec_K + kSpecChainsPerWg - 1) / kSpecChainsPerWg <= 0xffff;
}
template <bool FUSE>
static void launch_hidden(DenseParams& p, PrepArgs& pa, hipStream_t s, int n_cu = 256, int spec_K = 0, bool waves4 = false) {
  p.grid_m = (p.B + 31) / 32;
  p.grid_n = (p.N + 31) / 32;
  pa.n_gemm = p.grid_m * p.grid_n;
  if (!FUSE) { pa.out = nullptr; pa.sed_mags = nullptr; }
  pa.n_prep = pa.out ? (p.B + 255) / 256 : 0;
  pa.n_spec = pa.spec_walk ? (spec_K + kSpecChainsPerWg - 1) / kSpecChainsPerWg : 0;
  int n_sed = 0;
  if (pa.sed_mags) {
    // candidates per photometric tile: as few as keeps F x blocks within the workgroup slots the GEMM tiles, the record writers
    // and the proposals made ahead leave free -- TWO per CU (the launch's 79.9 KB of LDS): 16-candidate tiles at C3 (224 of them,
    // hidden launch 10.2 -> 9.4 us; a tile's time is mostly its fixed cost, 32-candidate tiles on one slot per CU measured 10.6)
    const int cb = sed_tile_cands(p.B, pa.P.F, 2 * n_cu - pa.n_gemm - pa.n_prep - pa.n_spec);
    pa.sed_cb = cb;
    n_sed = pa.P.F * ((p.B + cb - 1) / cb);
  }
#ifdef PAYNE_STAMPS
  p.stamps = FUSE ? g_hidden_stamps : nullptr;
#endif
  pa.n_sed = n_sed;
  // Eight waves for hk_tile_h2's tiles where the first layer is the expensive phase -- a sigmoid net's: forty activations a lane with four
  // waves (LinNet300: -1.2 us a step); a leaky-ReLU net's tile gains nothing (C2: 5.16 against 5.21 us) -- and no photometric tile rides
  // along: those are sized for two workgroups a CU.  PAYNE_HK_WAVES = 4 | 8 overrides (A/B runs).
  static const int force_waves = [] { const char* e = getenv("PAYNE_HK_WAVES"); return e ? atoi(e) : 0; }();
  const bool wide = FUSE && p.h2_tiles && n_sed == 0 && !waves4 && (force_waves ? force_waves == 8 : p.act0 == PAYNE_ACT_SIGMOID);
  const dim3 grid(pa.n_gemm + pa.n_prep + n_sed + pa.n_spec), block(wide ? 512 : 256);
  // the kernel's leading scalar parameters (preloaded into registers at wave start; two 16-bit values a dword)
  p.dma_tiles = (FUSE && p.Wd != nullptr) ? 1 : 0;
  const unsigned i0 = (unsigned)pa.n_spec | ((unsigned)pa.n_prep << 16) | ((unsigned)p.dma_tiles << 31), i1 = (unsigned)pa.n_gemm | ((unsigned)p.grid_n << 16);
  const unsigned i2 = FUSE ? ((unsigned)p.ld_theta | ((unsigned)p.n_labels << 16) | ((unsigned)(p.h2_tiles ? 1 : 0) << 31)) : ((unsigned)p.ldx | ((unsigned)p.ldwd << 16));
  const unsigned i4 = (unsigned)p.K | ((unsigned)(FUSE ? p.K0 : 0) << 16) | ((!FUSE && p.h2_tiles) ? 0x80000000u : 0u);
  const void* p0 = FUSE ? static_cast<const void*>(p.theta) : static_cast<const void*>(p.X);
  const float* p1 = FUSE ? p.W0 : p.Wd;
#define PAYNE_HK_ARGS p0, p1, p.b0, p.bias, i0, i1, i2, p.B, i4, p.N, p, pa
  if (!FUSE) PAYNE_LAUNCH_DENSE((payne_dense_hidden_kernel<false, 4>), grid, block, s, PAYNE_HK_ARGS);
  else if (p.n_labels <= 4) {
    if (wide) PAYNE_LAUNCH_DENSE((payne_dense_hidden_kernel<true, 4, 8>), grid, block, s, PAYNE_HK_ARGS);
    else PAYNE_LAUNCH_DENSE((payne_dense_hidden_kernel<true, 4>), grid, block, s, PAYNE_HK_ARGS);
  } else {
    if (wide) PAYNE_LAUNCH_DENSE((payne_dense_hidden_kernel<true, PAYNE_MAX_LABELS, 8>), grid, block, s, PAYNE_HK_ARGS);
    else PAYNE_LAUNCH_DENSE((payne_dense_hidden_kernel<true, PAYNE_MAX_LABELS>), grid, block, s, PAYNE_HK_ARGS);
  }
#undef PAYNE_HK_ARGS
}

// One network of the context: the spectral emulator or the continuum network.
struct NetRef {
  const payne_layer* layers; int n_layers; int n_labels; const double* xmin; const double* xden;
  float* const* hid; int ld_hid; float* out; int ld_out; float out_shift;
  bool spectral;                      // the spectral net owns the DMA / bf16x3 operand copies and the prep records
  bool freq = false;                  // spectral net: rows written in the frequency domain (c->out_frq)
  bool sel = false;                   // ... as rows of the resampled grid, or pixel rows if the batch's records say so (freq_rs)
};
static NetRef spectral_net(const payne_ctx* c) {
  return NetRef{c->layers, c->n_layers, c->n_labels, c->xmin, c->xden, c->hid, c->ld_hid, c->raw, c->T.npix, kBase, true};
}
static NetRef continuum_net(const payne_ctx* c) {
  return NetRef{c->clayers, c->cn_layers, c->n_labels, c->cxmin, c->cxden, c->chid, c->cn_ld_hid, c->cont_raw, c->cn_npix, 0.f, false};
}
// What one forward pass left for the post stage: filled by run_ann (payne_smooth_batch: the caller's pixels), read by run_post and
// everything below it.  A value of the call, not of the context: a view of some of the rows is a copy with the pointers moved on.
struct BatchRows {
  const float* rows = nullptr; int ld = 0;   // [B][ld]: the spectra shifted by -1, or their transforms
  bool freq = false;                  // the rows are in the frequency domain (PostTables::raw_freq of the launches that read them)
  // sel: ... rows of the resampled grid (pitch n1) that fall back to pixels (pitch npix) on the device if a candidate does not rotate;
  // rot_seq: the sequence number issued for them (c->rot_flag)
  bool sel = false; unsigned long long rot_seq = 0;
  const CandState* prep = nullptr;    // the batch's records; null: no dense launch wrote any for these rows
  bool spec = false;                  // the hidden-layer launch carried the walk's proposals (SpecReq)
};
// A sampler's walk in progress asks the likelihood batch being enqueued to make the next step's proposals ahead (rwalk_spec_wave).
struct SpecReq { const WalkTail* walk; const WalkState* w; int step, K; };      // (walk == null: no request)
// What plan_out and out_form (out_plan.hpp) read of this context for net N.
static OutFacts out_facts(const payne_ctx* c, const NetRef& N) {
  OutFacts f;
  f.variant = c->opts.variant; f.n_cu = c->n_cu; f.b_max = c->opts.b_max; f.ld_hid = c->ld_hid; f.w_out_kp = c->w_out_kp; f.n1 = c->T.n1;
  f.n_layers = N.n_layers; f.n_out = N.layers[N.n_layers - 1].n_out; f.spectral = N.spectral; f.freq = N.freq; f.sel = N.sel;
  f.dma_ok = c->dma_ok; f.act_scale = c->act_scale;
  f.p3 = c->out_pix.p3 && c->hid_p3; f.h2 = c->out_pix.h2; f.h2_freq = c->out_frq.h2; f.pad = c->out_pix.pad; f.pad_freq = c->out_frq.pad;
  return f;
}

// ---- one forward pass: run_net and its steps -------------------------------------------------------------------------
// Layer l of net N for a batch of B as every launch starts from it; layer 1 with the label encoding and the first layer fused in.
static DenseParams layer_params(const payne_ctx* c, const NetRef& N, int l, int B, const double* theta) {
  DenseParams p{};
  const payne_layer& L = N.layers[l];
  const bool last = l == N.n_layers - 1;
  p.W = L.w; p.K = L.n_in; p.bias = L.b; p.N = L.n_out; p.B = B; p.act = L.act;
  p.bias_shift = last ? N.out_shift : 0.f;
  p.Y = last ? N.out : N.hid[(l - 1) & 1];
  p.ldy = last ? N.ld_out : N.ld_hid;
  if (l > 1) { p.X = N.hid[(l - 2) & 1]; p.ldx = N.ld_hid; return p; }
  const payne_layer& L0 = N.layers[0];
  p.theta = theta; p.ld_theta = c->ncols;
  p.W0 = L0.w; p.b0 = L0.b; p.n_labels = N.n_labels; p.act0 = L0.act; p.K0 = L0.n_out;
  for (int d = 0; d < N.n_labels; ++d) { p.xmin[d] = N.xmin[d]; p.xden[d] = N.xden[d]; }
  return p;
}
// What hidden layer l adds: its weights' copy at the activations' pitch (hk_tile's LDS-DMA staging), and where its output goes as
// planes too -- the last one's as the output layer's operand (Bf16x3: three bf16 planes, H2: two fp16 planes), an earlier one's as the
// next layer's where the hidden layers run on fp16 pairs (hk_tile_h2x).  True: the copy is there.
static bool hidden_params(const payne_ctx* c, const NetRef& N, const OutPlan& plan, int l, DenseParams& p) {
  if (l == N.n_layers - 2 && plan.form >= OutForm::Bf16x3) {
    p.Yp = c->hid_p3; p.plane_y = (size_t)c->opts.b_max * c->ld_hid; p.ldp = c->ld_hid;
    if (plan.form == OutForm::H2) { p.yp_half = 1; p.yp_scale = c->act_scale; }
  } else if (l < N.n_layers - 2 && N.spectral && c->hid_pairs_deep) {
    p.Yp = c->hid_h2[(l - 1) & 1]; p.plane_y = (size_t)c->opts.b_max * 304; p.ldp = 304; p.yp_half = 1; p.yp_scale = c->hid_pairs[l + 1].in_scale;
  }
  if (!(N.spectral && c->w_hid_pad[l] && N.ld_hid >= HK_PITCH)) return false;
  p.Wd = c->w_hid_pad[l]; p.ldwd = N.ld_hid;
  return true;
}
// Layers 0 and 1 in one launch, and what rides in it: the post kernel's records (pa.out), a joint likelihood's photometric tiles
// (sed_tile), the walk's next proposals made ahead (spec_K of them; 0: none).  pairs: layer 1 on fp16 pairs (hk_tile_h2).
static void first_launch(payne_ctx* c, const NetRef& N, hipStream_t s, DenseParams& p, PrepArgs& pa, bool sed_rides, int spec_K, const SpecReq& spec,
                         bool pairs) {
  if (sed_rides) { pa.P = c->P; pa.sed_mags = c->mags_ws; pa.sed_off = 8 + c->opts.npoly; pa.sed_photscale = c->opts.photscale; }
  if (spec_K) { pa.spec_walk = spec.walk; pa.spec_w = *spec.w; pa.spec_step = spec.step; }
  if (pairs) {
    const payne_ctx::HidPairs& h = c->hid_pairs[1];
    p.h2_tiles = 1; p.Wh = h.planes; p.plane_wh = (size_t)p.N * 304; p.rs1 = h.rs; p.a0_scale = h.in_scale;
  }
  ProfScope ps(c, s, 3);
  launch_hidden<true>(p, pa, s, c->n_cu, spec_K, (c->opts.variant & PAYNE_V_HID_WAVES4) != 0);
}
static void hidden_launch(payne_ctx* c, const NetRef& N, int l, hipStream_t s, DenseParams& p) {
  PrepArgs pa{};
  if (N.spectral && c->hid_pairs_deep) {                    // both operands as planes
    const payne_ctx::HidPairs& h = c->hid_pairs[l];
    p.h2_tiles = 1; p.Wh = h.planes; p.plane_wh = (size_t)p.N * 304; p.rs1 = h.rs;
    p.Xp = c->hid_h2[(l - 2) & 1]; p.plane_x = (size_t)c->opts.b_max * 304;
  }
  ProfScope ps(c, s, 3);
  launch_hidden<false>(p, pa, s);
}
// Layers 2 .. n - 2 in ONE launch: hand-offs inside a 32-candidate row block (payne_dense_chain_kernel; opt-in: a hop costs more
// than a launch on this machine, NOTES R6.10).
static void chain_launch(payne_ctx* c, const NetRef& N, const OutPlan& plan, int B, hipStream_t s) {
  const int n = N.n_layers;
  ChainParams cp{};
  cp.n = n - 3;
  for (int q = 2; q <= n - 2; ++q) {
    const payne_layer& Lq = N.layers[q];
    cp.Wh[q - 2] = c->hid_pairs[q].planes; cp.rs[q - 2] = c->hid_pairs[q].rs; cp.bias[q - 2] = Lq.b; cp.act[q - 2] = Lq.act;
    cp.out_scale[q - 2] = (q == n - 2) ? c->act_scale : c->hid_pairs[q + 1].in_scale;
  }
  cp.buf[0] = c->hid_h2[0]; cp.buf[1] = c->hid_h2[1]; cp.plane_x = (size_t)c->opts.b_max * 304;
  cp.first_in = 0;                                          // (layer 1 wrote hid_h2[0]: hidden_params, (l - 1) & 1 at l = 1)
  cp.Yp_last = c->hid_p3; cp.plane_y_last = (size_t)c->opts.b_max * c->ld_hid; cp.ldp_last = c->ld_hid; cp.half_last = plan.form == OutForm::H2 ? 1 : 0;
  cp.flags = c->chain_flags; cp.grid_n = (N.layers[2].n_out + 31) / 32;
  cp.target0 = c->chain_calls * (unsigned long long)cp.grid_n;
  cp.B = B; cp.N = N.layers[2].n_out; cp.grid_m = (B + 31) / 32; cp.grid_m_max = (c->opts.b_max + 31) / 32;
  ++c->chain_calls;
  ProfScope ps(c, s, 3);
  PAYNE_LAUNCH_DENSE(payne_dense_chain_kernel, dim3(cp.grid_m_max * cp.grid_n), dim3(256), s, cp);
}
static void out_launch(payne_ctx* c, const NetRef& N, const OutPlan& plan, hipStream_t s, unsigned long long rot_seq, DenseParams& p) {
  ProfScope ps(c, s, 0);
  launch_out(c, p, s, plan, N.freq, rot_seq);
}

// ANN forward for the batch -> N.out [B][ld_out] (the spectral net: c->raw, shifted by -1): the first launch; the chain or the hidden
// layers 2 .. n - 2; the output layer.  A two-layer net is the output layer alone, the labels fused in (OutKernel::GenericFused).
// `sed`: a joint likelihood's photometric nets ride in the first launch; *sed is cleared when they did.
// `R` (the spectral net's): gets the records and whether the walk's proposals `spec` went along; R->rot_seq is read where plan.sel.
static int run_net(payne_ctx* c, const NetRef& N, const OutPlan& plan, const double* theta, int B, double instr_factor, hipStream_t s,
                   BatchRows* R = nullptr, bool* sed = nullptr, const SpecReq& spec = SpecReq{}) {
  const int n = N.n_layers;
  const unsigned v = c->opts.variant;
  const unsigned long long rot_seq = plan.sel ? R->rot_seq : 0;
  DenseParams out = layer_params(c, N, n - 1, B, theta);
  if (n > 2) {
    DenseParams p = layer_params(c, N, 1, B, theta);
    const bool dma_l1 = hidden_params(c, N, plan, 1, p);
    const bool records = N.spectral && c->prep && c->obs_bound && !(v & PAYNE_V_NO_PREP);
    const bool sed_rides = sed && *sed && N.spectral && sed_tile_ok(c->P.H) && !(v & PAYNE_V_SED_OWN_LAUNCH);
    // (proposals ahead: when this batch's post kernel will run the chain step at its tail, run_post)
    const int spec_K = (N.spectral && spec.walk && records && c->lean_available && !c->big_ws) ? spec.K : 0;
    // (hk_tile_h2: 32-bit byte offsets into theta)
    const bool pairs_l1 = dma_l1 && c->hid_pairs[1].planes && p.K <= 304 && (unsigned long long)B * (unsigned)c->ncols * 8ull < (1ull << 31);
    // layers 2 .. n - 2 as one launch: asked for, three at least, all on fp16 pairs, a workgroup slot for every tile of the largest batch
    const bool chained = N.spectral && c->hid_pairs_deep && plan.form >= OutForm::Bf16x3 && n - 2 >= 3 && (v & PAYNE_V_HID_CHAIN) &&
                         ((c->opts.b_max + 31) / 32) * ((N.layers[2].n_out + 31) / 32) <= 2 * c->n_cu && n - 3 <= kChainMax;
    for (int l = 1; l <= (chained ? 1 : n - 2); ++l) {     // what the packed arguments cannot hold is refused before anything is launched
      const payne_layer& L = N.layers[l];
      const int ldwd = (N.spectral && c->w_hid_pad[l] && N.ld_hid >= HK_PITCH) ? N.ld_hid : 0;
      if (!(l == 1 ? hk_lead_fits(B, L.n_out, L.n_in, p.K0, 0, ldwd, p.ld_theta, spec_K) : hk_lead_fits(B, L.n_out, L.n_in, 0, N.ld_hid, ldwd, 0, 0)))
        return fail(c, PAYNE_E_UNSUPPORTED, "batch x hidden width beyond what the hidden-layer kernel's packed arguments hold (65 535 tiles of 32 x 32)");
    }
    PrepArgs pa{};
    pa.T = c->T; pa.T.raw_freq = N.freq ? 1 : 0; pa.instr_factor = instr_factor;      // (the tables are read by the records' writers only)
    pa.out = records ? c->prep : nullptr;
    if (plan.sel) { pa.rot_flag = c->rot_flag; pa.rot_seq = rot_seq; }
    first_launch(c, N, s, p, pa, sed_rides, spec_K, spec, pairs_l1);
    if (sed_rides) *sed = false;
    if (R) { R->prep = pa.out; R->spec = spec_K != 0; }
    if (chained) chain_launch(c, N, plan, B, s);
    else
      for (int l = 2; l <= n - 2; ++l) {
        p = layer_params(c, N, l, B, theta);
        hidden_params(c, N, plan, l, p);
        hidden_launch(c, N, l, s, p);
      }
  }
  out_launch(c, N, plan, s, rot_seq, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("dense launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}

// ---- continuum network ------------------------------------------------------------------
// ystpred.py:191-209 for one candidate per workgroup: F_nu -> F_lambda, normalise by the NaN-ignoring
// median, interpolate onto the spectral ANN grid (NaN outside), multiply into the spectrum.
// The median is the middle of a bitonic sort in LDS (fp64 keys, NaN -> +inf); the spectrum row is stored
// shifted by -1, so (m C) - 1 = (m - 1) C + (C - 1).
__global__ void __launch_bounds__(256) payne_cont_kernel(const float* __restrict__ cont, int npc, int npc2,
                                                          const double* __restrict__ scale, const int* __restrict__ idx,
                                                          const double* __restrict__ frac, float* raw, int npix) {
  extern __shared__ __attribute__((aligned(16))) double cs[];       // [npc2] sort buffer (npc2 == 0: none, median by selection)
  __shared__ double med_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = cont + (size_t)b * npc;
  if (npc2 == 0) {                                                   // rows longer than LDS: radix selection, no size limit
    __shared__ int hist[256], cnt_s;
    __shared__ unsigned long long bc[2];
    const double med = nanmedian_select<256>([&](int i) { return (double)row[i] * scale[i]; }, npc, hist, bc, &cnt_s);
    float* r = raw + (size_t)b * npix;
    for (int i = tid; i < npix; i += 256) {
      const int k = idx[i];
      double C = __builtin_nan("");
      if (k >= 0) {
        const double q0 = (double)row[k] * scale[k], q1 = (double)row[k + 1] * scale[k + 1];
        C = (q0 + frac[i] * (q1 - q0)) / med;
      }
      const float m1 = r[i];
      r[i] = (float)((double)m1 * C + (C - 1.0));
    }
    return;
  }
  int nv = 0;
  for (int i = tid; i < npc2; i += 256) {
    double q = INFINITY;
    if (i < npc) { q = (double)row[i] * scale[i]; if (q != q) q = INFINITY; else ++nv; }
    cs[i] = q;
  }
  // number of non-NaN values: wave ballot sums through LDS would do; npc is small, use an LDS atomic
  __shared__ int nvalid;
  if (tid == 0) nvalid = 0;
  __syncthreads();
  atomicAdd(&nvalid, nv);
  for (int k = 2; k <= npc2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < npc2; i += 256) {
        const int p = i ^ j;
        if (p > i) {
          const double a = cs[i], c2 = cs[p];
          const bool up = (i & k) == 0;
          if ((a > c2) == up) { cs[i] = c2; cs[p] = a; }
        }
      }
    }
  __syncthreads();
  if (tid == 0) {
    const int n = nvalid;                                            // np.nanmedian: mean of the two middle values
    med_s = n == 0 ? __builtin_nan("") : ((n & 1) ? cs[n >> 1] : 0.5 * (cs[(n >> 1) - 1] + cs[n >> 1]));
  }
  __syncthreads();
  const double med = med_s;
  float* r = raw + (size_t)b * npix;
  for (int i = tid; i < npix; i += 256) {
    const int k = idx[i];
    double C = __builtin_nan("");
    if (k >= 0) {
      const double q0 = (double)row[k] * scale[k], q1 = (double)row[k + 1] * scale[k + 1];
      C = (q0 + frac[i] * (q1 - q0)) / med;
    }
    const float m1 = r[i];
    r[i] = (float)((double)m1 * C + (C - 1.0));
  }
}

// `instr_factor`: what Inst_R is multiplied by (2.355 in the likelihood / genspec, 1 in getspec): the
// first-layer launch also writes the post kernel's per-candidate records (c->prep) for that factor.
// `pixels`: the caller reads the rows themselves (stage 0); otherwise they may be handed to the post kernel already transformed.
// *R: what the post stage finds (run_post).
static int run_ann(payne_ctx* c, const double* theta, int B, double instr_factor, hipStream_t s, BatchRows* R, bool with_cont = true,
                   bool* sed = nullptr, bool pixels = false, const SpecReq& spec = SpecReq{}) {
  NetRef N = spectral_net(c);
  // (the continuum multiplies pixel by pixel; the form: the launch that reads the restated weights is the one that runs)
  N.freq = c->freq_ok && !pixels && !(c->has_cont && with_cont) && out_form(out_facts(c, N)) >= OutForm::Bf16x3;
  // rows of a resampled grid need this batch's records (their writers report a candidate that does not rotate) and a first layer
  // fused into the hidden-layer launch (>= 3 layers), and the plain post kernel behind them
  if (N.freq && c->freq_rs && !(c->prep && c->obs_bound && !(c->opts.variant & PAYNE_V_NO_PREP) && c->n_layers >= 3 && !c->has_lsf)) N.freq = false;
  N.sel = N.freq && c->freq_rs;
  *R = BatchRows{};
  R->rows = c->raw; R->ld = N.sel ? c->T.n1 : c->T.npix; R->freq = N.freq; R->sel = N.sel;
  if (N.sel) R->rot_seq = ++c->rot_seq;
  int rc = run_net(c, N, plan_out(out_facts(c, N), B), theta, B, instr_factor, s, R, sed, spec);
  if (rc || !c->has_cont || !with_cont) return rc;
  const NetRef C = continuum_net(c);
  if ((rc = run_net(c, C, plan_out(out_facts(c, C), B), theta, B, instr_factor, s))) return rc;
  int npc2 = 1;
  while (npc2 < c->cn_npix) npc2 <<= 1;
  if (npc2 > 4096 || (c->opts.variant & PAYNE_V_SELECT_MEDIAN)) npc2 = 0;     // median by selection instead of an LDS sort
  PAYNE_LAUNCH(payne_cont_kernel, dim3(B), dim3(256), (size_t)npc2 * 8, s, c->cont_raw, c->cn_npix, npc2, c->cont_scale,
                     c->cont_idx, c->cont_frac, c->raw, c->T.npix);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("continuum launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}

static int check_call(payne_ctx* c, const void* in, int B, const void* out) {
  if (!c) return PAYNE_E_INVALID;
  if (!in || !out) return fail(c, PAYNE_E_INVALID, "NULL input/output pointer");
  if (B <= 0) return fail(c, PAYNE_E_INVALID, "B must be > 0");
  if (B > c->opts.b_max) return fail(c, PAYNE_E_BATCH, "B exceeds opts.b_max");
  return on_device(c);
}

static int run_sed(payne_ctx* c, const double* in, int ld, int mode, int B, double* mags, hipStream_t s) {
  {
    ProfScope ps(c, s, 2);
    PAYNE_LAUNCH(payne_sed_kernel, dim3(c->P.F, B), dim3(64), (size_t)c->P.H * 16, s, c->P, in, ld, mode,
                       8 + c->opts.npoly, c->opts.photscale, mags);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("sed launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}

// One launch of the post kernel this context was built with, over the B candidates whose rows R describes.  `a` arrives with the
// caller's part (theta, instr_factor, stage and outputs, photometry; the diagnostic build's stamps); the rows' part is filled in here.
static int launch_post(payne_ctx* c, const BatchRows& R, PostArgs a, int B, hipStream_t s, TailReq* tail = nullptr) {
  PostTables T = c->T; T.raw_freq = R.freq ? 1 : 0;
  a.ld_theta = c->ncols;
  a.raw = R.rows; a.ld_raw = R.ld; a.prep = R.prep;
  if (R.sel) { a.ld_raw_alt = T.npix; a.rot_flag = c->rot_flag; a.rot_seq = R.rot_seq; }
  // (stamps are written by the full instantiations only, and not by payne_post_chip2_kernel: such a context's stamps are the big kernel's)
  const bool lean = a.out_stage < 0 && !a.out && a.prep && !c->big_ws && !a.stamps;
  if (tail && lean && c->lean_available) {
    a.tail = tail->dev; a.tail_step = tail->step; a.tail_propose = tail->propose; tail->done = true;
    a.tail_spec = (R.spec && tail->propose && tail->spec) ? 1 : 0;
  }
  c->last_rows_freq = R.freq;
  {
    ProfScope ps(c, s, 1);
    if (c->big_ws && c->big_chip) {
      const int grid = B < c->big_grid ? B : c->big_grid;
      PAYNE_LAUNCH(payne_post_chip_kernel, dim3(grid), dim3(kChipThreads), kChipLdsBytes, s, T, a, c->big_ws, B);
    } else if (c->big_ws && c->big_chip2 && !a.stamps) {
      const int pairs = (B + 1) / 2, grid = pairs < c->big_grid ? pairs : c->big_grid;
      PAYNE_LAUNCH(payne_post_chip2_kernel, dim3(grid), dim3(kChipThreads), kChipLdsBytes, s, T, a, c->big_ws, B);
    } else if (c->big_ws) {
      const int grid = B < c->big_grid ? B : c->big_grid;
      const int tiled = c->big_tiled ? 1 : 0;
      const size_t lds = (tiled & 1) ? 2 * (size_t)fft_tile_complex() * sizeof(c32) : 0;
      PAYNE_LAUNCH(payne_post_big_kernel, dim3(grid), dim3(kBigThreads), lds, s, T, a, c->big_ws, B, tiled);
    } else {
      if (!post_lead_fits(a.ld_raw, a.ld_theta, a.n_filters)) return fail(c, PAYNE_E_INVALID, "row pitch / theta columns / filters beyond what the post kernel's packed arguments hold");
      PAYNE_LAUNCH(lean ? c->post_fn_lean : c->post_fn, dim3(B), dim3(kPostThreads), c->post_lds, s, T.twf, a.raw, a.prep, a.theta,
                   a.rot_flag, a.mags, post_lead_ints(a.ld_raw, a.ld_theta, a.n_filters, T.raw_freq), (unsigned)a.rot_seq, T, a);
      c->last_kernel[1] = post_kernel_label((c->opts.variant & PAYNE_V_POST_GENERIC) ? 0 : T.n1, c->post_tw_lds, lean && c->lean_available);
    }
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("post launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}

// LSF path: spectra after rotational broadening (post kernel, stage 5) -> payne_lsf_kernel, a chunk of the batch at a time
static int run_post_lsf(payne_ctx* c, const BatchRows& R, const double* theta, int B, int stage, float* out, int ld_out, double* lnl,
                        bool with_phot, hipStream_t s) {
  for (int off = 0; off < B; off += c->lsf_chunk) {
    const int nb = std::min(c->lsf_chunk, B - off);
    const double* th = theta + (size_t)off * c->ncols;
    BatchRows v = R;                                        // this chunk's rows of the ANN output and their records
    v.rows += (size_t)off * R.ld; if (v.prep) v.prep += off;
    PostArgs p5{};
    p5.theta = th; p5.instr_factor = 1.0; p5.out = c->lsf_spec; p5.ld_out = c->T.npix; p5.out_stage = 5;
    if (int rc = launch_post(c, v, p5, nb, s)) return rc;
    LsfArgs a{};
    a.theta = th; a.ld_theta = c->ncols; a.spec = c->lsf_spec; a.ld_spec = c->T.npix;
    a.obs_wave = c->d_obs_wave; a.lsf = c->lsf; a.lsf_wave = c->lsf_wave; a.n_lsf = c->n_lsf;
    a.ws = c->lsf_ws; a.ws_stride = 2 * (size_t)c->T.npix + c->T.n1;
    a.fws = c->lsf_fws; a.fws_stride = 2 * (size_t)fft_buf_floats(c->T.n1);
    a.out = out ? out + (size_t)off * ld_out : nullptr; a.ld_out = ld_out; a.out_stage = stage; a.lnl = lnl ? lnl + off : nullptr;
    if (with_phot) { a.mags = c->mags_ws + (size_t)off * c->P.F; a.n_filters = c->P.F; a.obs_mag = c->obs_mag; a.obs_err = c->obs_err; }
    {
      ProfScope ps(c, s, 1);
      if (c->lsf_global) {
        PAYNE_LAUNCH(payne_lsf_kernel<true>, dim3(nb), dim3(256), (size_t)(256 + 8) * 8, s, c->T, a);
      } else {
        const size_t lds = (size_t)c->T.n1 * 8 + 2 * (size_t)fft_buf_floats(c->T.n1) * 4 + (256 + 8) * 8;
        PAYNE_LAUNCH(payne_lsf_kernel<false>, dim3(nb), dim3(256), lds, s, c->T, a);
      }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("lsf launch: ") + hipGetErrorString(e));
  }
  return PAYNE_OK;
}

// The post stage of a batch: with an LSF vector bound the stages that reach the observed grid take the LSF path, all else is one launch.
static int run_post(payne_ctx* c, const BatchRows& R, const double* theta, int B, double instr_factor, int stage, float* out, int ld_out,
                    double* lnl, bool with_phot, hipStream_t s, TailReq* tail = nullptr) {
  if (c->has_lsf && (stage < 0 || stage == 2 || stage == 3)) return run_post_lsf(c, R, theta, B, stage, out, ld_out, lnl, with_phot, s);
  PostArgs a{};
  a.theta = theta; a.instr_factor = instr_factor;
  a.out = out; a.ld_out = ld_out; a.out_stage = stage; a.lnl = lnl;
  if (with_phot) { a.mags = c->mags_ws; a.n_filters = c->P.F; a.obs_mag = c->obs_mag; a.obs_err = c->obs_err; }
  return launch_post(c, R, a, B, s, tail);
}

int payne::ctx_lnlike(payne_ctx* c, const double* theta, int B, double* lnl, void* stream, TailReq* tail) {
  int rc = check_call(c, theta, B, lnl);
  if (rc) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (c->has_phot && !c->has_obs_phot) return fail(c, PAYNE_E_INVALID, "photometric model without observed magnitudes");
  if (c->has_model && (!c->obs_bound || !c->T.obs_f1)) return fail(c, PAYNE_E_INVALID, "no observed spectrum (flux, eflux) bound");
  bool sed_pending = c->has_phot;                           // the photometric nets: in the hidden-layer launch when there is one
  TailReq* const tl = (c->has_lsf || (c->opts.variant & PAYNE_V_NO_WALK_TAIL)) ? nullptr : tail;
  SpecReq spec{};
  if (tl && tl->propose && tl->spec && !(c->opts.variant & PAYNE_V_NO_WALK_SPEC)) spec = SpecReq{tl->dev, tl->spec, tl->step, B};
  BatchRows R;
  if (c->has_model && (rc = run_ann(c, theta, B, 2.355, s, &R, true, &sed_pending, false, spec))) return rc;
  if (sed_pending && (rc = run_sed(c, theta, c->ncols, 1, B, c->mags_ws, s))) return rc;
  if (c->has_model) return run_post(c, R, theta, B, 2.355, -1, nullptr, 0, lnl, c->has_phot, s, tl);
  hipLaunchKernelGGL(payne_photonly_kernel, dim3((B + 127) / 128), dim3(128), 0, s, c->mags_ws, c->obs_mag, c->obs_err, c->P.F, B, lnl);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("photonly launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}
extern "C" int payne_lnlike_batch(payne_ctx* c, const double* theta, int B, double* lnl, void* stream) {
  return ctx_lnlike(c, theta, B, lnl, stream, nullptr);
}

extern "C" int payne_predict_batch(payne_ctx* c, const double* theta, int B, int stage, unsigned flags, float* out,
                                   int ld_out, void* stream) {
  int rc = check_call(c, theta, B, out);
  if (rc) return rc;
  if (!c->has_model) return fail(c, PAYNE_E_INVALID, "context has no spectral model");
  if (stage < 0 || stage > 4) return fail(c, PAYNE_E_INVALID, "stage must be 0..4");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (stage == PAYNE_STAGE_CONT) {                       // predictcont: the continuum network's own output
    if (!c->has_cont) return fail(c, PAYNE_E_INVALID, "no continuum network bound");
    if (ld_out < c->cn_npix) return fail(c, PAYNE_E_INVALID, "ld_out too small");
    const NetRef C = continuum_net(c);
    if ((rc = run_net(c, C, plan_out(out_facts(c, C), B), theta, B, 1.0, s))) return rc;
    hipError_t he = hipMemcpy2DAsync(out, (size_t)ld_out * 4, c->cont_raw, (size_t)c->cn_npix * 4, (size_t)c->cn_npix * 4, B,
                                     hipMemcpyDeviceToDevice, s);
    if (he != hipSuccess) return fail(c, PAYNE_E_HIP, std::string("hipMemcpy2DAsync: ") + hipGetErrorString(he));
    return PAYNE_OK;
  }
  if (stage >= 2 && !c->obs_bound) return fail(c, PAYNE_E_INVALID, "no observed grid bound");
  if (ld_out < (stage >= 2 ? c->T.nobs : c->T.npix)) return fail(c, PAYNE_E_INVALID, "ld_out too small");
  BatchRows R;
  if ((rc = run_ann(c, theta, B, (flags & PAYNE_F_FWHM_R) ? 2.355 : 1.0, s, &R, stage != 0, nullptr, stage == 0))) return rc;   // stage 0 = predictspec: no continuum
  return run_post(c, R, theta, B, (flags & PAYNE_F_FWHM_R) ? 2.355 : 1.0, stage, out, ld_out, nullptr, false, s);
}

// smoothspec on caller-supplied spectra (PayneSpecPredict.smoothspec, ystpred.py:279-281 -> utils.smoothing.smoothspec):
// the same stages as payne_predict_batch with the ANN forward pass replaced by `spectra` (full flux on the context's
// model grid).  stage 1: rotational broadening on the model grid; stage 2/3: ... and instrumental broadening onto
// the bound observed grid.
__global__ void payne_shift_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out, int npix, int B) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B * npix) { const size_t b = i / npix, p = i - b * npix; out[i] = in[b * ld_in + p] - kBase; }
}
extern "C" int payne_smooth_batch(payne_ctx* c, const float* spectra, int ld_spec, const double* theta, int B, int stage,
                                  unsigned flags, float* out, int ld_out, void* stream) {
  int rc = check_call(c, theta, B, out);
  if (rc) return rc;
  if (!spectra) return fail(c, PAYNE_E_INVALID, "spectra is NULL");
  if (!c->has_model) return fail(c, PAYNE_E_INVALID, "context has no spectral model");
  if (stage < 1 || stage > 4) return fail(c, PAYNE_E_INVALID, "stage must be 1..4");
  if (stage == PAYNE_SMOOTH_VSINI_TO_OBS && c->has_lsf) return fail(c, PAYNE_E_INVALID, "stage 4 with an LSF vector bound");
  if (ld_spec < c->T.npix) return fail(c, PAYNE_E_INVALID, "ld_spec too small");
  if (stage >= 2 && !c->obs_bound) return fail(c, PAYNE_E_INVALID, "no observed grid bound");
  if (ld_out < (stage >= 2 ? c->T.nobs : c->T.npix)) return fail(c, PAYNE_E_INVALID, "ld_out too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t n = (size_t)B * c->T.npix;
  hipLaunchKernelGGL(payne_shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, spectra, ld_spec, c->raw, c->T.npix, B);
  BatchRows R;                                             // the caller's pixels: no dense launch wrote records for these rows
  R.rows = c->raw; R.ld = c->T.npix;
  // stage 1 here is smoothspec('vsini') itself: getspec's edge rule (ystpred.py:223-224) is not part of it
  // stage 4: ... interpolated from the stage's own resampled grid onto the bound observed grid (smoothspec('vsini', outwave=...))
  return run_post(c, R, theta, B, (flags & PAYNE_F_FWHM_R) ? 2.355 : 1.0, stage == 1 ? 6 : (stage == PAYNE_SMOOTH_VSINI_TO_OBS ? 7 : stage), out, ld_out,
                  nullptr, false, s);
}

extern "C" int payne_sed_batch(payne_ctx* c, const double* pars, int B, double* mags, void* stream) {
  int rc = check_call(c, pars, B, mags);
  if (rc) return rc;
  if (!c->has_phot) return fail(c, PAYNE_E_INVALID, "context has no photometric model");
  return run_sed(c, pars, 9, 0, B, mags, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int payne_bc_batch(payne_ctx* c, const double* x, int B, double* bc, void* stream) {
  int rc = check_call(c, x, B, bc);
  if (rc) return rc;
  if (!c->has_phot) return fail(c, PAYNE_E_INVALID, "context has no photometric model");
  return run_sed(c, x, 6, 2, B, bc, reinterpret_cast<hipStream_t>(stream));
}

// ---- per-kernel timing ---------------------------------------------------------
extern "C" int payne_profile(payne_ctx* c, int enable) {
  if (!c) return PAYNE_E_INVALID;
  c->prof = enable != 0;
  if (enable) {
    c->prof_used = 0;
    for (int k = 0; k < 4; ++k) { c->prof_ms[k] = 0.0; c->prof_n[k] = 0; }
  }
  return PAYNE_OK;
}

extern "C" int payne_profile_read(payne_ctx* c, int kind, double* total_ms, long long* launches) {
  if (!c || kind < 0 || kind > 3) return PAYNE_E_INVALID;
  for (size_t i = 0; i < c->prof_used; ++i) {
    auto& r = c->prof_pool[i];
    float ms = 0.f;
    HIPCHK(c, hipEventSynchronize(r.e1));
    HIPCHK(c, hipEventElapsedTime(&ms, r.e0, r.e1));
    c->prof_ms[r.kind] += ms;
    c->prof_n[r.kind] += 1;
  }
  c->prof_used = 0;
  if (total_ms) *total_ms = c->prof_ms[kind];
  if (launches) *launches = c->prof_n[kind];
  return PAYNE_OK;
}

#ifdef PAYNE_STAMPS
// Diagnostic build only: cycle stamps of the first hidden-layer launch ([grid][16], slot 15 = grid size).
extern "C" int payne_diag_hidden_stamps(payne_ctx* c, const double* theta, int B, unsigned long long* host, int max_blocks) {
  int rc = check_call(c, theta, B, host);
  if (rc) return rc;
  unsigned long long* d = nullptr;
  const size_t nb_ = (size_t)(max_blocks < 0 ? -max_blocks : max_blocks);
  HIPCHK(c, hipMalloc(&d, nb_ * 16 * 8));
  HIPCHK(c, hipMemset(d, 0, nb_ * 16 * 8));
  if (max_blocks < 0) { max_blocks = -max_blocks; g_dense_stamps = d; } else g_hidden_stamps = d;   // negative: the output layer
  bool sed = c->has_phot;
  BatchRows R;
  rc = run_ann(c, theta, B, 2.355, nullptr, &R, true, &sed);
  g_hidden_stamps = nullptr; g_dense_stamps = nullptr;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(host, d, (size_t)max_blocks * 16 * 8, hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return rc;
}
// Diagnostic build only: one lnlike batch with per-phase cycle stamps of the post kernel.
// stamps: host [B][payne_diag_stamp_row()] (slot 0 = number of stamps, slots 1.. = s_memtime after each barrier).
extern "C" int payne_diag_stamp_row(void) { return kStampRow; }
extern "C" int payne_diag_post_stamps(payne_ctx* c, const double* theta, int B, unsigned long long* stamps_host) {
  int rc = check_call(c, theta, B, stamps_host);
  if (rc) return rc;
  unsigned long long* d = nullptr; double* lnl = nullptr;
  hipError_t e = hipMalloc(&d, (size_t)B * kStampRow * 8);
  if (e == hipSuccess) e = hipMalloc(&lnl, (size_t)B * 8);
  if (e == hipSuccess) e = hipMemset(d, 0, (size_t)B * kStampRow * 8);
  BatchRows R;
  if (e == hipSuccess) rc = run_ann(c, theta, B, 2.355, nullptr, &R);
  if (e == hipSuccess && !rc) {
    PostArgs a{};
    a.theta = theta; a.instr_factor = 2.355; a.out_stage = -1; a.lnl = lnl;
    a.stamps = d; a.stamp_sparse = getenv("PAYNE_DIAG_SPARSE") ? 1 : 0;
    rc = launch_post(c, R, a, B, nullptr);
  }
  if (e == hipSuccess && !rc) e = hipDeviceSynchronize();
  if (e == hipSuccess && !rc) e = hipMemcpy(stamps_host, d, (size_t)B * kStampRow * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d); (void)hipFree(lnl);
  return e != hipSuccess ? fail(c, PAYNE_E_HIP, std::string("post stamps: ") + hipGetErrorString(e)) : rc;
}
#endif
