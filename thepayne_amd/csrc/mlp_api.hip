// mlp_api.hip -- the entry points of the four MLP handle families of include/payne_hip.h, none of which touches a payne_ctx:
//   payne_lnmlp_*          the photometric LayerNorm + SiLU networks (photANN_new); the kernel is k_lnmlp.hip
//   payne_lnmlp_train_*    training them (trainphot.TrainMod), and payne_lnmlp_dropout_mask; the kernels are k_lnmlp_train.hip
//   payne_specmlp_train_*  training the spectral networks (trainspec.TrainMod); the kernels are k_specmlp_train.hip
//   payne_specjac_*        the spectral networks' label gradients, and payne_fisher_batch; the kernels are k_specjac.hip
// A handle is a device number, a bag of device allocations and the kernels' argument struct.  Every entry point selects the
// handle's device through an OnDevice (host_prologue.hpp), which puts the caller's back on every way out; the descriptors are checked by
// mlp_desc.hpp; a create call that fails leaves its message for payne_last_error(NULL).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/payne_hip.h"
#include "host_prologue.hpp"
#include "mlp_desc.hpp"
#include "specjac_core.hpp"

namespace ln = payne::lnmlp;
namespace sp = payne::specmlp;
namespace sj = payne::specjac;
namespace md = payne::mlp_desc;

int payne_lnmlp_launch(const ln::NetArgs& net, const double* x, int ld_x, int N, float* y, int ld_y, void* stream);
int payne_lnmlp_train_launch(const ln::TrainNet& net, const float* x, int ld_x, const float* t, int ld_t, int N, int train,
                             unsigned long long seed, unsigned long long step, float scale, void* stream);
int payne_lnmlp_train_update(const ln::TrainNet& net, int N, const ln::RadamStep& rs, void* stream);
int payne_lnmlp_train_loss_sum(const ln::TrainNet& net, int N, double* acc, int first, double denom, double* out, void* stream);
int payne_specmlp_train_forward(const sp::SpecNet& net, const float* x, int ld_x, const float* t, int ld_t, float* y, int ld_y, int N,
                                int train, void* stream);
int payne_specmlp_train_backward(const sp::SpecNet& net, int N, const ln::RadamStep& rs, void* stream);
int payne_specmlp_train_loss_sum(const sp::SpecNet& net, int N, double* acc, int first, double* out, void* stream);
int payne_specjac_launch(const sj::JacNet& net, const double* x, int ld_x, int N, float* y, int ld_y, float* jac, int ld_j, void* stream);
int payne_specjac_prepare(const sj::JacNet& net);
int payne_fisher_launch(const float* rows, int ld, int K, int n, int B, const double* w, double* F, void* stream);

namespace {

using payne::host::DeviceBag;
using payne::host::OnDevice;
using payne::host::destroy;
using payne::host::fail;
int fail(const md::Status& s) { return fail(s.code, s.msg); }

// N rows in chunks of the workspace's `rows`: pass(r0, n) for each chunk until one fails.
template <class Pass>
int for_row_chunks(int N, int rows, Pass&& pass) {
  int rc = PAYNE_OK;
  for (int r0 = 0; r0 < N && !rc; r0 += rows) rc = pass(r0, N - r0 < rows ? N - r0 : rows);
  return rc;
}

// The layers a training handle of either kind shares: the master weights, their two stored copies, the moments, the gradients
// and the workspace of `rows` rows; n_vec per-column vectors a layer (Net::kHiddenVecs).
template <class Layer, class DescLayer>
void train_layer_alloc(DeviceBag& bag, Layer& A, Layer* next, const DescLayer& L, bool first, size_t rows, int n_vec) {
  const size_t nw = (size_t)L.n_in * L.n_out, npad = (size_t)ln::pad32(L.n_out), kpad = (size_t)ln::pad32(L.n_in);
  const size_t tiles = rows / ln::kTileRows;
  A.n_in = L.n_in;
  A.n_out = L.n_out;
  A.wm = bag.floats(nw);
  A.gw = bag.floats(nw);
  A.mw = bag.floats(nw);
  A.vw = bag.floats(nw);
  A.wp = bag.floats(ln::packed_floats(L.n_in, L.n_out));
  A.wt = bag.floats(ln::packed_floats(L.n_out, L.n_in));
  A.vec = bag.floats(n_vec * npad);
  A.gvec = bag.floats(n_vec * npad);
  A.mvec = bag.floats(n_vec * npad);
  A.vvec = bag.floats(n_vec * npad);
  if (first) A.a_in = bag.floats(rows * kpad);                      // (a hidden block's output is the next layer's a_in, below)
  A.dz = bag.floats(rows * npad);
  A.slab = bag.floats(tiles * n_vec * npad);
  if (next) next->a_in = bag.floats(rows * npad);
  std::vector<float> pk, pt;
  md::pack_both(L.w, L.n_in, L.n_out, pk, pt);
  bag.put_floats(A.wm, L.w, nw);
  bag.put_floats(A.wp, pk.data(), pk.size());
  bag.put_floats(A.wt, pt.data(), pt.size());
  bag.put_floats(A.vec, L.b, (size_t)L.n_out);
}

// What the step / loss calls of either training family check of their arguments
template <class Handle>
int train_check(Handle* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N) {
  if (!h || N < 0) return PAYNE_E_INVALID;
  if (ld_x < h->net.L[0].n_in || ld_t < h->net.L[h->net.n_layers - 1].n_out) return PAYNE_E_INVALID;
  if (N > 0 && (!x_dev || !t_dev)) return PAYNE_E_INVALID;
  return PAYNE_OK;
}

// Device -> host copies of a _train_get call behind the handle's last stream; false once one has failed.
struct Fetch {
  bool ok;
  explicit Fetch(void* last_stream) : ok(hipStreamSynchronize(reinterpret_cast<hipStream_t>(last_stream)) == hipSuccess) {}
  void operator()(const float* dst, const float* src, size_t n) {
    if (ok && hipMemcpy(const_cast<float*>(dst), src, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) ok = false;
  }
};

}  // namespace

// ---- photometric LayerNorm + SiLU networks (photANN_new) ----------------------------------------------------------------
struct payne_lnmlp {
  int device = 0;
  ln::NetArgs net{};
  DeviceBag bag;
};

extern "C" void payne_lnmlp_destroy(payne_lnmlp* h) { destroy(h, false); }

extern "C" int payne_lnmlp_create(int device, const payne_lnmlp_desc* d, payne_lnmlp** out) {
  static_assert(PAYNE_LNMLP_MAX_LAYERS == ln::kMaxLayers && PAYNE_LNMLP_MAX_IN == ln::kMaxIn && PAYNE_LNMLP_MAX_WIDTH == ln::kMaxWidth,
                "payne_hip.h and lnmlp_core.hpp disagree on the limits");
  const char* fn = "payne_lnmlp_create";
  if (!d || !out) return fail(PAYNE_E_INVALID, "payne_lnmlp_create: null descriptor or handle pointer");
  *out = nullptr;
  if (md::Status s = md::check_lnmlp_layers(fn, d, true)) return fail(s);
  if (md::Status s = md::check_lnmlp_limits(fn, d)) return fail(s);

  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_lnmlp_create: hipSetDevice");
  payne_lnmlp* h = new payne_lnmlp;
  h->device = device;
  DeviceBag& bag = h->bag;
  auto padded = [&](const float* src, int n, int n_pad) {
    std::vector<float> v((size_t)n_pad, 0.0f);
    memcpy(v.data(), src, (size_t)n * sizeof(float));
    return static_cast<const float*>(bag.upload(v.data(), v.size() * sizeof(float)));
  };
  auto doubles = [&](const double* src, int n) { return static_cast<const double*>(bag.upload(src, (size_t)n * sizeof(double))); };
  h->net.n_layers = d->n_layers;
  for (int l = 0; l < d->n_layers; ++l) {
    const payne_lnmlp_layer& L = d->layers[l];
    ln::LayerArgs& A = h->net.L[l];
    const int n_pad = ln::col_tiles(L.n_out) * ln::kTile;
    std::vector<float> pk(ln::packed_floats(L.n_in, L.n_out));
    ln::pack_weights(L.w, L.n_in, L.n_out, pk.data());
    A.w = static_cast<const float*>(bag.upload(pk.data(), pk.size() * sizeof(float)));
    A.b = padded(L.b, L.n_out, n_pad);
    A.gain = L.ln_gain ? padded(L.ln_gain, L.n_out, n_pad) : nullptr;
    A.beta = L.ln_bias ? padded(L.ln_bias, L.n_out, n_pad) : nullptr;
    A.n_in = L.n_in;
    A.n_out = L.n_out;
  }
  const int d_in = d->layers[0].n_in, d_out = d->layers[d->n_layers - 1].n_out;
  if (d->in_mid) {
    h->net.in_mid = doubles(d->in_mid, d_in);
    h->net.in_std = doubles(d->in_std, d_in);
  }
  if (d->out_mid) {
    h->net.out_mid = doubles(d->out_mid, d_out);
    h->net.out_std = doubles(d->out_std, d_out);
  }
  if (!h->bag.ok) {
    payne_lnmlp_destroy(h);
    return fail(PAYNE_E_HIP, "payne_lnmlp_create: copying the network to the device failed");
  }
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_lnmlp_eval(payne_lnmlp* h, const double* x_dev, int ld_x, int N, float* y_dev, int ld_y, void* stream) {
  if (!h || N < 0) return PAYNE_E_INVALID;
  if (ld_x < h->net.L[0].n_in || ld_y < h->net.L[h->net.n_layers - 1].n_out) return PAYNE_E_INVALID;
  if (N == 0) return PAYNE_OK;
  if (!x_dev || !y_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  return payne_lnmlp_launch(h->net, x_dev, ld_x, N, y_dev, ld_y, stream);
}

// ---- training the photometric networks (trainphot.TrainMod) ---------------------------------------------------------------
struct payne_lnmlp_train {
  int device = 0;
  ln::TrainNet net{};
  payne_lnmlp_train_opts opts{};
  int rows = 0;                                                     // the workspace's rows: max_rows rounded up to the tile
  long long t = 0;                                                  // steps taken
  double* loss_acc = nullptr;
  void* last_stream = nullptr;
  DeviceBag bag;
};

extern "C" void payne_lnmlp_train_destroy(payne_lnmlp_train* h) { destroy(h, true); }

extern "C" int payne_lnmlp_train_create(int device, const payne_lnmlp_desc* d, const payne_lnmlp_train_opts* o, payne_lnmlp_train** out) {
  const char* fn = "payne_lnmlp_train_create";
  if (!d || !o || !out) return fail(PAYNE_E_INVALID, "payne_lnmlp_train_create: null descriptor, options or handle pointer");
  *out = nullptr;
  if (md::Status s = md::check_lnmlp_layers(fn, d, false)) return fail(s);
  for (int l = 0; l < ln::kMaxLayers; ++l)
    if (!(o->dropout_p[l] >= 0.0 && o->dropout_p[l] < 1.0)) return fail(PAYNE_E_INVALID, "payne_lnmlp_train_create: dropout_p outside [0, 1)");
  if (md::Status s = md::check_optimiser(fn, o->max_rows, o->lr, o->beta1, o->beta2, o->eps)) return fail(s);
  if (md::Status s = md::check_lnmlp_limits(fn, d)) return fail(s);

  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_lnmlp_train_create: hipSetDevice");
  payne_lnmlp_train* h = new payne_lnmlp_train;
  h->device = device;
  h->opts = *o;
  h->rows = (o->max_rows + ln::kTileRows - 1) / ln::kTileRows * ln::kTileRows;
  DeviceBag& bag = h->bag;
  const size_t rows = (size_t)h->rows;
  h->net.n_layers = d->n_layers;
  for (int l = 0; l < d->n_layers; ++l) {
    const payne_lnmlp_layer& L = d->layers[l];
    ln::TrainLayer& A = h->net.L[l];
    const bool last = l + 1 == d->n_layers;
    const size_t npad = (size_t)ln::pad32(L.n_out);
    train_layer_alloc(bag, A, last ? nullptr : &h->net.L[l + 1], L, l == 0, rows, ln::TrainNet::kHiddenVecs);
    A.p = last ? 0.0f : (float)o->dropout_p[l];
    A.xh = bag.floats(rows * npad);
    A.rs = bag.floats(rows);
    if (L.ln_gain) bag.put_floats(A.vec + npad, L.ln_gain, (size_t)L.n_out);
    if (L.ln_bias) bag.put_floats(A.vec + 2 * npad, L.ln_bias, (size_t)L.n_out);
  }
  h->net.loss_slab = static_cast<double*>(bag.zeros(rows / ln::kTileRows * sizeof(double)));
  h->loss_acc = static_cast<double*>(bag.zeros(sizeof(double)));
  if (!h->bag.ok) {
    payne_lnmlp_train_destroy(h);
    return fail(PAYNE_E_HIP, "payne_lnmlp_train_create: allocating or copying to the device failed");
  }
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_lnmlp_train_step(payne_lnmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N,
                                      double* loss_dev, void* stream) {
  int rc = train_check(h, x_dev, ld_x, t_dev, ld_t, N);
  if (rc) return rc;
  if (N > h->opts.max_rows) return PAYNE_E_INVALID;
  if (N == 0) return PAYNE_OK;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  const int d_out = h->net.L[h->net.n_layers - 1].n_out;
  h->last_stream = stream;
  rc = payne_lnmlp_train_launch(h->net, x_dev, ld_x, t_dev, ld_t, N, 1, h->opts.seed, (unsigned long long)h->t,
                                ln::loss_grad_scale(N, d_out), stream);
  if (!rc && loss_dev) rc = payne_lnmlp_train_loss_sum(h->net, N, h->loss_acc, 1, (double)N * (double)d_out, loss_dev, stream);
  if (!rc) {
    rc = payne_lnmlp_train_update(h->net, N, ln::radam_scalars(h->opts.lr, h->opts.beta1, h->opts.beta2, h->opts.eps, h->t + 1), stream);
    h->t += 1;
  }
  return rc;
}

extern "C" int payne_lnmlp_train_loss(payne_lnmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N,
                                      double* loss_dev, void* stream) {
  const int rc = train_check(h, x_dev, ld_x, t_dev, ld_t, N);
  if (rc) return rc;
  if (N == 0) return PAYNE_OK;
  if (!loss_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  const double denom = (double)N * (double)h->net.L[h->net.n_layers - 1].n_out;
  h->last_stream = stream;
  return for_row_chunks(N, h->rows, [&](int r0, int n) {
    const int rc = payne_lnmlp_train_launch(h->net, x_dev + (size_t)r0 * (size_t)ld_x, ld_x, t_dev + (size_t)r0 * (size_t)ld_t, ld_t, n, 0, 0,
                                            0, 0.0f, stream);
    return rc ? rc : payne_lnmlp_train_loss_sum(h->net, n, h->loss_acc, r0 == 0, denom, r0 + n == N ? loss_dev : nullptr, stream);
  });
}

extern "C" int payne_lnmlp_train_get(payne_lnmlp_train* h, int what, payne_lnmlp_desc* host_out) {
  if (!h || !host_out || (what != PAYNE_LNMLP_PARAMS && what != PAYNE_LNMLP_GRADS) || host_out->n_layers != h->net.n_layers)
    return PAYNE_E_INVALID;
  for (int l = 0; l < h->net.n_layers; ++l) {
    const payne_lnmlp_layer& L = host_out->layers[l];
    const bool last = l + 1 == h->net.n_layers;
    if (L.n_in != h->net.L[l].n_in || L.n_out != h->net.L[l].n_out || !L.w || !L.b || (!last && (!L.ln_gain || !L.ln_bias)))
      return PAYNE_E_INVALID;
  }
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  Fetch take(h->last_stream);
  for (int l = 0; l < h->net.n_layers; ++l) {
    const payne_lnmlp_layer& L = host_out->layers[l];
    const ln::TrainLayer& A = h->net.L[l];
    const size_t npad = (size_t)ln::pad32(A.n_out);
    const float* vec = what == PAYNE_LNMLP_PARAMS ? A.vec : A.gvec;
    take(L.w, what == PAYNE_LNMLP_PARAMS ? A.wm : A.gw, (size_t)A.n_in * A.n_out);
    take(L.b, vec, (size_t)A.n_out);
    if (l + 1 < h->net.n_layers) {
      take(L.ln_gain, vec + npad, (size_t)A.n_out);
      take(L.ln_bias, vec + 2 * npad, (size_t)A.n_out);
    }
  }
  return take.ok ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" long long payne_lnmlp_train_steps(payne_lnmlp_train* h) { return h ? h->t : -1; }

extern "C" int payne_lnmlp_dropout_mask(unsigned long long seed, unsigned long long step, int layer, int n_rows, int n_cols, double p,
                                        unsigned char* out_host) {
  if (!out_host || n_rows < 0 || n_cols < 0 || layer < 0 || !(p >= 0.0 && p < 1.0)) return PAYNE_E_INVALID;
  for (int r = 0; r < n_rows; ++r)
    for (int c = 0; c < n_cols; ++c) out_host[(size_t)r * (size_t)n_cols + (size_t)c] = ln::keep(seed, step, layer, r, c, (float)p) ? 1 : 0;
  return PAYNE_OK;
}

// ---- training the spectral networks (trainspec.TrainMod) --------------------------------------------------------------------
struct payne_specmlp_train {
  int device = 0;
  sp::SpecNet net{};
  payne_specmlp_train_opts opts{};
  int rows = 0;                                                     // the workspace's rows: max_rows rounded up to the tile
  long long t = 0;                                                  // steps taken
  double* loss_acc = nullptr;
  void* last_stream = nullptr;
  DeviceBag bag;
};

extern "C" void payne_specmlp_train_destroy(payne_specmlp_train* h) { destroy(h, true); }

extern "C" int payne_specmlp_train_create(int device, const payne_specmlp_desc* d, const payne_specmlp_train_opts* o, payne_specmlp_train** out) {
  const char* fn = "payne_specmlp_train_create";
  if (!d || !o || !out) return fail(PAYNE_E_INVALID, "payne_specmlp_train_create: null descriptor, options or handle pointer");
  *out = nullptr;
  if (md::Status s = md::check_specmlp_layers(fn, d)) return fail(s);
  if (md::Status s = md::check_optimiser(fn, o->max_rows, o->lr, o->beta1, o->beta2, o->eps)) return fail(s);
  if (md::Status s = md::check_specmlp_limits(fn, d, sp::kMaxIn, "inputs")) return fail(s);

  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_specmlp_train_create: hipSetDevice");
  payne_specmlp_train* h = new payne_specmlp_train;
  h->device = device;
  h->opts = *o;
  h->rows = (o->max_rows + sp::kTileRows - 1) / sp::kTileRows * sp::kTileRows;
  DeviceBag& bag = h->bag;
  const size_t rows = (size_t)h->rows, tiles = rows / sp::kTileRows;
  h->net.n_layers = d->n_layers;
  h->net.act = d->act == PAYNE_SPECMLP_SIGMOID ? sp::kActSigmoid : sp::kActLeaky;
  for (int l = 0; l < d->n_layers; ++l)
    train_layer_alloc(bag, h->net.L[l], l + 1 < d->n_layers ? &h->net.L[l + 1] : nullptr, d->layers[l], l == 0, rows, sp::SpecNet::kHiddenVecs);
  h->net.loss_slab = static_cast<double*>(bag.zeros(tiles * (size_t)sp::out_chunks(d->layers[d->n_layers - 1].n_out) * sizeof(double)));
  h->loss_acc = static_cast<double*>(bag.zeros(sizeof(double)));
  if (!h->bag.ok) {
    payne_specmlp_train_destroy(h);
    return fail(PAYNE_E_HIP, "payne_specmlp_train_create: allocating or copying to the device failed");
  }
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_specmlp_train_step(payne_specmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N,
                                        double* loss_dev, void* stream) {
  int rc = train_check(h, x_dev, ld_x, t_dev, ld_t, N);
  if (rc) return rc;
  if (N > h->opts.max_rows) return PAYNE_E_INVALID;
  if (N == 0) return PAYNE_OK;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  h->last_stream = stream;
  rc = payne_specmlp_train_forward(h->net, x_dev, ld_x, t_dev, ld_t, nullptr, 0, N, 1, stream);
  if (!rc && loss_dev) rc = payne_specmlp_train_loss_sum(h->net, N, h->loss_acc, 1, loss_dev, stream);
  if (!rc) {
    rc = payne_specmlp_train_backward(h->net, N, ln::radam_scalars(h->opts.lr, h->opts.beta1, h->opts.beta2, h->opts.eps, h->t + 1), stream);
    h->t += 1;
  }
  return rc;
}

extern "C" int payne_specmlp_train_loss(payne_specmlp_train* h, const float* x_dev, int ld_x, const float* t_dev, int ld_t, int N,
                                        double* loss_dev, void* stream) {
  const int rc = train_check(h, x_dev, ld_x, t_dev, ld_t, N);
  if (rc) return rc;
  if (N == 0) return PAYNE_OK;
  if (!loss_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  h->last_stream = stream;
  return for_row_chunks(N, h->rows, [&](int r0, int n) {
    const int rc = payne_specmlp_train_forward(h->net, x_dev + (size_t)r0 * (size_t)ld_x, ld_x, t_dev + (size_t)r0 * (size_t)ld_t, ld_t, nullptr,
                                               0, n, 0, stream);
    return rc ? rc : payne_specmlp_train_loss_sum(h->net, n, h->loss_acc, r0 == 0, r0 + n == N ? loss_dev : nullptr, stream);
  });
}

extern "C" int payne_specmlp_train_predict(payne_specmlp_train* h, const float* x_dev, int ld_x, int N, float* y_dev, int ld_y, void* stream) {
  if (!h || N < 0) return PAYNE_E_INVALID;
  if (ld_x < h->net.L[0].n_in || ld_y < h->net.L[h->net.n_layers - 1].n_out) return PAYNE_E_INVALID;
  if (N == 0) return PAYNE_OK;
  if (!x_dev || !y_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  h->last_stream = stream;
  return for_row_chunks(N, h->rows, [&](int r0, int n) {
    return payne_specmlp_train_forward(h->net, x_dev + (size_t)r0 * (size_t)ld_x, ld_x, nullptr, 0, y_dev + (size_t)r0 * (size_t)ld_y, ld_y, n, 0,
                                       stream);
  });
}

extern "C" int payne_specmlp_train_set_lr(payne_specmlp_train* h, double lr) {
  if (!h || !(lr > 0.0) || !std::isfinite(lr)) return PAYNE_E_INVALID;
  h->opts.lr = lr;
  return PAYNE_OK;
}

extern "C" int payne_specmlp_train_get(payne_specmlp_train* h, int what, payne_specmlp_desc* host_out) {
  if (!h || !host_out || (what != PAYNE_SPECMLP_PARAMS && what != PAYNE_SPECMLP_GRADS) || host_out->n_layers != h->net.n_layers)
    return PAYNE_E_INVALID;
  for (int l = 0; l < h->net.n_layers; ++l) {
    const payne_specmlp_layer& L = host_out->layers[l];
    if (L.n_in != h->net.L[l].n_in || L.n_out != h->net.L[l].n_out || !L.w || !L.b) return PAYNE_E_INVALID;
  }
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  Fetch take(h->last_stream);
  for (int l = 0; l < h->net.n_layers; ++l) {
    const payne_specmlp_layer& L = host_out->layers[l];
    const sp::SpecLayer& A = h->net.L[l];
    take(L.w, what == PAYNE_SPECMLP_PARAMS ? A.wm : A.gw, (size_t)A.n_in * A.n_out);
    take(L.b, what == PAYNE_SPECMLP_PARAMS ? A.vec : A.gvec, (size_t)A.n_out);
  }
  return take.ok ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" long long payne_specmlp_train_steps(payne_specmlp_train* h) { return h ? h->t : -1; }

// ---- label gradients of the spectral networks and Fisher matrices -----------------------------------------------------------
struct payne_specjac {
  int device = 0;
  sj::JacNet net{};                                                 // (scale: the physical one, 1 / (xmax - xmin))
  int stars = 0;                                                    // the workspace's stars: max_rows rounded up to whole tiles
  DeviceBag bag;
};

extern "C" void payne_specjac_destroy(payne_specjac* h) { destroy(h, true); }

extern "C" int payne_specjac_create(int device, const payne_specmlp_desc* d, const double* xmin, const double* xmax, int max_rows,
                                    payne_specjac** out) {
  const char* fn = "payne_specjac_create";
  if (!d || !xmin || !xmax || !out) return fail(PAYNE_E_INVALID, "payne_specjac_create: null descriptor, xmin, xmax or handle pointer");
  *out = nullptr;
  if (md::Status s = md::check_specmlp_layers(fn, d)) return fail(s);
  if (max_rows < 1) return fail(PAYNE_E_INVALID, "payne_specjac_create: max_rows < 1");
  if (md::Status s = md::check_specmlp_limits(fn, d, sj::kMaxLabels, "labels")) return fail(s);
  const int d_in = d->layers[0].n_in;
  for (int k = 0; k < d_in; ++k)
    if (!std::isfinite(xmin[k]) || !std::isfinite(xmax[k]) || xmin[k] == xmax[k])
      return fail(PAYNE_E_INVALID, "payne_specjac_create: label " + std::to_string(k) + ": xmin / xmax not finite or equal");

  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_specjac_create: hipSetDevice");
  payne_specjac* h = new payne_specjac;
  h->device = device;
  const int tiles = sj::tiles_of(max_rows, d_in);
  h->stars = tiles * sj::stars_per_tile(d_in);
  DeviceBag& bag = h->bag;
  h->net.n_layers = d->n_layers;
  h->net.act = d->act == PAYNE_SPECMLP_SIGMOID ? sj::kActSigmoid : sj::kActLeaky;
  for (int l = 0; l < d->n_layers; ++l) {
    const payne_specmlp_layer& L = d->layers[l];
    std::vector<float> pk(sj::packed_floats(L.n_in, L.n_out));
    sj::pack_weights(L.w, L.n_in, L.n_out, pk.data());
    float* w = bag.floats(pk.size());
    float* b = bag.floats((size_t)sj::pad32(L.n_out));
    bag.put_floats(w, pk.data(), pk.size());
    bag.put_floats(b, L.b, (size_t)L.n_out);
    h->net.L[l].w = w;
    h->net.L[l].b = b;
    h->net.L[l].n_in = L.n_in;
    h->net.L[l].n_out = L.n_out;
  }
  for (int k = 0; k < sj::kMaxLabels; ++k) {
    h->net.xmin[k] = k < d_in ? xmin[k] : 0.0;
    h->net.xmax[k] = k < d_in ? xmax[k] : 1.0;
    h->net.scale[k] = sj::label_scale(h->net.xmin[k], h->net.xmax[k]);
  }
  h->net.a_last = bag.floats((size_t)tiles * sj::kTileRows * (size_t)sj::pad32(d->layers[d->n_layers - 1].n_in));
  if (bag.ok && payne_specjac_prepare(h->net) != PAYNE_OK) bag.ok = false;
  if (!h->bag.ok) {
    payne_specjac_destroy(h);
    return fail(PAYNE_E_HIP, "payne_specjac_create: allocating, copying to the device or reserving LDS failed");
  }
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_specjac_eval(payne_specjac* h, const double* labels_dev, int ld_x, int N, float* y_dev, int ld_y, float* jac_dev,
                                  int ld_j, unsigned flags, void* stream) {
  if (!h || N < 0 || (flags & ~PAYNE_JAC_ENCODED)) return PAYNE_E_INVALID;
  const int d_in = h->net.L[0].n_in, d_out = h->net.L[h->net.n_layers - 1].n_out;
  if (ld_x < d_in || ld_j < d_out || (y_dev && ld_y < d_out)) return PAYNE_E_INVALID;
  if (N == 0) return PAYNE_OK;
  if (!labels_dev || !jac_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  sj::JacNet net = h->net;
  if (flags & PAYNE_JAC_ENCODED)
    for (int k = 0; k < sj::kMaxLabels; ++k) net.scale[k] = 1.0f;
  return for_row_chunks(N, h->stars, [&](int r0, int n) {
    return payne_specjac_launch(net, labels_dev + (size_t)r0 * (size_t)ld_x, ld_x, n, y_dev ? y_dev + (size_t)r0 * (size_t)ld_y : nullptr, ld_y,
                                jac_dev + (size_t)r0 * (size_t)d_in * (size_t)ld_j, ld_j, stream);
  });
}

extern "C" int payne_fisher_batch(int device, const float* rows_dev, int ld, int K, int n, int B, const double* w_dev, double* F_dev,
                                  void* stream) {
  if (K < 1 || n < 1 || B < 0 || ld < n) return PAYNE_E_INVALID;
  if (K > sj::kMaxFisherRows) return PAYNE_E_UNSUPPORTED;
  if (B == 0) return PAYNE_OK;
  if (!rows_dev || !w_dev || !F_dev) return PAYNE_E_INVALID;
  OnDevice on(device);
  if (!on.ok()) return PAYNE_E_HIP;
  return payne_fisher_launch(rows_dev, ld, K, n, B, w_dev, F_dev, stream);
}
