// sampler_api.hip -- the sampler's entry points of include/payne_hip.h: payne_sampler_*, payne_prior_transform_batch,
// payne_lnprob_u_batch, the random walk (payne_rwalk_*), slice sampling (payne_slice_*) and the nested sampler's proposal queue with
// its turn on the host (payne_ns_rwalk_queue*) or on the device (payne_ns_queue_dev_*); payne_ns_consume and its kin are ns_core.hpp.
// The only unit that includes sampler_kernels.hpp and ns_core.hpp: the kernels launched here, and the one whose attribute
// payne_ns_queue_dev_init sets, are this unit's copies.  A sampler belongs to a context and asks of it what ctx_api.hpp offers: the
// error string, the device (sticky, as in every entry point of a context), three numbers and the likelihood batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/payne_hip.h"
#include "ctx_api.hpp"
#include "ns_core.hpp"
#include "queue_block.hpp"
#include "sampler_kernels.hpp"

using namespace payne;

#define HIPCHK(ctx, call)                                                                                   \
  do {                                                                                                      \
    hipError_t e_ = (call);                                                                                 \
    if (e_ != hipSuccess) return ctx_fail((ctx), PAYNE_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct payne_sampler {
  payne_ctx* ctx = nullptr;
  SamplerDev sd{};
  int k_max = 0;
  double *u_prop = nullptr, *v_prop = nullptr, *lnprior = nullptr, *lnl = nullptr, *rows = nullptr, *axes = nullptr;
  int* inside = nullptr;
  int* ell = nullptr;                     // per-chain ellipsoid index of the walk in progress
  int* nredraw = nullptr;                 // per-chain count of proposals redrawn because they left the unit cube
  double* spec = nullptr;                 // [k_max][2][kSpecStride] the next step's proposals made ahead (null: more dimensions / columns than a record holds)
  // staging of payne_ns_rwalk_queue: chains (u | v | lnprob) and counters (nacc | ncall | nredraw), device + pinned host
  double *q_dev = nullptr, *q_host = nullptr;
  // the queue's transfers as KERNELS on mapped host memory (q_host_dev: the device's address of q_host) and its completion as a word
  // the last of them writes into it (q_flag, behind the staging block; q_seq: the value the queue in flight will write) -- the
  // host reads that word instead of synchronising the stream: hipMemcpyAsync's own enqueue (17 us) and the wake-up out of
  // hipStreamSynchronize were most of the GPU's idle time between two queues (NOTES R4.16).  Null: the block has no device address.
  double* q_host_dev = nullptr; volatile unsigned long long* q_flag = nullptr; unsigned long long* q_flag_dev = nullptr; unsigned long long q_seq = 0;
  unsigned* q_arrivals = nullptr;         // device word: workgroups of the results' transfer that have finished (wraps to zero)
  // The queue's TURN on the device (payne_ns_queue_dev_*): the live set lives there (two copies, written in turn), the turn kernel
  // merges a queue's proposals into it, adapts the scale, raises the threshold and draws the next start points -- the next queue
  // is ENQUEUED before the current one has finished, and the GPU goes from one to the other without the host (NOTES R4.18).
  double *lv_u[2] = {nullptr, nullptr}, *lv_v[2] = {nullptr, nullptr}, *lv_l[2] = {nullptr, nullptr};
  int lv_n = 0, lv_cur = 0;
  bool lv_sorted = false;    // the current live set is the output of a merging turn: best first
  bool turn_lds_ok = false;  // this device lets payne_ns_turn_kernel have kTurnRowsLdsMax bytes of dynamic LDS (asked in payne_ns_queue_dev_init)
  double* dyn = nullptr;                  // device: {scale, loglstar}
  double* dq_host[2] = {nullptr, nullptr}; double* dq_host_dev[2] = {nullptr, nullptr};      // two mapped result blocks (+ flag word each)
  volatile unsigned long long* dq_flag[2] = {nullptr, nullptr}; unsigned long long* dq_flag_dev[2] = {nullptr, nullptr};
  unsigned long long dq_seq[2] = {0, 0};
  double* dax_host[2] = {nullptr, nullptr}; double* dax_host_dev[2] = {nullptr, nullptr};    // two mapped blocks for the bound
  int dq_launched = 0, dq_collected = 0, dq_exported = 0, dq_K = 0, dq_n_ell = 0, dax_n = 0;   // (exported: queues whose results' transfer is enqueued)
  std::vector<int> pk_src, pk_heap;       // payne_ns_rwalk_queue_turn: the live set its peek predicts, by index (payne_ns::peek_index)
  std::vector<double> pk_l;
  WalkTail* tail_dev = nullptr;           // the walk in progress as the post kernel's tail reads it (written by the launch that opens the walk)
  WalkState walk{};                       // the walk in progress
  bool queue_open = false; int queue_K = 0; void* queue_stream = nullptr;   // payne_ns_rwalk_queue_begin .. _end
  bool tail_done = false;                 // the last likelihood batch ran the next step at its tail
  long long n_tail = 0, n_own = 0;        // chain steps at the post kernel's tail / as launches of their own
  std::vector<void*> owned;
  // a walk in progress (payne_rwalk_begin / payne_rwalk_step)
  struct { double *u, *v, *lnprob; int K, walks; double scale, loglstar; unsigned long long seed; int *nacc, *ncall; void* stream; bool open; bool multi; int* nredraw; } run{};
  // a slice walk in progress (payne_slice_begin / payne_slice_rounds): the windows (left | right | axis), the chains' scalars
  // (phase | dir | attempt | nshrink) and the word the closing launch counts the unfinished chains in; its pinned landing place
  double* sl_win = nullptr; int* sl_int = nullptr; int* sl_active_host = nullptr;
  SliceState slice{};
  struct { bool open, pending, first; void* stream; } srun{};
  long long n_slice = 0;                  // slice rounds (launches of their own)
};

// (the queue's staging block -- q_dev, q_host, dq_host --: its regions, sizes and the words behind it are queue_block.hpp's)
namespace pq = payne_queue;
static int adv_on(const SamplerDev& sd) { return (sd.adv.imf || sd.adv.vrot || sd.adv.plx_dim >= 0) ? 1 : 0; }

// One allocation of the sampler's device memory, freed at destroy; `what` heads the message of a failure.
template <class T>
static int sampler_alloc(payne_sampler* s, size_t bytes, T** out, const char* what = "hipMalloc(sampler)") {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return ctx_fail(s->ctx, PAYNE_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  s->owned.push_back(p);
  *out = static_cast<T*>(p);
  return PAYNE_OK;
}

extern "C" void payne_sampler_destroy(payne_sampler* s) {
  if (!s) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ctx_view(s->ctx).device);
  for (void* p : s->owned) (void)hipFree(p);
  if (s->q_host) (void)hipHostFree(s->q_host);
  if (s->sl_active_host) (void)hipHostFree(s->sl_active_host);
  for (int b = 0; b < 2; ++b) { if (s->dq_host[b]) (void)hipHostFree(s->dq_host[b]); if (s->dax_host[b]) (void)hipHostFree(s->dax_host[b]); }
  (void)hipSetDevice(prev);
  delete s;
}

extern "C" int payne_sampler_create(payne_ctx* c, const payne_sampler_desc* d, int k_max, payne_sampler** out) {
  if (!c || !out) return PAYNE_E_INVALID;
  *out = nullptr;
  const CtxView cv = ctx_view(c);
  if (!d || d->ndim <= 0 || d->ndim > PAYNE_MAX_DIM) return ctx_fail(c, PAYNE_E_INVALID, "sampler.ndim out of range");
  if (d->n_fixed < 0 || d->n_fixed > PAYNE_MAX_FIXED) return ctx_fail(c, PAYNE_E_INVALID, "sampler.n_fixed out of range");
  if (k_max <= 0 || k_max > cv.b_max) return ctx_fail(c, PAYNE_E_INVALID, "sampler.k_max must be in 1..opts.b_max");
  for (int i = 0; i < d->ndim; ++i)
    if (d->dims[i].theta_col >= cv.ncols || d->dims[i].kind < 0 || d->dims[i].kind > PAYNE_PRIOR_TABLE)
      return ctx_fail(c, PAYNE_E_INVALID, "sampler dimension with bad theta_col / kind");
  for (int i = 0; i < d->n_fixed; ++i)
    if (d->fixed_col[i] < 0 || d->fixed_col[i] >= cv.ncols) return ctx_fail(c, PAYNE_E_INVALID, "fixed parameter with bad column");
  {
    const payne_adv_priors& a = d->adv;
    int ntab = 0;
    for (int i = 0; i < d->ndim; ++i) ntab += d->dims[i].kind == PAYNE_PRIOR_TABLE;
    if (ntab > 1 || (ntab == 1 && (!a.tab_cdf || !a.tab_val || a.tab_n < 2))) return ctx_fail(c, PAYNE_E_INVALID, "PAYNE_PRIOR_TABLE needs adv.tab_* (one table per sampler)");
    if (a.dim_logg >= d->ndim || a.dim_logr >= d->ndim || a.dim_vrot >= d->ndim || a.plx_dim >= d->ndim)
      return ctx_fail(c, PAYNE_E_INVALID, "adv.dim_* out of range");
  }
  int rc = ctx_on_device(c);
  if (rc) return rc;
  std::unique_ptr<payne_sampler, decltype(&payne_sampler_destroy)> owner(new payne_sampler(), payne_sampler_destroy);   // a failing exit frees once
  payne_sampler* const s = owner.get();
  s->ctx = c; s->k_max = k_max;
  s->sd.ndim = d->ndim; s->sd.ncols = cv.ncols; s->sd.nfixed = d->n_fixed;
  for (int i = 0; i < d->ndim; ++i) s->sd.dims[i] = d->dims[i];
  for (int i = 0; i < d->n_fixed; ++i) { s->sd.fixed_col[i] = d->fixed_col[i]; s->sd.fixed_val[i] = d->fixed_val[i]; }
  for (int k = 0; k < kMaxThetaCols; ++k) { s->sd.col_src[k] = -1; s->sd.col_val[k] = std::nan(""); }
  for (int i = 0; i < d->n_fixed; ++i) s->sd.col_val[d->fixed_col[i]] = d->fixed_val[i];
  for (int i = 0; i < d->ndim; ++i) if (d->dims[i].theta_col >= 0) s->sd.col_src[d->dims[i].theta_col] = i;
  s->sd.adv = d->adv;
  s->sd.adv.tab_cdf = nullptr; s->sd.adv.tab_val = nullptr;
  const size_t K = (size_t)k_max, nd = (size_t)d->ndim;
  if ((rc = sampler_alloc(s, K * nd * 8, &s->u_prop)) || (rc = sampler_alloc(s, K * nd * 8, &s->v_prop)) ||
      (rc = sampler_alloc(s, K * 8, &s->lnprior)) || (rc = sampler_alloc(s, K * 8, &s->lnl)) ||
      (rc = sampler_alloc(s, K * cv.ncols * 8, &s->rows)) || (rc = sampler_alloc(s, (size_t)PAYNE_MAX_ELL * nd * nd * 8, &s->axes)) ||
      (rc = sampler_alloc(s, K * 4, &s->inside)) || (rc = sampler_alloc(s, K * 4, &s->ell)) || (rc = sampler_alloc(s, K * 4, &s->nredraw)) ||
      (rc = sampler_alloc(s, std::max<size_t>(pq::capacity(K, nd), 2 * PAYNE_MAX_DIM) * 8, &s->q_dev)) ||
      (rc = sampler_alloc(s, sizeof(WalkTail), &s->tail_dev)) ||
      (rc = sampler_alloc(s, 3 * K * nd * 8, &s->sl_win)) || (rc = sampler_alloc(s, (4 * K + 1) * 4, &s->sl_int)) ||
      (spec_fits(d->ndim, cv.ncols) && (rc = sampler_alloc(s, K * 2 * kSpecStride * 8, &s->spec)))) return rc;
  if (d->adv.tab_cdf && d->adv.tab_val && d->adv.tab_n >= 2) {          // the tabulated inverse CDF (PAYNE_PRIOR_TABLE)
    double *tc = nullptr, *tv = nullptr;
    const size_t nb = (size_t)d->adv.tab_n * 8;
    if ((rc = sampler_alloc(s, nb, &tc)) || (rc = sampler_alloc(s, nb, &tv))) return rc;
    s->sd.adv.tab_cdf = tc; s->sd.adv.tab_val = tv;                     // (owned by the sampler from here on)
    if (hipMemcpy(tc, d->adv.tab_cdf, nb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tv, d->adv.tab_val, nb, hipMemcpyHostToDevice) != hipSuccess)
      return ctx_fail(c, PAYNE_E_HIP, "upload of the tabulated prior");
  }
  {   // the transforms' per-dimension constants, computed by the device functions the steps use (q_dev: staging, free here)
    double qh[2 * PAYNE_MAX_DIM];
    hipLaunchKernelGGL(payne_prior_cache_kernel, dim3(1), dim3(64), 0, nullptr, s->sd, s->q_dev);
    if (hipGetLastError() != hipSuccess || hipMemcpy(qh, s->q_dev, sizeof(qh), hipMemcpyDeviceToHost) != hipSuccess)
      return ctx_fail(c, PAYNE_E_HIP, "prior cache kernel");
    for (int i = 0; i < PAYNE_MAX_DIM; ++i) { s->sd.q0[i] = qh[i]; s->sd.q1[i] = qh[PAYNE_MAX_DIM + i]; }
  }
  // the descriptor as the post kernel's tail reads it: it never changes after this point, so it is published here, once (the launch
  // that opens a walk publishes the walk's own record only -- it used to copy these 4 KB too, by one thread, in front of every queue)
  if (hipMemcpy(&s->tail_dev->sd, &s->sd, sizeof(SamplerDev), hipMemcpyHostToDevice) != hipSuccess)
    return ctx_fail(c, PAYNE_E_HIP, "upload of the sampler descriptor");
  (void)hipMemset(s->inside, 0, K * 4);
  const pq::HostBlock qh = pq::q_host_block(K, nd);
  if (hipHostMalloc((void**)&s->q_host, qh.doubles * 8, hipHostMallocMapped) != hipSuccess ||
      hipHostMalloc((void**)&s->sl_active_host, 8, hipHostMallocDefault) != hipSuccess)
    return ctx_fail(c, PAYNE_E_HIP, "hipHostMalloc(sampler staging)");
  {                                                          // (no device address for the block: hipMemcpyAsync + hipStreamSynchronize)
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, s->q_host, 0) == hipSuccess && dp) {
      s->q_host_dev = static_cast<double*>(dp);
      s->q_flag = reinterpret_cast<volatile unsigned long long*>(s->q_host + qh.flag);
      s->q_flag_dev = reinterpret_cast<unsigned long long*>(s->q_host_dev + qh.flag);
      *s->q_flag = 0ull;
      void* ap = nullptr;
      if (hipMalloc(&ap, 8) == hipSuccess && hipMemset(ap, 0, 8) == hipSuccess) { s->owned.push_back(ap); s->q_arrivals = static_cast<unsigned*>(ap); }
    }
  }
  *out = owner.release();
  return PAYNE_OK;
}

static int sampler_check(payne_sampler* s, const void* a, int K, const void* b) {
  if (!s) return PAYNE_E_INVALID;
  payne_ctx* c = s->ctx;
  if (!a || !b) return ctx_fail(c, PAYNE_E_INVALID, "NULL input/output pointer");
  if (K <= 0 || K > s->k_max) return ctx_fail(c, PAYNE_E_BATCH, "K exceeds the sampler's k_max");
  return ctx_on_device(c);
}

extern "C" int payne_prior_transform_batch(payne_sampler* s, const double* u, int K, double* v, void* stream) {
  int rc = sampler_check(s, u, K, v);
  if (rc) return rc;
  hipLaunchKernelGGL(payne_prior_kernel, dim3((K + 127) / 128), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), s->sd, u, K,
                     v, (double*)nullptr, (double*)nullptr, 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(s->ctx, PAYNE_E_HIP, std::string("prior launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}

extern "C" int payne_lnprob_u_batch(payne_sampler* s, const double* u, int K, double* v, double* lnprob, void* stream) {
  int rc = sampler_check(s, u, K, v);
  if (rc) return rc;
  if (!lnprob) return ctx_fail(s->ctx, PAYNE_E_INVALID, "lnprob is NULL");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(payne_prior_kernel, dim3((K + 127) / 128), dim3(128), 0, st, s->sd, u, K, v, s->lnprior, s->rows, 1);
  if ((rc = payne_lnlike_batch(s->ctx, s->rows, K, s->lnl, stream))) return rc;
  hipLaunchKernelGGL(payne_lnprob_kernel, dim3((K + 127) / 128), dim3(128), 0, st, s->lnprior, s->lnl, K, lnprob);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(s->ctx, PAYNE_E_HIP, std::string("lnprob launch: ") + hipGetErrorString(e));
  return PAYNE_OK;
}

// The walk in two parts, so that a caller can interleave the steps of several samplers (one context and
// one HIP stream each) from one host thread: two independent batches in flight fill the idle time a single
// chain of dependent launches leaves (13.6 M against 10.6 M evaluations/s at 512 x 4096 pixels).
// (the walk's counters -- nacc, ncall, nredraw -- are zeroed by its first step: payne_rwalk_kernel with settle = 0)
static void rwalk_begin_impl(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes_dev, const int* ell_dev,
                             double scale, double loglstar, int walks, unsigned long long seed, int* nacc, int* ncall, int* nredraw,
                             void* stream) {
  s->run = {u, v, lnprob, K, walks, scale, loglstar, seed, nacc, ncall, stream, true, ell_dev != nullptr, nredraw};
  s->walk = WalkState{u, v, lnprob, nacc, ncall, s->u_prop, s->v_prop, s->lnprior, s->inside, s->rows, axes_dev,
                      ell_dev, nredraw, scale, loglstar, seed, K,
                      s->sd.ndim, s->sd.ncols, adv_on(s->sd), s->spec,
                      nullptr, nullptr, nullptr, 0, nullptr};
  s->tail_done = false;
}
extern "C" int payne_rwalk_begin_ell(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes,
                                     int n_ell, const int* ell, double scale, double loglstar, int walks,
                                     unsigned long long seed, int* nacc, int* ncall, void* stream) {
  int rc = sampler_check(s, u, K, v);
  if (rc) return rc;
  if (!lnprob || !axes || !nacc || !ncall || walks <= 0) return ctx_fail(s->ctx, PAYNE_E_INVALID, "bad rwalk arguments");
  if (s->srun.open) return ctx_fail(s->ctx, PAYNE_E_INVALID, "a slice walk is open on this sampler");
  if (const char* bad = pq::check_ell_list(n_ell, ell != nullptr, ell, K)) return ctx_fail(s->ctx, PAYNE_E_INVALID, bad);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nd = s->sd.ndim;
  HIPCHK(s->ctx, hipMemcpyAsync(s->axes, axes, (size_t)n_ell * nd * nd * 8, hipMemcpyHostToDevice, st));
  if (ell) HIPCHK(s->ctx, hipMemcpyAsync(s->ell, ell, (size_t)K * 4, hipMemcpyHostToDevice, st));
  rwalk_begin_impl(s, u, v, lnprob, K, s->axes, ell ? s->ell : (const int*)nullptr, scale, loglstar, walks, seed, nacc, ncall, s->nredraw, stream);
  return PAYNE_OK;
}
extern "C" int payne_rwalk_begin(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes,
                                 double scale, double loglstar, int walks, unsigned long long seed, int* nacc, int* ncall,
                                 void* stream) {
  return payne_rwalk_begin_ell(s, u, v, lnprob, K, axes, 1, nullptr, scale, loglstar, walks, seed, nacc, ncall, stream);
}
// step w = 0 .. walks: settle proposal w-1, draw proposal w and evaluate it (the last step only settles)
extern "C" int payne_rwalk_step(payne_sampler* s, int w) {
  if (!s || !s->ctx) return PAYNE_E_INVALID;
  if (!s->run.open || w < 0 || w > s->run.walks) return ctx_fail(s->ctx, PAYNE_E_INVALID, "payne_rwalk_step outside a walk");
  const auto& r = s->run;
  hipStream_t st = reinterpret_cast<hipStream_t>(r.stream);
  // step w: settle proposal w-1, draw proposal w -- unless the previous likelihood batch already did it at its tail
  if (s->tail_done) s->n_tail += 1;
  else {
    s->n_own += 1;
    const dim3 grid((r.K + 3) / 4), block(256);                // one wave per chain
    hipLaunchKernelGGL(payne_rwalk_kernel, grid, block, 0, st, s->sd, s->walk, s->lnl, w, w > 0 ? 1 : 0, w < r.walks ? 1 : 0,
                       w == 0 ? s->tail_dev : (WalkTail*)nullptr);
  }
  s->tail_done = false;
  int rc = PAYNE_OK;
  if (w < r.walks) {
    TailReq tr{s->tail_dev, w + 1, w + 1 < r.walks ? 1 : 0, false, s->spec ? &s->walk : nullptr};
    rc = ctx_lnlike(s->ctx, s->rows, r.K, s->lnl, r.stream, &tr);
    s->tail_done = tr.done;
  } else s->run.open = false;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(s->ctx, PAYNE_E_HIP, std::string("rwalk launch: ") + hipGetErrorString(e));
  return rc;
}
static int rwalk_steps(payne_sampler* s, int walks) {
  int rc = PAYNE_OK;
  for (int w = 0; !rc && w <= walks; ++w) rc = payne_rwalk_step(s, w);
  return rc;
}
extern "C" int payne_sampler_counters(const payne_sampler* s, long long out[2]) {
  if (!s || !out) return PAYNE_E_INVALID;
  out[0] = s->n_tail; out[1] = s->n_own + s->n_slice;
  return PAYNE_OK;
}
extern "C" int payne_rwalk_batch(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes,
                                 double scale, double loglstar, int walks, unsigned long long seed, int* nacc, int* ncall,
                                 void* stream) {
  const int rc = payne_rwalk_begin(s, u, v, lnprob, K, axes, scale, loglstar, walks, seed, nacc, ncall, stream);
  return rc ? rc : rwalk_steps(s, walks);
}

// Slice sampling as lock-step chains on the device (header: payne_slice_begin).  A round is payne_slice_kernel -- settle the value
// that came back, go on to the chain's next in-cube point -- and one likelihood batch over the rows it wrote; the host enqueues
// rounds and reads ONE word per call (the chains not finished), nothing per chain.
extern "C" int payne_slice_begin(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes, int n_ell,
                                 const int* ell, double scale, double loglstar, int slices, int random_dirs,
                                 unsigned long long seed, int* ncall, int* nexpand, int* ncontract, void* stream) {
  int rc = sampler_check(s, u, K, v);
  if (rc) return rc;
  payne_ctx* c = s->ctx;
  if (!lnprob || !axes || !ncall || !nexpand || !ncontract) return ctx_fail(c, PAYNE_E_INVALID, "bad slice arguments");
  if (slices <= 0) return ctx_fail(c, PAYNE_E_INVALID, "slices must be > 0");
  if (const char* bad = pq::check_ell_list(n_ell, ell != nullptr, ell, K)) return ctx_fail(c, PAYNE_E_INVALID, bad);
  if (s->run.open || s->queue_open || s->dq_launched != s->dq_collected)
    return ctx_fail(c, PAYNE_E_INVALID, "a random walk is open on this sampler");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nd = s->sd.ndim;
  HIPCHK(c, hipMemcpyAsync(s->axes, axes, (size_t)n_ell * nd * nd * 8, hipMemcpyHostToDevice, st));
  if (ell) HIPCHK(c, hipMemcpyAsync(s->ell, ell, (size_t)K * 4, hipMemcpyHostToDevice, st));
  const size_t kn = (size_t)s->k_max * nd, km = (size_t)s->k_max;
  s->slice = SliceState{u, v, lnprob, s->sl_win, s->sl_win + kn, s->sl_win + 2 * kn,
                        s->sl_int, s->sl_int + km, s->sl_int + 2 * km, s->sl_int + 3 * km, ncall, nexpand, ncontract,
                        s->u_prop, s->v_prop, s->lnprior, s->inside, s->rows, s->axes, ell ? s->ell : (const int*)nullptr,
                        s->sl_int + 4 * km, scale, loglstar, seed, K, nd, s->sd.ncols,
                        adv_on(s->sd),
                        random_dirs ? slices : slices * nd, random_dirs ? 1 : 0};
  s->srun = {true, false, true, stream};
  return PAYNE_OK;
}
extern "C" int payne_slice_rounds(payne_sampler* s, int n, int* n_active) {
  if (!s || !s->ctx) return PAYNE_E_INVALID;
  payne_ctx* c = s->ctx;
  if (!s->srun.open) return ctx_fail(c, PAYNE_E_INVALID, "payne_slice_rounds outside a walk");
  if (n <= 0 || !n_active) return ctx_fail(c, PAYNE_E_INVALID, "bad payne_slice_rounds arguments");
  int rc = ctx_on_device(c);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(s->srun.stream);
  const int K = s->slice.K;
  const dim3 grid((K + 3) / 4), block(256);                     // one wave per chain
  for (int r = 0; r < n && !rc; ++r) {
    hipLaunchKernelGGL(payne_slice_kernel, grid, block, 0, st, s->sd, s->slice, s->lnl, s->srun.pending ? 1 : 0, 1, s->srun.first ? 1 : 0);
    s->srun.pending = true; s->srun.first = false;
    s->n_slice += 1;
    rc = ctx_lnlike(c, s->rows, K, s->lnl, s->srun.stream, nullptr);
  }
  if (rc) { s->srun.open = false; return rc; }
  // the closing launch settles what is pending and counts the chains that have not finished: one word for the host
  hipLaunchKernelGGL(payne_slice_kernel, grid, block, 0, st, s->sd, s->slice, s->lnl, 1, 0, 0);
  s->srun.pending = false;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(s->sl_active_host, s->slice.n_active, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { s->srun.open = false; return ctx_fail(c, PAYNE_E_HIP, std::string("slice rounds: ") + hipGetErrorString(e)); }
  *n_active = *s->sl_active_host;
  if (*n_active == 0) s->srun.open = false;
  return PAYNE_OK;
}
extern "C" int payne_slice_batch(payne_sampler* s, double* u, double* v, double* lnprob, int K, const double* axes, int n_ell,
                                 const int* ell, double scale, double loglstar, int slices, int random_dirs,
                                 unsigned long long seed, int* ncall, int* nexpand, int* ncontract, void* stream, int chunk,
                                 int max_rounds, int* n_active) {
  if (s && (chunk <= 0 || max_rounds <= 0 || !n_active)) return ctx_fail(s->ctx, PAYNE_E_INVALID, "bad payne_slice_batch arguments");
  int rc = payne_slice_begin(s, u, v, lnprob, K, axes, n_ell, ell, scale, loglstar, slices, random_dirs, seed, ncall, nexpand,
                             ncontract, stream);
  if (rc) return rc;
  *n_active = K;
  for (int done = 0; !rc && *n_active > 0 && done < max_rounds; ) {
    const int n = std::min(chunk, max_rounds - done);
    rc = payne_slice_rounds(s, n, n_active);
    done += n;
  }
  s->srun.open = false;                                         // (max_rounds reached: the unfinished chains stay where they are)
  return rc;
}

// The walk opened on the queue's device block as L lays it out, and its walks + 1 steps enqueued (dyn: the {scale, loglstar} the
// turn kernel left on the device, or null: the ones given here)
static int queue_walk(payne_sampler* s, const pq::Layout& L, double scale, double loglstar, int walks, unsigned long long seed,
                      const double* dyn, void* stream) {
  const pq::View q = L.view(s->q_dev);                      // (q.ell: device only, written by the first step)
  rwalk_begin_impl(s, q.u, q.v, q.lnprob, (int)L.K, q.axes, q.ell, scale, loglstar, walks, seed, q.nacc, q.ncall, q.nredraw, stream);
  s->walk.dyn = dyn;
  if (L.n_ell > 1) { s->walk.as_ctr = q.ctr; s->walk.as_ainv = q.ainv; s->walk.ell_out = q.ell; s->walk.n_ell = (int)L.n_ell; }
  return rwalk_steps(s, walks);
}
// The random-walk queue of the batched nested sampler in one call: start points, ellipsoid assignment, upload, the walk,
// download, and the chains that moved as the proposal queue (header: payne_ns_rwalk_queue).
// In two parts, so that the caller's host work (the next bound, bookkeeping of another fit) can run while the GPU walks:
// _begin returns once everything is enqueued (start points, ellipsoid assignment, upload, walks + 1 steps, download requests),
// _end waits for the stream and selects the chains that moved.  payne_ns_rwalk_queue is the two back to back.
// `src` (payne_ns_rwalk_queue_turn): live slot i holds row src[i] of (qu, qv) with lnprob lg[i] when src[i] >= 0 -- the live set a
// queue's consumption will leave, by index (payne_ns::peek_index), never copied
static int queue_begin_core(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl,
                            int nlive, int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv,
                            double scale, double loglstar, int walks, unsigned long long seed, void* stream,
                            const int* src, const double* qu, const double* qv, const double* lg) {
  int rc = sampler_check(s, live_u, K, live_v);
  if (rc) return rc;
  payne_ctx* c = s->ctx;
  if (s->queue_open) {
    // a queue begun and never collected (an abandoned generator, a caller of _begin that skipped _end): its transfer DOWN into
    // q_host may still be pending on its stream and would land on top of the start points written below -- wait for it first
    HIPCHK(c, hipStreamSynchronize(reinterpret_cast<hipStream_t>(s->queue_stream)));
  }
  s->queue_open = false;
  if (!live_logl || !axes_unit || nlive <= 0 || walks <= 0)
    return ctx_fail(c, PAYNE_E_INVALID, "bad payne_ns_rwalk_queue arguments");
  if (const char* bad = pq::check_ell_list(n_ell, ctr && ainv)) return ctx_fail(c, PAYNE_E_INVALID, bad);
  const pq::Layout L(K, s->sd.ndim, n_ell);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  pq::fill_starts(L, s->q_host, seed, nlive, live_u, live_v, live_logl, src, qu, qv, lg);
  // one transfer each way: chains, axes and (several ellipsoids) centres and inverse axes up; chains, then the three counters down
  pq::pack_bound(L, L.view(s->q_host).axes, axes_unit, ctr, ainv);
  if (s->q_host_dev) {
    const size_t n_up = L.n_up();
    hipLaunchKernelGGL(payne_stage_in_kernel, dim3((unsigned)((n_up + 1023) / 1024)), dim3(256), 0, st, s->q_dev, s->q_host_dev, n_up);
  } else {
    HIPCHK(c, hipMemcpyAsync(s->q_dev, s->q_host, L.n_up() * 8, hipMemcpyHostToDevice, st));
  }
  if ((rc = queue_walk(s, L, scale, loglstar, walks, seed, nullptr, stream))) return rc;
  if (s->q_host_dev) {
    ++s->q_seq;
    hipLaunchKernelGGL(payne_stage_out_kernel, dim3(s->q_arrivals ? 8 : 1), dim3(1024), 0, st, s->q_host_dev, s->q_dev, L.n_down(), s->q_flag_dev, s->q_seq,
                       (const double*)nullptr, 0, s->q_arrivals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ctx_fail(c, PAYNE_E_HIP, std::string("queue staging launch: ") + hipGetErrorString(e));
  } else {
    HIPCHK(c, hipMemcpyAsync(s->q_host, s->q_dev, L.n_down() * 8, hipMemcpyDeviceToHost, st));
  }
  s->queue_open = true; s->queue_K = K; s->queue_stream = stream;
  return PAYNE_OK;
}
extern "C" int payne_ns_rwalk_queue_begin(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl,
                                          int nlive, int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv,
                                          double scale, double loglstar, int walks, unsigned long long seed, void* stream) {
  return queue_begin_core(s, live_u, live_v, live_logl, nlive, K, axes_unit, n_ell, ctr, ainv, scale, loglstar, walks, seed, stream,
                          nullptr, nullptr, nullptr, nullptr);
}
static bool wait_word(volatile unsigned long long* w, unsigned long long want, double seconds) {
  // Spin while the wait is as long as queues have been taking (1.5 x the wait before: a C2 queue is ~1 ms, and a timer's wake-up
  // after a 50 us sleep cost the host-turn loop 50-100 us a collect when queues ran just over a fixed 1 ms window), at least one
  // millisecond; beyond that give the core away between looks -- a queue of 65 536-pixel spectra takes seconds, which one host
  // core used to burn: first by yielding, from 20 ms on by sleeping.
  static thread_local double last_wait = 1e-3;
  const double spin_for = std::min(20e-3, std::max(1e-3, 1.5 * last_wait));
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  int polite = 0;                                            // 0 spin | 1 yield | 2 sleep
  double dt = 0.0;
  bool ok = true;
  while (__atomic_load_n(const_cast<const unsigned long long*>(w), __ATOMIC_ACQUIRE) != want) {
    if (polite == 2) std::this_thread::sleep_for(std::chrono::microseconds(50));
    else if (polite == 1) std::this_thread::yield();
    if (polite || (++spins & 0x3FFu) == 0) {
      dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (dt > seconds) { ok = false; break; }
      polite = dt > 20e-3 ? 2 : (dt > spin_for ? 1 : 0);
    }
  }
  if (ok) {
    dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    last_wait = 0.5 * last_wait + 0.5 * dt;
  }
  return ok;
}
extern "C" int payne_ns_rwalk_queue_end(payne_sampler* s, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats) {
  if (!s) return PAYNE_E_INVALID;
  payne_ctx* c = s->ctx;
  if (!s->queue_open) return ctx_fail(c, PAYNE_E_INVALID, "payne_ns_rwalk_queue_end without a queue in flight");
  if (!qu || !qv || !ql || !qnc || !nq || !stats) return ctx_fail(c, PAYNE_E_INVALID, "bad payne_ns_rwalk_queue_end arguments");
  s->queue_open = false;
  const int K = s->queue_K, nd = s->sd.ndim;
  hipStream_t st = reinterpret_cast<hipStream_t>(s->queue_stream);
  const double* hu = s->q_host;
  if (s->q_flag) {
    // the word the queue's last kernel writes behind its results (every kernel before it on the stream has completed by then);
    // a queue that does not report within 10 s is handed to hipStreamSynchronize, which returns the fault if there was one
    if (!wait_word(s->q_flag, s->q_seq, 10.0)) HIPCHK(c, hipStreamSynchronize(st));
  } else {
    HIPCHK(c, hipStreamSynchronize(st));
  }
  pq::queue_extract(hu, K, nd, qu, qv, ql, qnc, nq, stats);
  return PAYNE_OK;
}
// ---- the queue's turn on the device: host entry points (header: payne_ns_queue_dev_*) ------------------------------------------
extern "C" int payne_ns_queue_dev_init(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl, int nlive,
                                       double scale, double loglstar) {
  if (!s) return PAYNE_E_INVALID;
  payne_ctx* c = s->ctx;
  if (!live_u || !live_v || !live_logl || nlive <= 0) return ctx_fail(c, PAYNE_E_INVALID, "bad payne_ns_queue_dev_init arguments");
  if (!s->q_host_dev) return ctx_fail(c, PAYNE_E_UNSUPPORTED, "the device-side turn needs the mapped staging block");
  if (s->dq_launched != s->dq_collected) return ctx_fail(c, PAYNE_E_INVALID, "payne_ns_queue_dev_init with queues in flight");
  const int nd = s->sd.ndim, K = s->k_max;
  if (nlive + K > 2048) return ctx_fail(c, PAYNE_E_UNSUPPORTED, "nlive + queue size > 2048");
  int rc = ctx_on_device(c);
  if (rc) return rc;
  if (nlive != s->lv_n) {
    for (int b = 0; b < 2; ++b)                              // (the messages: those of the HIPCHK lines these were)
      if ((rc = sampler_alloc(s, (size_t)nlive * nd * 8, &s->lv_u[b], "hipMalloc(&p, (size_t)nlive * nd * 8)")) ||
          (rc = sampler_alloc(s, (size_t)nlive * nd * 8, &s->lv_v[b], "hipMalloc(&p, (size_t)nlive * nd * 8)")) ||
          (rc = sampler_alloc(s, (size_t)nlive * 8, &s->lv_l[b], "hipMalloc(&p, (size_t)nlive * 8)"))) return rc;
    s->lv_n = nlive;
  }
  if (!s->dyn && (rc = sampler_alloc(s, 4 * 8, &s->dyn, "hipMalloc(&p, 4 * 8)"))) return rc;
  const pq::HostBlock blk = pq::dq_host_block(K, nd);
  for (int b = 0; b < 2; ++b) {
    if (!s->dq_host[b]) {
      HIPCHK(c, hipHostMalloc((void**)&s->dq_host[b], blk.doubles * 8, hipHostMallocMapped));
      void* dp = nullptr;
      HIPCHK(c, hipHostGetDevicePointer(&dp, s->dq_host[b], 0));
      s->dq_host_dev[b] = static_cast<double*>(dp);
      s->dq_flag[b] = reinterpret_cast<volatile unsigned long long*>(s->dq_host[b] + blk.flag);
      s->dq_flag_dev[b] = reinterpret_cast<unsigned long long*>(s->dq_host_dev[b] + blk.flag);
      s->dax_n = (int)pq::bound_capacity(nd);
      HIPCHK(c, hipHostMalloc((void**)&s->dax_host[b], (size_t)s->dax_n * 8, hipHostMallocMapped));
      HIPCHK(c, hipHostGetDevicePointer(&dp, s->dax_host[b], 0));
      s->dax_host_dev[b] = static_cast<double*>(dp);
    }
    *s->dq_flag[b] = 0ull;
    s->dq_seq[b] = 0;
  }
  HIPCHK(c, hipMemcpy(s->lv_u[0], live_u, (size_t)nlive * nd * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(s->lv_v[0], live_v, (size_t)nlive * nd * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(s->lv_l[0], live_logl, (size_t)nlive * 8, hipMemcpyHostToDevice));
  const double d2[4] = {scale, loglstar, 0.0, 0.0};
  HIPCHK(c, hipMemcpy(s->dyn, d2, sizeof(d2), hipMemcpyHostToDevice));
  // (a function attribute belongs to the device it was set on: asked here, with the sampler's device current, not once per process)
  s->turn_lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(payne_ns_turn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kTurnRowsLdsMax) == hipSuccess;
  s->lv_cur = 0; s->lv_sorted = false; s->dq_launched = 0; s->dq_collected = 0; s->dq_exported = 0; s->dq_n_ell = 0;
  return PAYNE_OK;
}
extern "C" int payne_ns_queue_dev_launch(payne_sampler* s, int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv,
                                         int walks, unsigned long long seed, int merge, void* stream) {
  if (!s) return PAYNE_E_INVALID;
  payne_ctx* c = s->ctx;
  if (s->lv_n <= 0 || !s->dyn) return ctx_fail(c, PAYNE_E_INVALID, "payne_ns_queue_dev_launch before payne_ns_queue_dev_init");
  if (K <= 0 || K > s->k_max || walks <= 0) return ctx_fail(c, PAYNE_E_INVALID, "bad payne_ns_queue_dev_launch arguments");
  if (s->dq_launched - s->dq_collected >= 2) return ctx_fail(c, PAYNE_E_INVALID, "two queues already in flight");
  if (s->dq_launched != s->dq_collected && K != s->dq_K) return ctx_fail(c, PAYNE_E_INVALID, "queue size changed with a queue in flight");
  if (s->queue_open) return ctx_fail(c, PAYNE_E_INVALID, "a host-turn queue is in flight");
  if (axes_unit) {
    if (const char* bad = pq::check_ell_list(n_ell, ctr && ainv)) return ctx_fail(c, PAYNE_E_INVALID, bad);
  } else {
    n_ell = s->dq_n_ell;
    if (n_ell < 1) return ctx_fail(c, PAYNE_E_INVALID, "no bound on the device yet");
  }
  int rc = ctx_on_device(c);
  if (rc) return rc;
  const int nd = s->sd.ndim, nl = s->lv_n, b = s->dq_launched & 1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const pq::Layout L(K, nd, n_ell);
  const pq::View q = L.view(s->q_dev);
  if (axes_unit) {                                          // a new bound: up through its own mapped block (two, used in turn)
    pq::pack_bound(L, s->dax_host[b], axes_unit, ctr, ainv);
    s->dq_n_ell = n_ell;
  }
  TurnArgs ta{};
  ta.ax_src = s->dyn; ta.ax_dst = nullptr; ta.ax_n = 0;
  if (axes_unit) { ta.ax_src = s->dax_host_dev[b]; ta.ax_dst = q.axes; ta.ax_n = (int)L.n_bound(); }   // (up with the turn kernel)
  const int cur = s->lv_cur, nxt = merge ? cur ^ 1 : cur;
  ta.lu = s->lv_u[cur]; ta.lv = s->lv_v[cur]; ta.ll = s->lv_l[cur];
  ta.ou = s->lv_u[nxt]; ta.ov = s->lv_v[nxt]; ta.ol = s->lv_l[nxt];
  ta.nlive = nl; ta.nd = nd; ta.K = K; ta.merge = merge ? 1 : 0;
  int n2 = 2;
  while (n2 < nl + K) n2 <<= 1;
  ta.n2 = n2;
  ta.cu = q.u; ta.cv = q.v; ta.cl = q.lnprob; ta.na = q.nacc; ta.nc = q.ncall; ta.nr = q.nredraw;
  ta.dyn = s->dyn; ta.scale0 = 0.0; ta.lstar0 = 0.0; ta.seed = seed;
  if (s->dq_launched > s->dq_exported) {                    // the queue before this one: its results leave with this turn
    const int pb = s->dq_exported & 1;
    ta.exp_dst = s->dq_host_dev[pb]; ta.exp_n = (int)L.n_down();
    ta.exp_flag = s->dq_flag_dev[pb];
    ta.exp_seq = ++s->dq_seq[pb];
    ++s->dq_exported;
  }
  if (!merge) {                                             // the values payne_ns_queue_dev_init left stay
    double d2[2];
    HIPCHK(c, hipMemcpy(d2, s->dyn, sizeof(d2), hipMemcpyDeviceToHost));
    ta.scale0 = d2[0]; ta.lstar0 = d2[1];
  }
  size_t rows_bytes = (size_t)nl * nd * 16;
  if (rows_bytes > kTurnRowsLdsMax || !s->turn_lds_ok) rows_bytes = 0;
  ta.rows_lds = rows_bytes ? 1 : 0;
  ta.live_sorted = s->lv_sorted ? 1 : 0;
  if (merge) s->lv_sorted = true;
  hipLaunchKernelGGL(payne_ns_turn_kernel, dim3(1), dim3(1024), rows_bytes, st, ta);
  s->lv_cur = nxt;
  if ((rc = queue_walk(s, L, 0.0, 0.0, walks, seed, s->dyn, stream))) return rc;
  // (its results: with the NEXT queue's turn, or by payne_ns_queue_dev_collect when none has been launched by then)
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx_fail(c, PAYNE_E_HIP, std::string("device-turn launch: ") + hipGetErrorString(e));
  ++s->dq_launched; s->dq_K = K; s->queue_stream = stream;
  return PAYNE_OK;
}
extern "C" int payne_ns_queue_dev_collect(payne_sampler* s, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats,
                                          double* dyn_used) {
  if (!s) return PAYNE_E_INVALID;
  payne_ctx* c = s->ctx;
  if (s->dq_collected >= s->dq_launched) return ctx_fail(c, PAYNE_E_INVALID, "payne_ns_queue_dev_collect without a queue in flight");
  if (!qu || !qv || !ql || !qnc || !nq || !stats) return ctx_fail(c, PAYNE_E_INVALID, "bad payne_ns_queue_dev_collect arguments");
  const int b = s->dq_collected & 1, K = s->dq_K, nd = s->sd.ndim;
  const pq::Layout L(K, nd, 1);                             // (what comes down lies in front of the bound)
  if (s->dq_exported <= s->dq_collected) {                  // the newest queue, no turn behind it: a transfer of its own
    ++s->dq_seq[b];
    hipLaunchKernelGGL(payne_stage_out_kernel, dim3(s->q_arrivals ? 8 : 1), dim3(1024), 0, reinterpret_cast<hipStream_t>(s->queue_stream),
                       s->dq_host_dev[b], s->q_dev, L.n_down(), s->dq_flag_dev[b], s->dq_seq[b], s->dyn, 2, s->q_arrivals);
    ++s->dq_exported;
  }
  volatile unsigned long long* flag = s->dq_flag[b];
  if (!wait_word(flag, s->dq_seq[b], 10.0)) {
    HIPCHK(c, hipStreamSynchronize(reinterpret_cast<hipStream_t>(s->queue_stream)));
    if (*flag != s->dq_seq[b]) return ctx_fail(c, PAYNE_E_HIP, "the queue's completion word never arrived");
  }
  pq::queue_extract(s->dq_host[b], K, nd, qu, qv, ql, qnc, nq, stats);
  if (dyn_used) { dyn_used[0] = s->dq_host[b][L.dyn_pair()]; dyn_used[1] = s->dq_host[b][L.dyn_pair() + 1]; }
  ++s->dq_collected;
  return PAYNE_OK;
}
// One turn of the sampler's pipelined loop in ONE call: collect the queue in flight (_end), adapt the step scale to its acceptance
// (dynesty's rule, as thepayne_amd/sampler/nested.py applies it), predict the live set and threshold its consumption will leave
// (payne_ns_peek) and launch the next queue from there (_begin) -- between a queue's last transfer and the next one's first
// kernel the GPU idles, and every microsecond of interpreter there is one of those.
extern "C" int payne_ns_rwalk_queue_turn(payne_sampler* s, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats,
                                         const double* live_u, const double* live_v, const double* live_logl, int nlive, int K,
                                         const double* axes_unit, int n_ell, const double* ctr, const double* ainv, double* scale,
                                         double* loglstar, int walks, unsigned long long seed, int* n_dead) {
  if (!s) return PAYNE_E_INVALID;
  if (!scale || !loglstar || !n_dead || !live_u || !live_v || !live_logl || nlive <= 0) return ctx_fail(s->ctx, PAYNE_E_INVALID, "bad payne_ns_rwalk_queue_turn arguments");
  void* stream = s->queue_stream;
  int rc = payne_ns_rwalk_queue_end(s, qu, qv, ql, qnc, nq, stats);
  if (rc) return rc;
  *scale = pq::adapt_scale(*scale, stats, s->sd.ndim);
  payne_ns::peek_index(nlive, live_logl, ql, *nq, s->pk_src, s->pk_l, s->pk_heap, loglstar, n_dead);
  return queue_begin_core(s, live_u, live_v, live_logl, nlive, K, axes_unit, n_ell, ctr, ainv, *scale, *loglstar, walks, seed, stream,
                          s->pk_src.data(), qu, qv, s->pk_l.data());
}
extern "C" int payne_ns_rwalk_queue(payne_sampler* s, const double* live_u, const double* live_v, const double* live_logl,
                                    int nlive, int K, const double* axes_unit, int n_ell, const double* ctr, const double* ainv,
                                    double scale, double loglstar, int walks, unsigned long long seed, double* qu, double* qv,
                                    double* ql, int* qnc, int* nq, long long* stats, void* stream) {
  if (s && (!qu || !qv || !ql || !qnc || !nq || !stats)) return ctx_fail(s->ctx, PAYNE_E_INVALID, "bad payne_ns_rwalk_queue arguments");
  const int rc = payne_ns_rwalk_queue_begin(s, live_u, live_v, live_logl, nlive, K, axes_unit, n_ell, ctr, ainv, scale, loglstar,
                                            walks, seed, stream);
  return rc ? rc : payne_ns_rwalk_queue_end(s, qu, qv, ql, qnc, nq, stats);
}
