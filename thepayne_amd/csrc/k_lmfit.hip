// k_lmfit.hip -- payne_lmfit_*: batched Levenberg-Marquardt (include/payne_hip.h).  The arithmetic is lmfit_core.hpp, which runs on
// the host too (tests/emul/lmfit_emul.cpp, lmfit_poly_emul.cpp, lmfit_phot_emul.cpp); the tile, its loop and the 16-byte loads are normal_tile.hpp.
//
//   payne_lmfit_update_kernel  one 256-thread workgroup a star, skipped when the star is no longer RUNNING.  Lane (i = lane & 15,
//     q = lane >> 4) of every wave reads four consecutive fp32 pixels of row i of R and the four fp64 weights and hands them to
//     normal_tile.hpp's loop (wave_sums); the four partial tiles meet in LDS (sum_waves).  Thread 0 then takes the star's step
//     (lmfit_core.hpp: update_star) on LDS and the handle's arrays.  <VEC>: 16-byte loads (ld, ld_f multiples of four, aligned
//     pointers); otherwise element by element, the same values in the same places.
//       <POLY = false>  payne_lmfit_update: R = [rows 1..K ; flux - row 0].  The kernel streams (1 + K) n fp32 + n fp32 + n fp64 per
//         star once and is bound by HBM; the matrix instruction takes the (K + 1)^2 / 2 products a pixel off the vector pipeline,
//         which would otherwise bind it for K >= 4.
//       <POLY = true>   payne_lmfit_update_poly: a model times a Chebyshev series whose P coefficients are the last P of the K
//         parameters.  R = [p dm/dtheta ; m T_j(x) ; flux - m p] is formed in registers from the caller's 1 + Km rows, the star's
//         coefficients (x_trial, copied to LDS) and x, and never stored.  Every lane evaluates one series at its four pixels in one
//         loop of P - 2 steps (cheb_series.hpp: series4): p, or T_j as the series of a unit vector.
//   payne_lmfit_update_phot_kernel  payne_lmfit_update_phot: the same body (update_body<VEC, POLY, PHOT = true>) for a spectrum and
//     magnitudes fitted together.  K = Km + Kp + P: the lanes of rows Km .. Km + Kp - 1, the parameters only the photometry sees, are
//     not live.  Every thread asks for up to two of the star's F ncol <= 448 derivatives (and thread f for filter f's weight and
//     residual) before the pixel loop and keeps them in registers; behind sum_waves they go to LDS (the space of `part`), thread
//     (i, j) sums element (i, j) of the photometric block over the filters in ascending order (lmfit_phot_core.hpp: phot_element),
//     and thread 0 adds the priors and the block to the tile (add_block) before it takes the step.
//   payne_lmfit_update_pair_kernel  payne_lmfit_update_pair: two components with a light ratio q times a Chebyshev series, K = Kl + 1 + P
//     (lmfit_pair_core.hpp).  A body of its own (update_pair_body), so that the kernels above keep their code: the same tile, loop and
//     step.  Every lane reads one row of A's block and one of B's (row 0, the model, where it has no derivative; nothing where the map
//     says -1), mixes them with (1 - q, q), or (-1, 1) in the ratio's row, and multiplies by its series; q and the coefficients come
//     from x_trial through LDS.  It streams (2 + Ka + Kb) n fp32 + n fp32 + n fp64 per star once; nothing of R is stored.
//   payne_lmfit_begin_kernel   one thread a star: x_trial = clip(x0), the state reset.
//   No atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/payne_hip.h"
#include "host_prologue.hpp"
#include "lmfit_core.hpp"
#include "lmfit_pair_core.hpp"
#include "lmfit_phot_core.hpp"

namespace lm = payne::lmfit;
namespace nt = payne::ntile;
namespace chebs = payne::chebs;

struct payne_lmfit {
  int device = 0, K = 0, max_stars = 0, B = 0;
  payne_lmfit_opts opts;
  lm::Box box;
  lm::State st;
  std::vector<void*> owned;
};

namespace {

using payne::host::OnDevice;
using payne::host::aligned16;
using payne::host::fail;

__global__ void __launch_bounds__(nt::kThreads) payne_lmfit_begin_kernel(const double* __restrict__ x0, int B, int K, const lm::State st,
                                                                         const lm::Box box, double lambda0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) lm::begin_star(st, (size_t)b, K, x0 + (size_t)b * (size_t)K, box, lambda0);
}

// The photometric arrays of payne_lmfit_update_phot, by value: one star's are [F], dmags [F][ncol], the priors [K] (or both NULL).
struct PhotArgs {
  const double *mags, *dmags, *obs, *pw, *mu, *sigma;
  int F;
  lm::PhotMap map;
};

// One star's update, the body of both kernels below.  rows holds 1 + K rows a star, or with POLY 1 + Km, Km = K - P; x and P are read
// with POLY only, ph with PHOT only (then Km = K - P - ph.map.Kp).
template <bool VEC, bool POLY, bool PHOT>
__device__ __forceinline__ void update_body(const float* __restrict__ rows, long long ld, const float* __restrict__ flux,
                                            const double* __restrict__ w, long long ld_f, const double* __restrict__ x, int n, int K, int P,
                                            const lm::State& st, const lm::Box& box, const payne_lmfit_opts& opts, const PhotArgs& ph) {
  __shared__ double part[nt::kWaves][nt::kTileSize];
  __shared__ double tile[nt::kTileSize];
  __shared__ double work[lm::kWorkDoubles];
  __shared__ double coef[lm::kMaxK];                                // (POLY only: the plain form never names it)
  const size_t b = blockIdx.x;
  if (st.status[b] != PAYNE_LMFIT_RUNNING) return;                  // (the whole workgroup)
  const int tid = threadIdx.x, i = tid & 15;
  const int Kp = PHOT ? ph.map.Kp : 0;
  const int Km = (POLY ? K - P : K) - Kp;
  if constexpr (POLY) {
    if (tid < P) coef[tid] = st.x_trial[b * (size_t)K + (size_t)(Km + Kp + tid)];
    __syncthreads();
  }
  const bool live = PHOT ? lm::has_row(i, Km, Kp, K) : i <= K, residual = i == K;
  const int j = lm::series_index(i, Km + Kp, K);
  const float* ra = rows + (b * (size_t)(1 + Km) + (size_t)lm::row_of(i, Km)) * (size_t)ld;   // the lane's row (row 0, the model, where it has none)
  // PHOT: the star's filters are asked for here and wait in registers behind the pixels: F ncol <= 448 derivatives, two a thread
  double pd0 = 0.0, pd1 = 0.0, pres = 0.0, pwt = 0.0;
  if constexpr (PHOT) {
    const int nd = ph.F * ph.map.ncol;
    if (tid < nd) pd0 = ph.dmags[b * (size_t)nd + (size_t)tid];
    if (tid + nt::kThreads < nd) pd1 = ph.dmags[b * (size_t)nd + (size_t)(tid + nt::kThreads)];
    if (tid < ph.F) {
      pwt = ph.pw[b * (size_t)ph.F + (size_t)tid];
      pres = lm::phot_residual(ph.obs[b * (size_t)ph.F + (size_t)tid], ph.mags[b * (size_t)ph.F + (size_t)tid]);
    }
  }
  const float* fb = flux + b * (size_t)ld_f;
  const double* wb = w + b * (size_t)ld_f;
  const nt::d4 acc = nt::wave_sums(n, [&](int p) PAYNE_TILE_CALLABLE {
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double wv[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0}, sv[4];                       // (sv: POLY only)
    if constexpr (POLY) nt::load4<VEC>(x, p, n, p + 3 < n, xv);     // (x holds n values and no more)
    if (p < n) {                                                    // p + 3 < ld and ld_f where VEC: both are multiples of four
      nt::load4<VEC>(wb, p, n, true, wv);
      if (live) nt::load4<VEC>(ra, p, n, true, a);
      if (residual) nt::load4<VEC>(fb, p, n, true, f);
    }
    if constexpr (POLY) chebs::series4(coef, j, P, xv, sv);
    return [=](int t, double* r, double* wt) PAYNE_TILE_CALLABLE {
      if constexpr (POLY) *r = lm::operand_poly(i, K, a[t], f[t], sv[t]);
      else *r = lm::operand(i, K, a[t], f[t]);
      *wt = wv[t];
      return live && p + t < n && wv[t] != 0.0;
    };
  });
  nt::sum_waves(acc, part, tile, []() PAYNE_TILE_CALLABLE { __syncthreads(); });
  if constexpr (PHOT) {                                             // (part is free behind sum_waves' barrier: the block and the filters)
    double* pt = &part[0][0];
    double* dm = pt + nt::kTileSize;
    double* res = dm + lm::kPhotMaxF * lm::kPhotMaxCol;
    double* pw = res + lm::kPhotMaxF;
    static_assert(nt::kTileSize + lm::kPhotMaxF * (lm::kPhotMaxCol + 2) <= nt::kWaves * nt::kTileSize, "the filters fit into part");
    static_assert(lm::kPhotMaxF * lm::kPhotMaxCol <= 2 * nt::kThreads && lm::kPhotMaxF <= nt::kThreads, "two derivatives a thread");
    const int nd = ph.F * ph.map.ncol;
    if (tid < nd) dm[tid] = pd0;
    if (tid + nt::kThreads < nd) dm[tid + nt::kThreads] = pd1;
    if (tid < ph.F) { res[tid] = pres; pw[tid] = pwt; }
    __syncthreads();
    const int ei = tid >> 4, ej = tid & 15;
    pt[tid] = ei <= ej && ej <= K ? lm::phot_element(ph.map, ei, ej, K, ph.F, dm, res, pw) : 0.0;
    __syncthreads();
    if (tid == 0)
      lm::add_block(tile, pt, K, st.x_trial + b * (size_t)K, ph.mu ? ph.mu + b * (size_t)K : nullptr, ph.sigma ? ph.sigma + b * (size_t)K : nullptr);
  }
  if (tid == 0) lm::update_star(st, b, K, tile, opts, box, work);
}

// payne_lmfit_update / _poly, and payne_lmfit_update_phot with the photometric arrays behind the same arguments.
template <bool VEC, bool POLY>
__global__ void __launch_bounds__(nt::kThreads) payne_lmfit_update_kernel(const float* __restrict__ rows, long long ld,
                                                                          const float* __restrict__ flux, const double* __restrict__ w,
                                                                          long long ld_f, const double* __restrict__ x, int n, int K, int P,
                                                                          const lm::State st, const lm::Box box, const payne_lmfit_opts opts) {
  update_body<VEC, POLY, false>(rows, ld, flux, w, ld_f, x, n, K, P, st, box, opts, PhotArgs{});
}
template <bool VEC, bool POLY>
__global__ void __launch_bounds__(nt::kThreads) payne_lmfit_update_phot_kernel(const float* __restrict__ rows, long long ld,
                                                                               const float* __restrict__ flux, const double* __restrict__ w,
                                                                               long long ld_f, const double* __restrict__ x, int n, int K, int P,
                                                                               const lm::State st, const lm::Box box,
                                                                               const payne_lmfit_opts opts, const PhotArgs ph) {
  update_body<VEC, POLY, true>(rows, ld, flux, w, ld_f, x, n, K, P, st, box, opts, ph);
}

// One star's update for two components: rows_a [B][1 + Ka][ld], rows_b [B][1 + Kb][ld]; x is read with P > 0 only.
template <bool VEC>
__device__ __forceinline__ void update_pair_body(const float* __restrict__ rows_a, int Ka, const float* __restrict__ rows_b, int Kb, long long ld,
                                                 const float* __restrict__ flux, const double* __restrict__ w, long long ld_f,
                                                 const double* __restrict__ x, int n, int K, int Kl, int P, const lm::State& st, const lm::Box& box,
                                                 const payne_lmfit_opts& opts, const lm::PairMap& map) {
  __shared__ double part[nt::kWaves][nt::kTileSize];
  __shared__ double tile[nt::kTileSize];
  __shared__ double work[lm::kWorkDoubles];
  __shared__ double qc[1 + lm::kMaxK];                              // the star's q, then its coefficients
  const size_t b = blockIdx.x;
  if (st.status[b] != PAYNE_LMFIT_RUNNING) return;                  // (the whole workgroup)
  const int tid = threadIdx.x, i = tid & 15;
  if (tid <= P) qc[tid] = st.x_trial[b * (size_t)K + (size_t)(Kl + tid)];
  __syncthreads();
  const double q = qc[0], omq = 1.0 - q;
  const double* coef = qc + 1;
  const bool live = i <= K, residual = i == K;
  const int j = lm::pair_series_index(i, Kl, K);
  const int ia = i < Kl ? map.ia[i] : 0, ib = i < Kl ? map.ib[i] : 0;
  const bool has_a = live && ia >= 0, has_b = live && ib >= 0;
  const float* ra = rows_a + (b * (size_t)(1 + Ka) + (size_t)(i < Kl && ia >= 0 ? 1 + ia : 0)) * (size_t)ld;
  const float* rb = rows_b + (b * (size_t)(1 + Kb) + (size_t)(i < Kl && ib >= 0 ? 1 + ib : 0)) * (size_t)ld;
  double ca, cb;
  lm::pair_weights(i, Kl, omq, q, &ca, &cb);
  const float* fb = flux + b * (size_t)ld_f;
  const double* wb = w + b * (size_t)ld_f;
  const nt::d4 acc = nt::wave_sums(n, [&](int p) PAYNE_TILE_CALLABLE {
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, c[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double wv[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0}, sv[4] = {1.0, 1.0, 1.0, 1.0};
    if (P > 0) nt::load4<VEC>(x, p, n, p + 3 < n, xv);              // (x holds n values and no more)
    if (p < n) {                                                    // p + 3 < ld and ld_f where VEC: both are multiples of four
      nt::load4<VEC>(wb, p, n, true, wv);
      if (has_a) nt::load4<VEC>(ra, p, n, true, a);
      if (has_b) nt::load4<VEC>(rb, p, n, true, c);
      if (residual) nt::load4<VEC>(fb, p, n, true, f);
    }
    if (P > 0) chebs::series4(coef, j, P, xv, sv);
    return [=](int t, double* r, double* wt) PAYNE_TILE_CALLABLE {
      *r = lm::operand_pair_mix(i, K, ca, cb, a[t], c[t], f[t], sv[t]);
      *wt = wv[t];
      return live && p + t < n && wv[t] != 0.0;
    };
  });
  nt::sum_waves(acc, part, tile, []() PAYNE_TILE_CALLABLE { __syncthreads(); });
  if (tid == 0) lm::update_star(st, b, K, tile, opts, box, work);
}

template <bool VEC>
__global__ void __launch_bounds__(nt::kThreads) payne_lmfit_update_pair_kernel(const float* __restrict__ rows_a, int Ka,
                                                                               const float* __restrict__ rows_b, int Kb, long long ld,
                                                                               const float* __restrict__ flux, const double* __restrict__ w,
                                                                               long long ld_f, const double* __restrict__ x, int n, int K, int Kl,
                                                                               int P, const lm::State st, const lm::Box box,
                                                                               const payne_lmfit_opts opts, const lm::PairMap map) {
  update_pair_body<VEC>(rows_a, Ka, rows_b, Kb, ld, flux, w, ld_f, x, n, K, Kl, P, st, box, opts, map);
}

template <class T>
bool alloc(payne_lmfit* h, T** p, size_t count) {
  void* v = nullptr;
  if (hipMalloc(&v, count * sizeof(T)) != hipSuccess || hipMemset(v, 0, count * sizeof(T)) != hipSuccess) return false;
  h->owned.push_back(v);
  *p = static_cast<T*>(v);
  return true;
}

// One update of the handle's B stars; P == 0 and x == NULL (which aligned16 passes): the plain form.  ph: the photometric block, or NULL.
int launch_update(payne_lmfit* h, int P, const float* rows, int ld, const float* flux, const double* w, int ld_f, const double* x, int n,
                  void* stream, const PhotArgs* ph = nullptr) {
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  const bool vec = ld % 4 == 0 && ld_f % 4 == 0 && aligned16(rows) && aligned16(flux) && aligned16(w) && aligned16(x);
  const dim3 grid((unsigned)h->B), block(nt::kThreads);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (ph) {
    const auto kernel = P ? (vec ? payne_lmfit_update_phot_kernel<true, true> : payne_lmfit_update_phot_kernel<false, true>)
                          : (vec ? payne_lmfit_update_phot_kernel<true, false> : payne_lmfit_update_phot_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, rows, (long long)ld, flux, w, (long long)ld_f, x, n, h->K, P, h->st, h->box, h->opts, *ph);
  } else {
    const auto kernel = P ? (vec ? payne_lmfit_update_kernel<true, true> : payne_lmfit_update_kernel<false, true>)
                          : (vec ? payne_lmfit_update_kernel<true, false> : payne_lmfit_update_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, rows, (long long)ld, flux, w, (long long)ld_f, x, n, h->K, P, h->st, h->box, h->opts);
  }
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

}  // namespace

extern "C" int payne_lmfit_create(int device, int K, int max_stars, const payne_lmfit_opts* opts, payne_lmfit** out) {
  if (!out) return fail(PAYNE_E_INVALID, "payne_lmfit_create: null handle pointer");
  *out = nullptr;
  if (K < 1 || max_stars < 1) return fail(PAYNE_E_INVALID, "payne_lmfit_create: K < 1 or max_stars < 1");
  if (K > lm::kMaxK) return fail(PAYNE_E_UNSUPPORTED, "payne_lmfit_create: K > 15 (K + 1 rows fill one 16 x 16 tile)");
  const payne_lmfit_opts o = opts ? *opts : lm::default_opts();
  if (!lm::opts_ok(o)) return fail(PAYNE_E_INVALID, "payne_lmfit_create: an option is out of range");
  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_lmfit_create: hipSetDevice");
  payne_lmfit* h = new payne_lmfit;
  h->device = device;
  h->K = K;
  h->max_stars = max_stars;
  h->opts = o;
  for (int k = 0; k < lm::kMaxK; ++k) {
    h->box.lo[k] = 0.0;
    h->box.hi[k] = 1.0;
  }
  const size_t S = (size_t)max_stars, k = (size_t)K;
  lm::State& st = h->st;
  const bool ok = alloc(h, &st.x_best, S * k) && alloc(h, &st.x_trial, S * k) && alloc(h, &st.A, S * k * k) && alloc(h, &st.g, S * k) &&
                  alloc(h, &st.chisq, S) && alloc(h, &st.lambda, S) && alloc(h, &st.status, S) && alloc(h, &st.niter, S) &&
                  alloc(h, &st.at_bound, S);
  if (!ok) {
    payne_lmfit_destroy(h);
    return fail(PAYNE_E_HIP, "payne_lmfit_create: allocating the state failed");
  }
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_lmfit_begin(payne_lmfit* h, const double* x0_dev, const double* lo, const double* hi, int B, void* stream) {
  if (!h || !lo || !hi || B < 0 || B > h->max_stars) return PAYNE_E_INVALID;
  for (int k = 0; k < h->K; ++k)
    if (!lm::finite(lo[k]) || !lm::finite(hi[k]) || !(lo[k] < hi[k])) return PAYNE_E_INVALID;
  if (B > 0 && !x0_dev) return PAYNE_E_INVALID;
  for (int k = 0; k < h->K; ++k) {
    h->box.lo[k] = lo[k];
    h->box.hi[k] = hi[k];
  }
  h->B = B;
  if (B == 0) return PAYNE_OK;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  hipLaunchKernelGGL(payne_lmfit_begin_kernel, dim3((unsigned)((B + nt::kThreads - 1) / nt::kThreads)), dim3(nt::kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), x0_dev, B, h->K, h->st, h->box, h->opts.lambda0);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" double* payne_lmfit_trial(payne_lmfit* h) { return h ? h->st.x_trial : nullptr; }

extern "C" int payne_lmfit_update(payne_lmfit* h, const float* rows_dev, int ld, const float* flux_dev, const double* w_dev, int ld_f,
                                  int n, void* stream) {
  if (!h || n < 1 || ld < n || ld_f < n) return PAYNE_E_INVALID;
  if (h->B == 0) return PAYNE_OK;
  if (!rows_dev || !flux_dev || !w_dev) return PAYNE_E_INVALID;
  return launch_update(h, 0, rows_dev, ld, flux_dev, w_dev, ld_f, nullptr, n, stream);
}

extern "C" int payne_lmfit_update_poly(payne_lmfit* h, int P, const float* rows_dev, int ld, const float* flux_dev, const double* w_dev,
                                       int ld_f, const double* x_dev, int n, void* stream) {
  if (!h || n < 1 || ld < n || ld_f < n || P < 1 || P > h->K) return PAYNE_E_INVALID;
  if (h->B == 0) return PAYNE_OK;
  if (!rows_dev || !flux_dev || !w_dev || !x_dev) return PAYNE_E_INVALID;
  return launch_update(h, P, rows_dev, ld, flux_dev, w_dev, ld_f, x_dev, n, stream);
}

extern "C" int payne_lmfit_update_phot(payne_lmfit* h, int Km, int Kp, int P, const float* rows_dev, int ld, const float* flux_dev,
                                       const double* w_dev, int ld_f, const double* x_dev, int n, int F, int ncol, const int* sed_col,
                                       const double* mags_dev, const double* dmags_dev, const double* obs_dev, const double* pw_dev,
                                       const double* prior_mu_dev, const double* prior_sigma_dev, void* stream) {
  if (!h || n < 1 || ld < n || ld_f < n) return PAYNE_E_INVALID;
  const int rc = lm::check_phot(h->K, Km, Kp, P, F, ncol, sed_col, h->box, prior_mu_dev != nullptr, prior_sigma_dev != nullptr);
  if (rc == PAYNE_E_UNSUPPORTED) return fail(rc, "payne_lmfit_update_phot: F > 64 (a star's filters are staged in LDS)");
  if (rc != PAYNE_OK) return rc;
  if (h->B == 0) return PAYNE_OK;
  if (!rows_dev || !flux_dev || !w_dev || (P > 0 && !x_dev)) return PAYNE_E_INVALID;
  if (F > 0 && (!mags_dev || !dmags_dev || !obs_dev || !pw_dev)) return PAYNE_E_INVALID;
  PhotArgs ph{mags_dev, dmags_dev, obs_dev, pw_dev, prior_mu_dev, prior_sigma_dev, F, lm::PhotMap{}};
  ph.map.ncol = ncol;
  ph.map.Kp = Kp;
  for (int k = 0; k < lm::kMaxK; ++k) ph.map.sed_col[k] = k < h->K ? sed_col[k] : -1;
  return launch_update(h, P, rows_dev, ld, flux_dev, w_dev, ld_f, P > 0 ? x_dev : nullptr, n, stream, &ph);
}

extern "C" int payne_lmfit_update_pair(payne_lmfit* h, int Kl, int P, const int* ia, const int* ib, const float* rows_a_dev, int Ka,
                                       const float* rows_b_dev, int Kb, int ld, const float* flux_dev, const double* w_dev, int ld_f,
                                       const double* x_dev, int n, void* stream) {
  if (!h || n < 1 || ld < n || ld_f < n) return PAYNE_E_INVALID;
  const int rc = lm::check_pair(h->K, Kl, P, Ka, Kb, ia, ib);
  if (rc != PAYNE_OK) return rc;
  if (h->B == 0) return PAYNE_OK;
  if (!rows_a_dev || !rows_b_dev || !flux_dev || !w_dev || (P > 0 && !x_dev)) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  const double* x = P > 0 ? x_dev : nullptr;
  const bool vec = ld % 4 == 0 && ld_f % 4 == 0 && aligned16(rows_a_dev) && aligned16(rows_b_dev) && aligned16(flux_dev) && aligned16(w_dev) && aligned16(x);
  const auto kernel = vec ? payne_lmfit_update_pair_kernel<true> : payne_lmfit_update_pair_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)h->B), dim3(nt::kThreads), 0, reinterpret_cast<hipStream_t>(stream), rows_a_dev, Ka, rows_b_dev, Kb,
                     (long long)ld, flux_dev, w_dev, (long long)ld_f, x, n, h->K, Kl, P, h->st, h->box, h->opts, lm::pair_map(Kl, ia, ib));
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" int payne_lmfit_result(payne_lmfit* h, double* x_best, double* chisq, double* A, double* g, double* lambda, int* status,
                                  int* niter, unsigned* at_bound, void* stream) {
  if (!h) return PAYNE_E_INVALID;
  if (h->B == 0) return PAYNE_OK;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t B = (size_t)h->B, K = (size_t)h->K;
  bool ok = true;
  auto copy = [&](void* dst, const void* src, size_t bytes) {
    if (dst && ok) ok = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  };
  copy(x_best, h->st.x_best, B * K * sizeof(double));
  copy(chisq, h->st.chisq, B * sizeof(double));
  copy(A, h->st.A, B * K * K * sizeof(double));
  copy(g, h->st.g, B * K * sizeof(double));
  copy(lambda, h->st.lambda, B * sizeof(double));
  copy(status, h->st.status, B * sizeof(int));
  copy(niter, h->st.niter, B * sizeof(int));
  copy(at_bound, h->st.at_bound, B * sizeof(unsigned));
  return ok ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" void payne_lmfit_destroy(payne_lmfit* h) {
  if (!h) return;
  {
    OnDevice on(h->device);
    if (on.ok()) {
      (void)hipDeviceSynchronize();
      for (void* p : h->owned) (void)hipFree(p);
    }
  }
  delete h;
}
