// k_lmfit.hip -- payne_lmfit_*: batched Levenberg-Marquardt (include/payne_hip.h).  The arithmetic is lmfit_core.hpp, which runs on
// the host too (tests/emul/lmfit_emul.cpp).
//
//   payne_lmfit_update_kernel  one 256-thread workgroup a star, skipped when the star is no longer RUNNING.  Lane (i = lane & 15,
//     q = lane >> 4) of every wave reads four consecutive fp32 pixels of row i of R = [rows 1..K ; flux - row 0] and the four fp64
//     weights, and hands them to four v_mfma_f64_16x16x4_f64: A[i][k = q] = R[i][p], B[k = q][j = i] = R[i][p] w[p], the same
//     lane's value times w, so nothing is transposed.  D[i = (lane >> 4) + 4 v][j = lane & 15], v = 0..3, is G = R diag(w) R^T.
//     Each wave owns a contiguous stripe of pixel groups; the four partial tiles meet in LDS and are added in wave order.  Thread 0
//     then takes the star's step (lmfit_core.hpp: update_star) on LDS and the handle's arrays.  <VEC>: 16-byte loads (ld, ld_f
//     multiples of four, aligned pointers); otherwise element by element, the same values in the same places.
//     The kernel streams (1 + K) n fp32 + n fp32 + n fp64 per star once and is bound by HBM; the matrix instruction takes the
//     (K + 1)^2 / 2 products a pixel off the vector pipeline, which would otherwise bind it for K >= 4.
//   payne_lmfit_update_poly_kernel  the same launch for a model times a Chebyshev series whose P coefficients are the last P of the K
//     parameters: R = [p dm/dtheta ; m T_j(x) ; flux - m p] is formed in registers from the caller's 1 + Km rows, the star's
//     coefficients (x_trial, copied to LDS) and x, and never stored.  Every lane evaluates one series at its four pixels in one
//     loop of P - 2 steps (lmfit_core.hpp: series4): p, or T_j as the series of a unit vector.  Loads, pixel order, operand map,
//     the select for w == 0 and the wave-order sum are the kernel's above; update_star is the same call.
//   payne_lmfit_begin_kernel   one thread a star: x_trial = clip(x0), the state reset.
//   No atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/payne_hip.h"
#include "ctx_api.hpp"
#include "lmfit_core.hpp"

namespace lm = payne::lmfit;

struct payne_lmfit {
  int device = 0, K = 0, max_stars = 0, B = 0;
  payne_lmfit_opts opts;
  lm::Box box;
  lm::State st;
  std::vector<void*> owned;
};

namespace {

typedef double lm_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(lm::kThreads) payne_lmfit_begin_kernel(const double* __restrict__ x0, int B, int K, const lm::State st,
                                                                         const lm::Box box, double lambda0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) lm::begin_star(st, (size_t)b, K, x0 + (size_t)b * (size_t)K, box, lambda0);
}

template <bool VEC>
__global__ void __launch_bounds__(lm::kThreads) payne_lmfit_update_kernel(const float* __restrict__ rows, long long ld,
                                                                          const float* __restrict__ flux, const double* __restrict__ w,
                                                                          long long ld_f, int n, int K, const lm::State st, const lm::Box box,
                                                                          const payne_lmfit_opts opts) {
  __shared__ double part[lm::kWaves][lm::kTileSize];
  __shared__ double tile[lm::kTileSize];
  __shared__ double work[lm::kWorkDoubles];
  const size_t b = blockIdx.x;
  if (st.status[b] != PAYNE_LMFIT_RUNNING) return;                  // (the whole workgroup)
  const int tid = threadIdx.x, lane = tid & (lm::kWave - 1), wave = tid / lm::kWave;
  const int i = lane & 15, q = lane >> 4;
  const bool live = i <= K, residual = i == K;
  const float* ra = rows + (b * (size_t)(1 + K) + (size_t)(i < K ? 1 + i : 0)) * (size_t)ld;   // the lane's row (row 0 where it has none)
  const float* fb = flux + b * (size_t)ld_f;
  const double* wb = w + b * (size_t)ld_f;
  const int gpw = lm::groups_per_wave(n), groups = lm::groups_of(n);
  const int g0 = wave * gpw, g1 = g0 + gpw < groups ? g0 + gpw : groups;
  lm_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int grp = g0; grp < g1; ++grp) {
    const int p = lm::pixel_of(grp, q, 0);
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double wv[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
      if (p < n) {                                                  // p + 3 < ld and ld_f: both are multiples of four
        const double2 w01 = *reinterpret_cast<const double2*>(wb + p), w23 = *reinterpret_cast<const double2*>(wb + p + 2);
        wv[0] = w01.x; wv[1] = w01.y; wv[2] = w23.x; wv[3] = w23.y;
        if (live) {
          const float4 a4 = *reinterpret_cast<const float4*>(ra + p);
          a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
        }
        if (residual) {
          const float4 f4 = *reinterpret_cast<const float4*>(fb + p);
          f[0] = f4.x; f[1] = f4.y; f[2] = f4.z; f[3] = f4.w;
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (p + t < n) {
          wv[t] = wb[p + t];
          if (live) a[t] = ra[p + t];
          if (residual) f[t] = fb[p + t];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double av, bv;
      lm::operand_pair(lm::operand(i, K, a[t], f[t]), wv[t], live && p + t < n && wv[t] != 0.0, &av, &bv);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) part[wave][(q + 4 * v) * lm::kTile + i] = acc[v];
  __syncthreads();
  tile[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  __syncthreads();
  if (tid == 0) lm::update_star(st, b, K, tile, opts, box, work);
}

// The same with a continuum polynomial: K = Km + P, rows holds 1 + Km rows a star.
template <bool VEC>
__global__ void __launch_bounds__(lm::kThreads) payne_lmfit_update_poly_kernel(const float* __restrict__ rows, long long ld,
                                                                               const float* __restrict__ flux, const double* __restrict__ w,
                                                                               long long ld_f, const double* __restrict__ x, int n, int K, int P,
                                                                               const lm::State st, const lm::Box box, const payne_lmfit_opts opts) {
  __shared__ double part[lm::kWaves][lm::kTileSize];
  __shared__ double tile[lm::kTileSize];
  __shared__ double work[lm::kWorkDoubles];
  __shared__ double coef[lm::kMaxK];
  const size_t b = blockIdx.x;
  if (st.status[b] != PAYNE_LMFIT_RUNNING) return;                  // (the whole workgroup)
  const int tid = threadIdx.x, lane = tid & (lm::kWave - 1), wave = tid / lm::kWave;
  const int i = lane & 15, q = lane >> 4;
  const int Km = K - P;
  if (tid < P) coef[tid] = st.x_trial[b * (size_t)K + (size_t)(Km + tid)];
  __syncthreads();
  const bool live = i <= K, residual = i == K;
  const int j = lm::series_index(i, Km, K);
  const float* ra = rows + (b * (size_t)(1 + Km) + (size_t)(i < Km ? 1 + i : 0)) * (size_t)ld;   // the lane's row (row 0, the model, where it has none)
  const float* fb = flux + b * (size_t)ld_f;
  const double* wb = w + b * (size_t)ld_f;
  const int gpw = lm::groups_per_wave(n), groups = lm::groups_of(n);
  const int g0 = wave * gpw, g1 = g0 + gpw < groups ? g0 + gpw : groups;
  lm_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int grp = g0; grp < g1; ++grp) {
    const int p = lm::pixel_of(grp, q, 0);
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double wv[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC && p + 3 < n) {                                         // (x holds n values and no more)
      const double2 x01 = *reinterpret_cast<const double2*>(x + p), x23 = *reinterpret_cast<const double2*>(x + p + 2);
      xv[0] = x01.x; xv[1] = x01.y; xv[2] = x23.x; xv[3] = x23.y;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (p + t < n) xv[t] = x[p + t];
    }
    if (VEC) {
      if (p < n) {                                                  // p + 3 < ld and ld_f: both are multiples of four
        const double2 w01 = *reinterpret_cast<const double2*>(wb + p), w23 = *reinterpret_cast<const double2*>(wb + p + 2);
        wv[0] = w01.x; wv[1] = w01.y; wv[2] = w23.x; wv[3] = w23.y;
        if (live) {
          const float4 a4 = *reinterpret_cast<const float4*>(ra + p);
          a[0] = a4.x; a[1] = a4.y; a[2] = a4.z; a[3] = a4.w;
        }
        if (residual) {
          const float4 f4 = *reinterpret_cast<const float4*>(fb + p);
          f[0] = f4.x; f[1] = f4.y; f[2] = f4.z; f[3] = f4.w;
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (p + t < n) {
          wv[t] = wb[p + t];
          if (live) a[t] = ra[p + t];
          if (residual) f[t] = fb[p + t];
        }
    }
    double sv[4];
    lm::series4(coef, j, P, xv, sv);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double av, bv;
      lm::operand_pair(lm::operand_poly(i, K, a[t], f[t], sv[t]), wv[t], live && p + t < n && wv[t] != 0.0, &av, &bv);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) part[wave][(q + 4 * v) * lm::kTile + i] = acc[v];
  __syncthreads();
  tile[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  __syncthreads();
  if (tid == 0) lm::update_star(st, b, K, tile, opts, box, work);
}

int fail(int code, const std::string& msg) {
  payne::set_create_error(msg);
  return code;
}

// Selects `device` for its scope and puts the caller's device back on the way out.
class OnDevice {
 public:
  explicit OnDevice(int device) {
    (void)hipGetDevice(&prev_);
    ok_ = hipSetDevice(device) == hipSuccess;
  }
  ~OnDevice() { (void)hipSetDevice(prev_); }
  OnDevice(const OnDevice&) = delete;
  OnDevice& operator=(const OnDevice&) = delete;
  bool ok() const { return ok_; }

 private:
  int prev_ = 0;
  bool ok_ = false;
};

template <class T>
bool alloc(payne_lmfit* h, T** p, size_t count) {
  void* v = nullptr;
  if (hipMalloc(&v, count * sizeof(T)) != hipSuccess || hipMemset(v, 0, count * sizeof(T)) != hipSuccess) return false;
  h->owned.push_back(v);
  *p = static_cast<T*>(v);
  return true;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

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
  hipLaunchKernelGGL(payne_lmfit_begin_kernel, dim3((unsigned)((B + lm::kThreads - 1) / lm::kThreads)), dim3(lm::kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), x0_dev, B, h->K, h->st, h->box, h->opts.lambda0);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" double* payne_lmfit_trial(payne_lmfit* h) { return h ? h->st.x_trial : nullptr; }

extern "C" int payne_lmfit_update(payne_lmfit* h, const float* rows_dev, int ld, const float* flux_dev, const double* w_dev, int ld_f,
                                  int n, void* stream) {
  if (!h || n < 1 || ld < n || ld_f < n) return PAYNE_E_INVALID;
  if (h->B == 0) return PAYNE_OK;
  if (!rows_dev || !flux_dev || !w_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool vec = ld % 4 == 0 && ld_f % 4 == 0 && aligned16(rows_dev) && aligned16(flux_dev) && aligned16(w_dev);
  if (vec)
    hipLaunchKernelGGL(payne_lmfit_update_kernel<true>, dim3((unsigned)h->B), dim3(lm::kThreads), 0, st, rows_dev, (long long)ld, flux_dev,
                       w_dev, (long long)ld_f, n, h->K, h->st, h->box, h->opts);
  else
    hipLaunchKernelGGL(payne_lmfit_update_kernel<false>, dim3((unsigned)h->B), dim3(lm::kThreads), 0, st, rows_dev, (long long)ld, flux_dev,
                       w_dev, (long long)ld_f, n, h->K, h->st, h->box, h->opts);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" int payne_lmfit_update_poly(payne_lmfit* h, int P, const float* rows_dev, int ld, const float* flux_dev, const double* w_dev,
                                       int ld_f, const double* x_dev, int n, void* stream) {
  if (!h || n < 1 || ld < n || ld_f < n || P < 1 || P > h->K) return PAYNE_E_INVALID;
  if (h->B == 0) return PAYNE_OK;
  if (!rows_dev || !flux_dev || !w_dev || !x_dev) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool vec = ld % 4 == 0 && ld_f % 4 == 0 && aligned16(rows_dev) && aligned16(flux_dev) && aligned16(w_dev) && aligned16(x_dev);
  if (vec)
    hipLaunchKernelGGL(payne_lmfit_update_poly_kernel<true>, dim3((unsigned)h->B), dim3(lm::kThreads), 0, st, rows_dev, (long long)ld,
                       flux_dev, w_dev, (long long)ld_f, x_dev, n, h->K, P, h->st, h->box, h->opts);
  else
    hipLaunchKernelGGL(payne_lmfit_update_poly_kernel<false>, dim3((unsigned)h->B), dim3(lm::kThreads), 0, st, rows_dev, (long long)ld,
                       flux_dev, w_dev, (long long)ld_f, x_dev, n, h->K, P, h->st, h->box, h->opts);
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
