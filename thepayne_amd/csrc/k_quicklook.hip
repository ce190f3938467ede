// k_quicklook.hip -- the two grid scans of the reference's quick-look classes (Payne/fitting/fitutils.py), one chi^2 per grid
// value over a whole spectrum:
//   payne_rv_scan      RVcalc.chisq_rv (:79-94) for G velocities: the model interpolated at the observed pixels on the
//                      Doppler-shifted grid (interp1d linear, fill value 1.0), chi^2 against the observed flux;
//   payne_chisq_below  the tail of BROADcalc.chisq_broad (:148-154) for G broadened rows that payne_smooth_batch left on
//                      the device: pixels below a threshold compacted in order, chi^2 with the reference's pairing.
// One 256-thread workgroup per grid value, threads over pixels, fp64 throughout (quicklook_core.hpp holds the arithmetic and
// runs on the host too).  The sums are reduced in a fixed order -- shuffles inside a wave, then LDS across the four waves --
// without floating-point atomics, so a call returns the same bits every time.  Analysis helpers of the public classes:
// nothing the likelihood calls.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/payne_hip.h"

// (a fused multiply-add would round modwave * (1 + rv / c) and the interpolation differently from the host restatement)
#pragma clang fp contract(off)

#include "quicklook_core.hpp"

using namespace payne;

namespace {

// Sum of one value per thread over the workgroup, on thread 0: lanes by halving, then the waves in ascending order.
__device__ __forceinline__ double block_sum(double v, double* wave_sum) {
  for (int off = ql::kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, ql::kWave);
  const int lane = threadIdx.x & (ql::kWave - 1), wave = threadIdx.x / ql::kWave;
  if (lane == 0) wave_sum[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < ql::kWaves; ++w) total += wave_sum[w];
  return total;
}

__global__ void __launch_bounds__(ql::kThreads) payne_rv_scan_kernel(const double* __restrict__ modwave, const double* __restrict__ modflux,
                                                                      int nm, const double* __restrict__ wave,
                                                                      const double* __restrict__ flux, const double* __restrict__ eflux,
                                                                      int nobs, const double* __restrict__ rv, int G,
                                                                      double* __restrict__ chisq) {
  __shared__ double wave_sum[ql::kWaves];
  const int g = blockIdx.x;
  if (g >= G) return;
  const double part = ql::rv_partial(modwave, modflux, nm, wave, flux, eflux, nobs, rv[g], threadIdx.x, ql::kThreads);
  const double total = block_sum(part, wave_sum);
  if (threadIdx.x == 0) chisq[g] = total;
}

__global__ void __launch_bounds__(ql::kThreads) payne_chisq_below_kernel(const float* __restrict__ rows, int ld, int n, int G,
                                                                          const double* __restrict__ flux,
                                                                          const double* __restrict__ eflux, double threshold,
                                                                          double* __restrict__ chisq, int* __restrict__ n_kept) {
  __shared__ double wave_sum[ql::kWaves];
  __shared__ int wave_total[ql::kWaves];
  const int g = blockIdx.x;
  if (g >= G) return;
  const float* row = rows + (size_t)g * (size_t)ld;
  const int lane = threadIdx.x & (ql::kWave - 1), wave = threadIdx.x / ql::kWave;
  int kept_before = 0;                            // kept pixels of the chunks already done (the same in every thread)
  double acc = 0.0;
  for (int base = 0; base < n; base += ql::kThreads) {
    const int i = base + (int)threadIdx.x;
    const bool keep = i < n && ql::keep_below(row[i < n ? i : 0], threshold);
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) wave_total[wave] = __builtin_popcountll(ballot);
    __syncthreads();
    if (keep) acc += ql::below_term(row, flux, eflux, i, kept_before + ql::wave_prefix(wave_total, wave) + ql::lane_prefix(ballot, lane));
    kept_before += ql::wave_prefix(wave_total, ql::kWaves);
    __syncthreads();                              // wave_total is rewritten by the next chunk
  }
  const double total = block_sum(acc, wave_sum);
  if (threadIdx.x == 0) {
    chisq[g] = total;
    n_kept[g] = kept_before;
  }
}

struct DevBuf {
  std::vector<void*> p;
  ~DevBuf() { for (void* q : p) (void)hipFree(q); }
  template <class V> V* put(const V* host, size_t n) {
    void* d = nullptr;
    if (hipMalloc(&d, (n ? n : 1) * sizeof(V)) != hipSuccess) return nullptr;
    p.push_back(d);
    if (host && n && hipMemcpy(d, host, n * sizeof(V), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return reinterpret_cast<V*>(d);
  }
};

}  // namespace

extern "C" int payne_rv_scan(int device, const double* modwave, const double* modflux, int nm, const double* wave,
                             const double* flux, const double* eflux, int nobs, const double* rv, int G, double* chisq) {
  if (!modwave || !modflux || !wave || !flux || !eflux || !rv || !chisq || nm < 2 || nobs < 1 || G < 1) return PAYNE_E_INVALID;
  for (int j = 1; j < nm; ++j)
    if (!(modwave[j] > modwave[j - 1])) return PAYNE_E_INVALID;      // (also refuses a NaN wavelength)
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(device) != hipSuccess) return PAYNE_E_HIP;
  int rc = PAYNE_OK;
  {
    DevBuf B;
    const double* dmw = B.put(modwave, (size_t)nm);
    const double* dmf = B.put(modflux, (size_t)nm);
    const double* dw = B.put(wave, (size_t)nobs);
    const double* df = B.put(flux, (size_t)nobs);
    const double* de = B.put(eflux, (size_t)nobs);
    const double* drv = B.put(rv, (size_t)G);
    double* dchi = B.put<double>(nullptr, (size_t)G);
    if (!dmw || !dmf || !dw || !df || !de || !drv || !dchi) rc = PAYNE_E_HIP;
    if (!rc) {
      hipLaunchKernelGGL(payne_rv_scan_kernel, dim3(G), dim3(ql::kThreads), 0, 0, dmw, dmf, nm, dw, df, de, nobs, drv, G, dchi);
      if (hipGetLastError() != hipSuccess) rc = PAYNE_E_HIP;
      if (!rc && hipDeviceSynchronize() != hipSuccess) rc = PAYNE_E_HIP;
      if (!rc && hipMemcpy(chisq, dchi, (size_t)G * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = PAYNE_E_HIP;
    }
  }
  (void)hipSetDevice(prev);
  return rc;
}

extern "C" int payne_chisq_below(int device, const float* rows, int ld, int n, int G, const double* flux, const double* eflux,
                                 double threshold, double* chisq, int* n_kept, void* stream) {
  if (!rows || !flux || !eflux || !chisq || !n_kept || n < 1 || n > ld || G < 1) return PAYNE_E_INVALID;
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(device) != hipSuccess) return PAYNE_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = PAYNE_OK;
  {
    DevBuf B;
    const double* df = B.put(flux, (size_t)n);
    const double* de = B.put(eflux, (size_t)n);
    double* dchi = B.put<double>(nullptr, (size_t)G);
    int* dkept = B.put<int>(nullptr, (size_t)G);
    if (!df || !de || !dchi || !dkept) rc = PAYNE_E_HIP;
    if (!rc) {
      // (the rows were written on `stream`: the launch is ordered behind them there; the uploads above have completed)
      hipLaunchKernelGGL(payne_chisq_below_kernel, dim3(G), dim3(ql::kThreads), 0, st, rows, ld, n, G, df, de, threshold, dchi, dkept);
      if (hipGetLastError() != hipSuccess) rc = PAYNE_E_HIP;
      if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = PAYNE_E_HIP;
      if (!rc && hipMemcpy(chisq, dchi, (size_t)G * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = PAYNE_E_HIP;
      if (!rc && hipMemcpy(n_kept, dkept, (size_t)G * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = PAYNE_E_HIP;
    }
    if (rc == PAYNE_E_HIP) (void)hipStreamSynchronize(st);       // nothing of DevBuf is freed under a running kernel
  }
  (void)hipSetDevice(prev);
  return rc;
}
