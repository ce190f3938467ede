// k_mad.hip -- payne_mad_stats: the medians of |truth - pred| that Payne/testing/testspec.py takes of its residual matrix
// (TestSpec's report, :94-108, :125-208, :227-361): down the columns -- per pixel, over the rows of each of G row sets -- and
// along the rows -- per spectrum.  Both inputs are row-major fp32 [N][ld] on the device; the residual is formed in fp64 and
// never stored, every pass recomputes it.  The selection itself (radix selection on the integer image of the residual, 8 passes
// of 8 bits and, for an even count, one more sweep) is mad_core.hpp, which runs on the host too (tests/emul/mad_emul.cpp).
//
//   payne_mad_cols_kernel  one 256-thread workgroup per (64 columns, row set).  Lane l of every wave owns column l of the block,
//                          so a wave reads 64 adjacent pixels of one row (256 B) per load; the four waves split the rows in
//                          chunks of 64, find a chunk's members with one ballot over the set's bytes and skip the rest without
//                          reading them.  The counters -- 256 bins x 64 columns x 4 B = 64 KiB of LDS, bin-major, so that the
//                          lanes of a wave land on different banks -- are shared by the four waves: integer ds_add, no order to
//                          depend on.  After a sweep each wave adds up a quarter of every column's bins and wave 0 walks the four
//                          sums and one quarter for the digit.
//   payne_mad_rows_kernel  one wave per row (four rows per workgroup), lanes striding over the row's pixels; 256 counters per
//                          wave, each lane adds up four of them, lane 0 walks.
// There are no floating-point sums anywhere: a second call returns the same bits.  Analysis helper of Payne.testing: nothing
// the likelihood calls.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "mad_core.hpp"

using namespace payne;

namespace {

typedef unsigned long long u64;

constexpr size_t kColsLds = (size_t)mad::kBins * mad::kCols * sizeof(unsigned)        // hist [kBins][kCols]
                            + (size_t)mad::kWaves * mad::kCols * sizeof(unsigned)     // part [kWaves][kCols]
                            + (size_t)mad::kWaves * mad::kCols * sizeof(u64)          // mins [kWaves][kCols]
                            + (size_t)mad::kCols * sizeof(mad::Sel)                   // sel  [kCols]
                            + (size_t)mad::kCols * sizeof(unsigned);                  // any_nan [kCols]

// f(key) for the residual of every member row of this wave's chunks at column `col` (kRowUnroll rows' loads in flight).
// `grp` = the row set's N bytes.  Every lane of the wave must call it (the ballot); lanes with live == false load nothing.
template <class F>
__device__ __forceinline__ void for_member_rows(const float* __restrict__ pred, int ld_pred, const float* __restrict__ truth,
                                                int ld_truth, int N, int col, bool live, const unsigned char* __restrict__ grp,
                                                int wave, int lane, F&& f) {
  for (long long row0 = (long long)wave * mad::kWave; row0 < (long long)N; row0 += (long long)mad::kWaves * mad::kWave) {
    const long long mine = row0 + lane;
    u64 members = __ballot(mine < (long long)N && grp[mine < (long long)N ? mine : 0] != 0);
    while (members) {
      float t[mad::kRowUnroll], p[mad::kRowUnroll];
      bool have[mad::kRowUnroll];
#pragma unroll
      for (int u = 0; u < mad::kRowUnroll; ++u) {
        have[u] = members != 0ull;
        const long long row = row0 + (have[u] ? __builtin_ctzll(members) : 0);
        members &= members - 1ull;
        t[u] = p[u] = 0.0f;
        if (have[u] && live) {
          t[u] = truth[(size_t)row * (size_t)ld_truth + (size_t)col];
          p[u] = pred[(size_t)row * (size_t)ld_pred + (size_t)col];
        }
      }
#pragma unroll
      for (int u = 0; u < mad::kRowUnroll; ++u)
        if (have[u] && live) f(mad::residual_key(t[u], p[u]));
    }
  }
}

__global__ void __launch_bounds__(mad::kThreads) payne_mad_cols_kernel(const float* __restrict__ pred, int ld_pred,
                                                                        const float* __restrict__ truth, int ld_truth, int N, int P,
                                                                        const unsigned char* __restrict__ groups,
                                                                        double* __restrict__ pix_med) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mad_sm[];
  unsigned* hist = reinterpret_cast<unsigned*>(mad_sm);
  unsigned* part = hist + mad::kBins * mad::kCols;
  u64* mins = reinterpret_cast<u64*>(part + mad::kWaves * mad::kCols);
  mad::Sel* sel = reinterpret_cast<mad::Sel*>(mins + mad::kWaves * mad::kCols);
  unsigned* any_nan = reinterpret_cast<unsigned*>(sel + mad::kCols);

  const int tid = threadIdx.x, lane = tid & (mad::kWave - 1), wave = tid / mad::kWave;
  const int g = blockIdx.y;
  const long long col_ll = (long long)blockIdx.x * mad::kCols + lane;
  const bool live = col_ll < (long long)P;
  const int col = live ? (int)col_ll : 0;
  const unsigned char* grp = groups + (size_t)g * (size_t)N;
  unsigned* my_bins = hist + lane;                                  // this column's counters, kCols apart

  for (int b = tid; b < mad::kBins * mad::kCols; b += mad::kThreads) hist[b] = 0u;
  if (tid < mad::kCols) any_nan[tid] = 0u;
  __syncthreads();

  u64 prefix = 0ull;
  for (int pass = 0; pass < mad::kPasses; ++pass) {
    bool saw_nan = false;
    for_member_rows(pred, ld_pred, truth, ld_truth, N, col, live, grp, wave, lane, [&](u64 k) {
      if (pass == 0) saw_nan = saw_nan || mad::key_is_nan(k);
      if (mad::in_prefix(k, prefix, pass)) atomicAdd(&my_bins[mad::digit_of(k, pass) * mad::kCols], 1u);
    });
    if (saw_nan) atomicOr(&any_nan[lane], 1u);
    __syncthreads();
    part[wave * mad::kCols + lane] = mad::sum_bins(my_bins + wave * mad::kQuarter * mad::kCols, mad::kCols, mad::kQuarter);
    __syncthreads();
    if (wave == 0) mad::choose_digit(&sel[lane], pass, part + lane, mad::kCols, mad::kWaves, my_bins, mad::kCols, mad::kQuarter);
    __syncthreads();
    prefix = sel[lane].prefix;
    for (int b = tid; b < mad::kBins * mad::kCols; b += mad::kThreads) hist[b] = 0u;
    __syncthreads();
  }

  const mad::Sel s = sel[lane];
  // (m is the set's, the same in every live column: an even set takes the extra sweep unless no column needs it)
  if (__syncthreads_or(live && mad::needs_next(s))) {
    u64 mn = mad::kNoKey;
    for_member_rows(pred, ld_pred, truth, ld_truth, N, col, live, grp, wave, lane, [&](u64 k) {
      if (k > s.prefix && k < mn) mn = k;
    });
    mins[wave * mad::kCols + lane] = mn;
    __syncthreads();
  }
  if (wave == 0 && live) {
    u64 next = mad::kNoKey;
    if (mad::needs_next(s))
      for (int w = 0; w < mad::kWaves; ++w) { const u64 v = mins[w * mad::kCols + lane]; next = v < next ? v : next; }
    pix_med[(size_t)g * (size_t)P + (size_t)col] = mad::median_of(s, next, any_nan[lane] != 0u);
  }
}

__global__ void __launch_bounds__(mad::kThreads) payne_mad_rows_kernel(const float* __restrict__ pred, int ld_pred,
                                                                        const float* __restrict__ truth, int ld_truth, int N, int P,
                                                                        double* __restrict__ row_med) {
  __shared__ unsigned hist_all[mad::kWaves][mad::kBins];
  __shared__ unsigned part_all[mad::kWaves][mad::kWave];
  __shared__ u64 mins_all[mad::kWaves][mad::kWave];
  __shared__ mad::Sel sel_all[mad::kWaves];
  __shared__ unsigned any_nan_all[mad::kWaves];

  const int tid = threadIdx.x, lane = tid & (mad::kWave - 1), wave = tid / mad::kWave;
  const long long row = (long long)blockIdx.x * mad::kWaves + wave;
  const bool active = row < (long long)N;                           // (an idle wave still meets every barrier)
  const float* t_row = truth + (size_t)(active ? row : 0) * (size_t)ld_truth;
  const float* p_row = pred + (size_t)(active ? row : 0) * (size_t)ld_pred;
  unsigned* hist = hist_all[wave];
  unsigned* part = part_all[wave];

  for (int b = lane; b < mad::kBins; b += mad::kWave) hist[b] = 0u;
  if (lane == 0) any_nan_all[wave] = 0u;
  __syncthreads();

  u64 prefix = 0ull;
  for (int pass = 0; pass < mad::kPasses; ++pass) {
    bool saw_nan = false;
    if (active) {
#pragma unroll 4
      for (int j = lane; j < P; j += mad::kWave) {
        const u64 k = mad::residual_key(t_row[j], p_row[j]);
        if (pass == 0) saw_nan = saw_nan || mad::key_is_nan(k);
        if (mad::in_prefix(k, prefix, pass)) atomicAdd(&hist[mad::digit_of(k, pass)], 1u);
      }
    }
    if (saw_nan) atomicOr(&any_nan_all[wave], 1u);
    __syncthreads();
    part[lane] = mad::sum_bins(hist + lane * mad::kPerLane, 1, mad::kPerLane);
    __syncthreads();
    if (lane == 0) mad::choose_digit(&sel_all[wave], pass, part, 1, mad::kWave, hist, 1, mad::kPerLane);
    __syncthreads();
    prefix = sel_all[wave].prefix;
    for (int b = lane; b < mad::kBins; b += mad::kWave) hist[b] = 0u;
    __syncthreads();
  }

  const mad::Sel s = sel_all[wave];
  if ((P & 1) == 0) {                                               // (m = P in every row)
    u64 mn = mad::kNoKey;
    if (active && mad::needs_next(s)) {
#pragma unroll 4
      for (int j = lane; j < P; j += mad::kWave) {
        const u64 k = mad::residual_key(t_row[j], p_row[j]);
        if (k > s.prefix && k < mn) mn = k;
      }
    }
    mins_all[wave][lane] = mn;
    __syncthreads();
  }
  if (lane == 0 && active) {
    u64 next = mad::kNoKey;
    if (mad::needs_next(s))
      for (int l = 0; l < mad::kWave; ++l) { const u64 v = mins_all[wave][l]; next = v < next ? v : next; }
    row_med[row] = mad::median_of(s, next, any_nan_all[wave] != 0u);
  }
}

}  // namespace

extern "C" int payne_mad_stats(int device, const float* pred, int ld_pred, const float* truth, int ld_truth, int N, int P,
                               const unsigned char* groups, int G, double* pix_med, double* row_med, void* stream) {
  if (!pred || !truth || !pix_med || N < 1 || P < 1 || ld_pred < P || ld_truth < P || G < 0 || (G > 0 && !groups))
    return PAYNE_E_INVALID;
  if (G > 65535) return PAYNE_E_UNSUPPORTED;                        // (the row sets are the grid's second dimension)
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(device) != hipSuccess) return PAYNE_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = PAYNE_OK;
  if (G > 0) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(payne_mad_cols_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kColsLds) != hipSuccess)
      rc = PAYNE_E_HIP;
    if (!rc) {
      const unsigned col_blocks = (unsigned)(((long long)P + mad::kCols - 1) / mad::kCols);
      hipLaunchKernelGGL(payne_mad_cols_kernel, dim3(col_blocks, (unsigned)G), dim3(mad::kThreads), kColsLds, st, pred, ld_pred, truth,
                         ld_truth, N, P, groups, pix_med);
      if (hipGetLastError() != hipSuccess) rc = PAYNE_E_HIP;
    }
  }
  if (!rc && row_med) {
    const unsigned row_blocks = (unsigned)(((long long)N + mad::kWaves - 1) / mad::kWaves);
    hipLaunchKernelGGL(payne_mad_rows_kernel, dim3(row_blocks), dim3(mad::kThreads), 0, st, pred, ld_pred, truth, ld_truth, N, P, row_med);
    if (hipGetLastError() != hipSuccess) rc = PAYNE_E_HIP;
  }
  if (hipStreamSynchronize(st) != hipSuccess) rc = PAYNE_E_HIP;
  (void)hipSetDevice(prev);
  return rc;
}
