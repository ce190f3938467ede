// mlp_train_tail.hpp -- the end of a training step, the same for the photometric and the spectral networks (k_lnmlp_train.hip on
// lnmlp::TrainNet, k_specmlp_train.hip on specmlp::SpecNet): the weight gradients, the RAdam update and the sum of the loss parts.
// What differs between the nets is Net::kHiddenVecs, the per-column vectors of a hidden layer (bias, LayerNorm gain and bias: 3;
// bias alone: 1), which is also the slabs' stride; the output layer has its bias only in both.
//   dw_kernel      dW_l = dZ_l^T A_{l-1} for every layer in one launch: one workgroup per 32 x 32 tile of dW, k = the batch rows, two
//     a matrix step, both operands read from the workspace (lanes 0..31: 32 consecutive floats of one row).  The rows go in groups
//     of 16, dealt round-robin to the four waves; the waves' parts are added as (p0 + p1) + (p2 + p3).
//   update_kernel  sums the slabs over the tiles in index order, applies RAdam to every parameter and writes the three copies of
//     the weights (row-major, the forward's stored order, the transposed stored order).  Padding is never touched and stays zero.
//   loss_kernel    one thread adds the workgroups' parts of the loss in index order.
//   No atomics; every sum has a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "lnmlp_train_core.hpp"
#include "mlp_tile.hpp"

namespace payne {
namespace mlp {

struct DwPlan {
  int first_tile[kMaxLayers + 1];                                   // layer l owns the blocks first_tile[l] .. first_tile[l + 1] - 1
};

template <class Net>
__global__ void __launch_bounds__(kThreads) payne_mlp_dw_kernel(int rows, const DwPlan plan, const Net net) {
  __shared__ float part[kWaves][16][kWave];
  int l = 0;
  while ((int)blockIdx.x >= plan.first_tile[l + 1]) ++l;            // (the same in every lane)
  const auto& L = net.L[l];
  const int local = (int)blockIdx.x - plan.first_tile[l], kt = col_tiles(L.n_in);
  const int n0 = (local / kt) * kTile, k0 = (local % kt) * kTile;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int ldz = pad32(L.n_out), lda = pad32(L.n_in);
  const float* dz = L.dz + (size_t)(lane >> 5) * (size_t)ldz + (size_t)(n0 + (lane & 31));
  const float* a = L.a_in + (size_t)(lane >> 5) * (size_t)lda + (size_t)(k0 + (lane & 31));
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  // wave w takes the 16-row groups w, w + 4, ... (rows is a multiple of 64); a group's operands are requested before the
  // matrix steps of the group before it are issued
  const int groups = rows / kDwGroup;
  float d[8], v[8], dn[8], vn[8];
  auto ld = [&](int g, float* dd, float* vv) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      dd[u] = dz[(size_t)(g * kDwGroup + 2 * u) * (size_t)ldz];
      vv[u] = a[(size_t)(g * kDwGroup + 2 * u) * (size_t)lda];
    }
  };
  if (wave < groups) ld(wave, d, v);
  for (int g = wave; g < groups; g += kWaves) {
    const int gn = g + kWaves < groups ? g + kWaves : g;
    ld(gn, dn, vn);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d[u], v[u], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      d[u] = dn[u];
      v[u] = vn[u];
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave][i][lane] = acc[i];
  __syncthreads();
  for (int e = tid; e < 16 * kWave; e += kThreads) {                // the four waves' parts in a fixed order
    const int i = e / kWave, ln = e % kWave;
    const int n = n0 + (i & 3) + 8 * (i >> 2) + 4 * (ln >> 5), k = k0 + (ln & 31);   // (the result map of acc_row)
    if (n < L.n_out && k < L.n_in)
      L.gw[(size_t)n * (size_t)L.n_in + (size_t)k] = combine_parts(part[0][i][ln], part[1][i][ln], part[2][i][ln], part[3][i][ln]);
  }
}

template <class Net>
__global__ void __launch_bounds__(256) payne_mlp_update_kernel(int tiles, const RadamStep rs, const Net net) {
  const int l = blockIdx.y;
  const auto& L = net.L[l];
  const int npad = pad32(L.n_out), nw = L.n_in * L.n_out;
  const int n_vec = l + 1 == net.n_layers ? 1 : Net::kHiddenVecs;   // the output layer has a bias only
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nw + n_vec * npad; idx += gridDim.x * blockDim.x) {
    if (idx < nw) {
      const int n = idx / L.n_in, k = idx - n * L.n_in;
      const float w = radam_update(L.wm[idx], L.gw[idx], L.mw + idx, L.vw + idx, rs);
      L.wm[idx] = w;
      L.wp[packed_at(n, k, L.n_in)] = w;
      L.wt[packed_t_at(n, k, L.n_out)] = w;
    } else {
      const int which = (idx - nw) / npad, j = (idx - nw) - which * npad;
      if (j >= L.n_out) continue;
      float g = 0.0f;
      for (int t = 0; t < tiles; ++t) g += L.slab[((size_t)t * Net::kHiddenVecs + (size_t)which) * (size_t)npad + (size_t)j];
      const int o = which * npad + j;
      L.gvec[o] = g;
      L.vec[o] = radam_update(L.vec[o], g, L.mvec + o, L.vvec + o, rs);
    }
  }
}

// acc = (first ? 0 : acc) + the parts in index order; with out != NULL also *out = acc, divided by denom where denom > 0
template <class Net>
__global__ void payne_mlp_loss_kernel(const double* __restrict__ slab, int parts, double* acc, int first, double denom, double* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = first ? 0.0 : *acc;
  for (int t = 0; t < parts; ++t) s += slab[t];
  *acc = s;
  if (out) *out = denom > 0.0 ? s / denom : s;
}

// The weight gradients of the N rows just passed and the RAdam update of every parameter.
template <class Net>
int launch_dw_update(const Net& net, int N, const RadamStep& rs, hipStream_t st) {
  const int tiles = (N + kTileRows - 1) / kTileRows;
  DwPlan plan;
  int total = 0, most = 0;
  for (int l = 0; l < kMaxLayers + 1; ++l) {
    plan.first_tile[l] = total;
    if (l < net.n_layers) {
      total += col_tiles(net.L[l].n_out) * col_tiles(net.L[l].n_in);
      const int count = net.L[l].n_in * net.L[l].n_out + Net::kHiddenVecs * pad32(net.L[l].n_out);
      most = count > most ? count : most;
    }
  }
  hipLaunchKernelGGL(payne_mlp_dw_kernel<Net>, dim3((unsigned)total), dim3(kThreads), 0, st, tiles * kTileRows, plan, net);
  if (hipGetLastError() != hipSuccess) return PAYNE_E_HIP;
  hipLaunchKernelGGL(payne_mlp_update_kernel<Net>, dim3((unsigned)((most + 255) / 256), (unsigned)net.n_layers), dim3(256), 0, st, tiles, rs, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

template <class Net>
int launch_loss_sum(const Net& net, int parts, double* acc, int first, double denom, double* out, hipStream_t st) {
  hipLaunchKernelGGL(payne_mlp_loss_kernel<Net>, dim3(1), dim3(1), 0, st, net.loss_slab, parts, acc, first, denom, out);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

}  // namespace mlp
}  // namespace payne
