// k_lnmlp_train.hip -- one training step of the photometric LayerNorm + SiLU networks (Payne/train/trainphot.py:411-447 on MLP_v0 /
// MLP_v1 of Payne/train/NNmodels_new.py): three launches.  The per-row arithmetic is lnmlp_train_core.hpp, which runs on the
// host too (tests/emul/lnmlp_train_emul.cpp).
//
//   payne_lnmlp_train_kernel   one 256-thread workgroup per 64 rows, k_lnmlp.hip's tile and LDS image: fp32 [64][stride].
//     Forward as payne_lnmlp_kernel (the same matrix steps in the same order: with no dropout the same bits); per hidden layer
//     x_hat, rstd and the block's output go to the handle's workspace as well.  The last layer's image becomes dY, the tile's
//     part of the loss goes to a slab.  Backward, from the last layer down: dA_in = dZ W is the forward's product on the
//     transposed stored copy of W; then four threads a row take the dropout / SiLU / LayerNorm backward in place, x_hat and
//     rstd read back from the workspace; dZ of every layer goes to the workspace; the tile's sums over its rows of dZ (db),
//     du x_hat (dgain) and du (dbeta) go to slabs [tiles][3][width], one thread a column, rows in index order.
//     One image serves activations and gradients in turn, so a width of 512 needs no second one.
//   payne_lnmlp_dw_kernel      dW_l = dZ_l^T A_{l-1} for every layer in one launch: one workgroup per 32 x 32 tile of dW, k = the
//     batch rows, two a matrix step, both operands read from the workspace (lanes 0..31: 32 consecutive floats of one row).
//     The rows go in groups of 16, dealt round-robin to the four waves; the waves' parts are added as (p0 + p1) + (p2 + p3).
//     A few hundred tiles at the default widths.
//   payne_lnmlp_update_kernel  sums the slabs over the tiles in index order, applies RAdam to every parameter and writes the
//     three copies of the weights (row-major, the forward's stored order, the transposed stored order).  Padding is never
//     touched and stays zero.
//   No atomics; every sum has a fixed order.  Rows of the last tile beyond N run as rows of zeros whose dY is zero.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "lnmlp_train_core.hpp"

using namespace payne;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// act[64][stride] (K = 8 KB inputs a row) times the stored weights w -> act[64][32 nct] (+ bias), in place: payne_lnmlp_kernel's
// layer product, the same matrix steps in the same order.  Ends behind a barrier.
template <int NT>
__device__ __forceinline__ void tile_product(float* act, int stride, const float* __restrict__ w, int KB, int nct,
                                             const float* __restrict__ bias, int lane, int wave) {
  const float* a_lo = act + (lane & 31) * stride + 4 * (lane >> 5);
  const float* a_hi = a_lo + lnmlp::kTile * stride;
  f32x16 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][h][i] = 0.0f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + lnmlp::kWaves * t;
    if (ct < nct) {
      const float* wp = w + lnmlp::packed_index(ct, 0, lane, 0, KB);
      f32x16 c0 = acc[t][0], c1 = acc[t][1];
      auto ld = [&](int kb, float4& lo, float4& hi, float4& wv) {
        lo = *reinterpret_cast<const float4*>(a_lo + kb * lnmlp::kKBlock);
        hi = *reinterpret_cast<const float4*>(a_hi + kb * lnmlp::kKBlock);
        wv = *reinterpret_cast<const float4*>(wp + (size_t)kb * (lnmlp::kWave * 4));
      };
      auto steps = [&](const float4& lo, const float4& hi, const float4& wv) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lo.x, wv.x, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hi.x, wv.x, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lo.y, wv.y, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hi.y, wv.y, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lo.z, wv.z, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hi.z, wv.z, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lo.w, wv.w, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hi.w, wv.w, c1, 0, 0, 0);
      };
      float4 plo, phi, pw, qlo, qhi, qw;
      ld(0, plo, phi, pw);
      for (int kb = 0; kb < KB; kb += 2) {                          // two blocks a turn, as in k_lnmlp.hip
        const bool two = kb + 1 < KB;
        ld(two ? kb + 1 : kb, qlo, qhi, qw);
        __builtin_amdgcn_sched_barrier(0);
        steps(plo, phi, pw);
        __builtin_amdgcn_sched_barrier(0);
        ld(kb + 2 < KB ? kb + 2 : kb, plo, phi, pw);
        __builtin_amdgcn_sched_barrier(0);
        if (two) steps(qlo, qhi, qw);
        __builtin_amdgcn_sched_barrier(0);
      }
      acc[t][0] = c0;
      acc[t][1] = c1;
    }
  }
  __syncthreads();                                                  // every wave has read the image it is about to overwrite
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + lnmlp::kWaves * t;
    if (ct < nct) {
      const int col = ct * lnmlp::kTile + (lane & 31);
      const float b = bias ? bias[col] : 0.0f;
      float* zc = act + 4 * (lane >> 5) * stride + col;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[t][h][i];
          zc[(h * lnmlp::kTile + (i & 3) + 8 * (i >> 2)) * stride] = bias ? v + b : v;
        }
    }
  }
  __syncthreads();
}

template <int NT>
__global__ void __launch_bounds__(lnmlp::kThreads) payne_lnmlp_train_kernel(const float* __restrict__ x, long long ld_x,
                                                                             const float* __restrict__ t, long long ld_t, int N,
                                                                             int stride, int train, unsigned long long seed,
                                                                             unsigned long long step, float scale,
                                                                             const lnmlp::TrainNet net) {
  extern __shared__ __attribute__((aligned(16))) float lnmlp_train_act[];
  float* act = lnmlp_train_act;
  double* row_loss = reinterpret_cast<double*>(act + lnmlp::kTileRows * stride);
  const int tid = threadIdx.x, lane = tid & (lnmlp::kWave - 1), wave = tid / lnmlp::kWave;
  const int tile = blockIdx.x;
  const long long row0 = (long long)tile * lnmlp::kTileRows;
  const int nl = net.n_layers;

  {  // the input, zeros beyond D_in and beyond N; kept as layer 0's A_in
    const int d_in = net.L[0].n_in, K0 = lnmlp::k_blocks(d_in) * lnmlp::kKBlock, w0 = lnmlp::pad32(d_in);
    for (int idx = tid; idx < lnmlp::kTileRows * K0; idx += lnmlp::kThreads) {
      const int r = idx / K0, k = idx - r * K0;
      float v = 0.0f;
      if (row0 + r < (long long)N && k < d_in) v = x[(size_t)(row0 + r) * (size_t)ld_x + (size_t)k];
      act[r * stride + k] = v;
      net.L[0].a_in[(size_t)(row0 + r) * (size_t)w0 + (size_t)k] = v;
    }
  }
  __syncthreads();

  const int part = tid & (lnmlp::kParts - 1), row = tid / lnmlp::kParts;
  const size_t grow = (size_t)(row0 + row);                         // this thread's row of the batch in the row passes
  float* zr = act + row * stride;

  // ---- forward ----
  for (int l = 0; l < nl; ++l) {
    const lnmlp::TrainLayer& L = net.L[l];
    const int npad = lnmlp::pad32(L.n_out), n = L.n_out;
    tile_product<NT>(act, stride, L.wp, lnmlp::k_blocks(L.n_in), lnmlp::col_tiles(n), L.vec, lane, wave);
    if (l + 1 == nl) break;
    float s = lnmlp::partial_sum(zr, part, n);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    const float mean = lnmlp::mean_of(s, n);
    float q = lnmlp::partial_sqdev(zr, part, n, mean);
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    const float rstd = lnmlp::rstd_of(q, n);
    if (part == 0) L.rs[grow] = rstd;
    const float p = train ? L.p : 0.0f;
    lnmlp::row_ln_silu_train(zr, part, n, mean, rstd, L.vec + npad, L.vec + 2 * npad, p, lnmlp::mask_stream(seed, step, l),
                             (int)grow, L.xh + grow * (size_t)npad, net.L[l + 1].a_in + grow * (size_t)npad);
    __syncthreads();
  }

  // ---- loss and dY ----
  {
    const lnmlp::TrainLayer& L = net.L[nl - 1];
    const int npad = lnmlp::pad32(L.n_out), n = L.n_out;
    if (tid < lnmlp::kTileRows) {
      float* yr = act + tid * stride;
      double acc = 0.0;
      if (row0 + tid < (long long)N) {
        acc = lnmlp::row_loss_grad(yr, t + (size_t)(row0 + tid) * (size_t)ld_t, n, scale);
      } else {
        for (int j = 0; j < n; ++j) yr[j] = 0.0f;
      }
      row_loss[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (int r = 0; r < lnmlp::kTileRows; ++r) acc += row_loss[r];
      net.loss_slab[tile] = acc;
    }
    if (!train) return;
    for (int idx = tid; idx < lnmlp::kTileRows * npad; idx += lnmlp::kThreads) {
      const int r = idx / npad, j = idx - r * npad;
      L.dz[(size_t)(row0 + r) * (size_t)npad + (size_t)j] = act[r * stride + j];
    }
    for (int j = tid; j < n; j += lnmlp::kThreads) {
      float sum = 0.0f;
      for (int r = 0; r < lnmlp::kTileRows; ++r) sum += act[r * stride + j];
      L.slab[((size_t)tile * 3 + 0) * (size_t)npad + (size_t)j] = sum;
    }
  }

  // ---- backward ----
  for (int l = nl - 1; l >= 1; --l) {
    const lnmlp::TrainLayer& L = net.L[l];
    const lnmlp::TrainLayer& P = net.L[l - 1];                      // the hidden block whose output this layer reads
    const int n = P.n_out, npad = lnmlp::pad32(n);
    tile_product<NT>(act, stride, L.wt, lnmlp::k_blocks(L.n_out), lnmlp::col_tiles(L.n_in), nullptr, lane, wave);
    const float* xh = P.xh + grow * (size_t)npad;
    const float* gain = P.vec + npad;
    float s1, s2;
    lnmlp::row_act_backward(zr, xh, gain, P.vec + 2 * npad, part, n, P.p, lnmlp::mask_stream(seed, step, l - 1), (int)grow, &s1, &s2);
    s1 += __shfl_xor(s1, 1);
    s1 += __shfl_xor(s1, 2);
    s2 += __shfl_xor(s2, 1);
    s2 += __shfl_xor(s2, 2);
    const float m1 = lnmlp::mean_of(s1, n), m2 = lnmlp::mean_of(s2, n);
    __syncthreads();
    for (int j = tid; j < n; j += lnmlp::kThreads) {                // dgain, dbeta of the tile
      float sg = 0.0f, sb = 0.0f;
      const float* xc = P.xh + (size_t)row0 * (size_t)npad + (size_t)j;
      for (int r = 0; r < lnmlp::kTileRows; ++r) {
        const float du = act[r * stride + j];
        sg = fmaf(du, xc[(size_t)r * (size_t)npad], sg);
        sb += du;
      }
      P.slab[((size_t)tile * 3 + 1) * (size_t)npad + (size_t)j] = sg;
      P.slab[((size_t)tile * 3 + 2) * (size_t)npad + (size_t)j] = sb;
    }
    __syncthreads();
    lnmlp::row_ln_backward(zr, xh, gain, part, n, P.rs[grow], m1, m2, P.dz + grow * (size_t)npad);
    __syncthreads();
    for (int j = tid; j < n; j += lnmlp::kThreads) {                // db of the tile
      float sum = 0.0f;
      for (int r = 0; r < lnmlp::kTileRows; ++r) sum += act[r * stride + j];
      P.slab[((size_t)tile * 3 + 0) * (size_t)npad + (size_t)j] = sum;
    }
  }
}

struct DwPlan {
  int first_tile[lnmlp::kMaxLayers + 1];                            // layer l owns the blocks first_tile[l] .. first_tile[l + 1] - 1
};

__global__ void __launch_bounds__(lnmlp::kThreads) payne_lnmlp_dw_kernel(int rows, const DwPlan plan, const lnmlp::TrainNet net) {
  __shared__ float part[lnmlp::kWaves][16][lnmlp::kWave];
  int l = 0;
  while ((int)blockIdx.x >= plan.first_tile[l + 1]) ++l;            // (the same in every lane)
  const lnmlp::TrainLayer& L = net.L[l];
  const int local = (int)blockIdx.x - plan.first_tile[l], kt = lnmlp::col_tiles(L.n_in);
  const int n0 = (local / kt) * lnmlp::kTile, k0 = (local % kt) * lnmlp::kTile;
  const int tid = threadIdx.x, lane = tid & (lnmlp::kWave - 1), wave = tid / lnmlp::kWave;
  const int ldz = lnmlp::pad32(L.n_out), lda = lnmlp::pad32(L.n_in);
  const float* dz = L.dz + (size_t)(lane >> 5) * (size_t)ldz + (size_t)(n0 + (lane & 31));
  const float* a = L.a_in + (size_t)(lane >> 5) * (size_t)lda + (size_t)(k0 + (lane & 31));
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  // wave w takes the 16-row groups w, w + 4, ... (rows is a multiple of 64); a group's operands are requested before the
  // matrix steps of the group before it are issued
  const int groups = rows / lnmlp::kDwGroup;
  float d[8], v[8], dn[8], vn[8];
  auto ld = [&](int g, float* dd, float* vv) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      dd[u] = dz[(size_t)(g * lnmlp::kDwGroup + 2 * u) * (size_t)ldz];
      vv[u] = a[(size_t)(g * lnmlp::kDwGroup + 2 * u) * (size_t)lda];
    }
  };
  if (wave < groups) ld(wave, d, v);
  for (int g = wave; g < groups; g += lnmlp::kWaves) {
    const int gn = g + lnmlp::kWaves < groups ? g + lnmlp::kWaves : g;
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
  for (int e = tid; e < 16 * lnmlp::kWave; e += lnmlp::kThreads) {  // the four waves' parts in a fixed order
    const int i = e / lnmlp::kWave, ln = e % lnmlp::kWave;
    const int n = n0 + (i & 3) + 8 * (i >> 2) + 4 * (ln >> 5), k = k0 + (ln & 31);
    if (n < L.n_out && k < L.n_in)
      L.gw[(size_t)n * (size_t)L.n_in + (size_t)k] = lnmlp::combine_parts(part[0][i][ln], part[1][i][ln], part[2][i][ln], part[3][i][ln]);
  }
}

__global__ void __launch_bounds__(256) payne_lnmlp_update_kernel(int tiles, const lnmlp::RadamStep rs, const lnmlp::TrainNet net) {
  const int l = blockIdx.y;
  const lnmlp::TrainLayer& L = net.L[l];
  const int npad = lnmlp::pad32(L.n_out), nw = L.n_in * L.n_out;
  const int n_vec = l + 1 == net.n_layers ? 1 : 3;                  // the output layer has a bias only
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nw + n_vec * npad; idx += gridDim.x * blockDim.x) {
    if (idx < nw) {
      const int n = idx / L.n_in, k = idx - n * L.n_in;
      const float w = lnmlp::radam_update(L.wm[idx], L.gw[idx], L.mw + idx, L.vw + idx, rs);
      L.wm[idx] = w;
      L.wp[lnmlp::packed_at(n, k, L.n_in)] = w;
      L.wt[lnmlp::packed_t_at(n, k, L.n_out)] = w;
    } else {
      const int which = (idx - nw) / npad, j = (idx - nw) - which * npad;
      if (j >= L.n_out) continue;
      float g = 0.0f;
      for (int t = 0; t < tiles; ++t) g += L.slab[((size_t)t * 3 + (size_t)which) * (size_t)npad + (size_t)j];
      const int o = which * npad + j;
      L.gvec[o] = g;
      L.vec[o] = lnmlp::radam_update(L.vec[o], g, L.mvec + o, L.vvec + o, rs);
    }
  }
}

// acc = (first ? 0 : acc) + the tiles' parts in index order; with denom > 0 also *out = acc / denom
__global__ void payne_lnmlp_loss_kernel(const double* __restrict__ slab, int tiles, double* acc, int first, double denom, double* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = first ? 0.0 : *acc;
  for (int t = 0; t < tiles; ++t) s += slab[t];
  *acc = s;
  if (denom > 0.0 && out) *out = s / denom;
}

template <int NT>
int launch_step(const lnmlp::TrainNet& net, const float* x, int ld_x, const float* t, int ld_t, int N, int train,
                unsigned long long seed, unsigned long long step, float scale, hipStream_t st) {
  const int stride = lnmlp::train_stride(net);
  const size_t lds = (size_t)lnmlp::kTileRows * (size_t)stride * sizeof(float) + lnmlp::kTileRows * sizeof(double);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(payne_lnmlp_train_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return PAYNE_E_HIP;
  const unsigned blocks = (unsigned)((N + lnmlp::kTileRows - 1) / lnmlp::kTileRows);
  hipLaunchKernelGGL(payne_lnmlp_train_kernel<NT>, dim3(blocks), dim3(lnmlp::kThreads), lds, st, x, (long long)ld_x, t, (long long)ld_t,
                     N, stride, train, seed, step, scale, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

}  // namespace

// Called by payne_lnmlp_train_step / _loss (payne_hip.hip) with checked arguments, 1 <= N <= the workspace's rows, on the handle's
// device.  Forward (+ backward with train != 0) of N rows; the tiles' parts of the loss are left in net.loss_slab.
int payne_lnmlp_train_launch(const lnmlp::TrainNet& net, const float* x, int ld_x, const float* t, int ld_t, int N, int train,
                             unsigned long long seed, unsigned long long step, float scale, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int max_ct = 0;
  for (int l = 0; l < net.n_layers; ++l) {
    const int c = lnmlp::col_tiles(net.L[l].n_out);
    max_ct = c > max_ct ? c : max_ct;
  }
  if (max_ct <= lnmlp::kWaves) return launch_step<1>(net, x, ld_x, t, ld_t, N, train, seed, step, scale, st);
  if (max_ct <= 2 * lnmlp::kWaves) return launch_step<2>(net, x, ld_x, t, ld_t, N, train, seed, step, scale, st);
  return launch_step<4>(net, x, ld_x, t, ld_t, N, train, seed, step, scale, st);
}

// The weight gradients of the N rows just passed and the RAdam update of every parameter.
int payne_lnmlp_train_update(const lnmlp::TrainNet& net, int N, const lnmlp::RadamStep& rs, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int tiles = (N + lnmlp::kTileRows - 1) / lnmlp::kTileRows;
  DwPlan plan;
  int total = 0, most = 0;
  for (int l = 0; l < lnmlp::kMaxLayers + 1; ++l) {
    plan.first_tile[l] = total;
    if (l < net.n_layers) {
      total += lnmlp::col_tiles(net.L[l].n_out) * lnmlp::col_tiles(net.L[l].n_in);
      const int count = net.L[l].n_in * net.L[l].n_out + 3 * lnmlp::pad32(net.L[l].n_out);
      most = count > most ? count : most;
    }
  }
  hipLaunchKernelGGL(payne_lnmlp_dw_kernel, dim3((unsigned)total), dim3(lnmlp::kThreads), 0, st, tiles * lnmlp::kTileRows, plan, net);
  if (hipGetLastError() != hipSuccess) return PAYNE_E_HIP;
  hipLaunchKernelGGL(payne_lnmlp_update_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)net.n_layers), dim3(256), 0, st, tiles, rs, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

int payne_lnmlp_train_loss_sum(const lnmlp::TrainNet& net, int N, double* acc, int first, double denom, double* out, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(payne_lnmlp_loss_kernel, dim3(1), dim3(1), 0, st, net.loss_slab, (N + lnmlp::kTileRows - 1) / lnmlp::kTileRows, acc,
                     first, denom, out);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}
