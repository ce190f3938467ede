// k_lnmlp_train.hip -- one training step of the photometric LayerNorm + SiLU networks (Payne/train/trainphot.py:411-447 on MLP_v0 /
// MLP_v1 of Payne/train/NNmodels_new.py): three launches.  The per-row arithmetic is lnmlp_train_core.hpp, which runs on the
// host too (tests/emul/lnmlp_train_emul.cpp).  The matrix product is mlp_tile.hpp's.
//
//   payne_lnmlp_train_kernel   one 256-thread workgroup per 64 rows, k_lnmlp.hip's tile and LDS image: fp32 [64][stride].
//     Forward as payne_lnmlp_kernel (the same matrix steps in the same order: with no dropout the same bits); per hidden layer
//     x_hat, rstd and the block's output go to the handle's workspace as well.  The last layer's image becomes dY, the tile's
//     part of the loss goes to a slab.  Backward, from the last layer down: dA_in = dZ W is the forward's product on the
//     transposed stored copy of W; then four threads a row take the dropout / SiLU / LayerNorm backward in place, x_hat and
//     rstd read back from the workspace; dZ of every layer goes to the workspace; the tile's sums over its rows of dZ (db),
//     du x_hat (dgain) and du (dbeta) go to slabs [tiles][3][width], one thread a column, rows in index order.
//     One image serves activations and gradients in turn, so a width of 512 needs no second one.
//   payne_mlp_dw_kernel, payne_mlp_update_kernel   the weight gradients of every layer in one launch (a few hundred 32 x 32 tiles
//     at the default widths), then the slabs' sums, RAdam and the three copies of the weights: mlp_train_tail.hpp.
//   No atomics; every sum has a fixed order.  Rows of the last tile beyond N run as rows of zeros whose dY is zero.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "lnmlp_train_core.hpp"
#include "mlp_tile.hpp"
#include "mlp_train_tail.hpp"

using namespace payne;

namespace {

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
    mlp::tile_product<NT>(act, stride, L.wp, lnmlp::k_blocks(L.n_in), lnmlp::col_tiles(n), L.vec, lane, wave);
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
    mlp::tile_product<NT>(act, stride, L.wt, lnmlp::k_blocks(L.n_out), lnmlp::col_tiles(L.n_in), nullptr, lane, wave);
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

// Called by payne_lnmlp_train_step / _loss (mlp_api.hip) with checked arguments, 1 <= N <= the workspace's rows, on the handle's
// device.  Forward (+ backward with train != 0) of N rows; the tiles' parts of the loss are left in net.loss_slab.
int payne_lnmlp_train_launch(const lnmlp::TrainNet& net, const float* x, int ld_x, const float* t, int ld_t, int N, int train,
                             unsigned long long seed, unsigned long long step, float scale, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int max_ct = 0;
  for (int l = 0; l < net.n_layers; ++l) {
    const int c = lnmlp::col_tiles(net.L[l].n_out);
    max_ct = c > max_ct ? c : max_ct;
  }
  return mlp::with_tiles_per_wave(max_ct, [&](auto nt) { return launch_step<decltype(nt)::value>(net, x, ld_x, t, ld_t, N, train, seed, step, scale, st); });
}

// The weight gradients of the N rows just passed and the RAdam update of every parameter.
int payne_lnmlp_train_update(const lnmlp::TrainNet& net, int N, const lnmlp::RadamStep& rs, void* stream) {
  return mlp::launch_dw_update(net, N, rs, reinterpret_cast<hipStream_t>(stream));
}

// acc = (first ? 0 : acc) + the tiles' parts of the N rows just passed; with out != NULL also *out = acc / denom
int payne_lnmlp_train_loss_sum(const lnmlp::TrainNet& net, int N, double* acc, int first, double denom, double* out, void* stream) {
  return mlp::launch_loss_sum(net, (N + lnmlp::kTileRows - 1) / lnmlp::kTileRows, acc, first, denom, out, reinterpret_cast<hipStream_t>(stream));
}
