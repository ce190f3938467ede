// k_specmlp_train.hip -- one training step of the spectral networks (Payne/train/trainspec.py:422-444 on SMLP / LinNet of
// Payne/train/NNmodels.py): five launches.  The per-row arithmetic is specmlp_train_core.hpp, which runs on the host too
// (tests/emul/specmlp_train_emul.cpp).  The matrix product is mlp_tile.hpp's; the backward launch runs one product on through
// several passes of the image (tile_mac / tile_store).  Launches 4 and 5 are mlp_train_tail.hpp's.
//
//   payne_specmlp_hidden_kernel  one 256-thread workgroup per 64 rows, k_lnmlp.hip's tile and LDS image: fp32 [64][stride].
//     Per hidden layer the product + bias, then the activation, four threads a row; the block's output goes to the workspace
//     as the next layer's A_in.
//   payne_specmlp_out_kernel     the output layer, thousands of columns wide: grid (64-row tiles) x (chunks of 128 columns =
//     four waves x one 32-column tile).  The tile's A_last is read into LDS once; Y = A_last W_out^T + b; per element inside N
//     and D_out r = y - t, dY = 2 r to the workspace (and Y to the caller's buffer when asked); elements outside write dY = 0.
//     The workgroup's sum of r^2 goes in fp64 to its own slab entry; its dY passes the image once more and one thread a column
//     sums the 64 rows in index order: the bias gradient's part.
//   payne_specmlp_back_kernel    one workgroup per 64 rows.  dA_last = dY W_out has K = pad32(D_out): dY passes the image in
//     chunks of at most 512 columns, the accumulators stay in registers across the chunks (at most 4 column tiles a wave x 2
//     halves), the product runs on the transposed stored copy.  Then from the top hidden layer down: the activation's backward
//     in place, dZ_l to the workspace, the tile's column sums to slabs, dA_{l-1} = dZ_l W_l.
//   payne_mlp_dw_kernel          dW_l = dZ_l^T A_{l-1} for every layer in one launch (mlp_train_tail.hpp): 1280 tiles for an output
//     layer of 4096 x 300.
//   payne_mlp_update_kernel      the slabs' sums, RAdam and the three copies of the weights (mlp_train_tail.hpp).
//   No atomics; every sum has a fixed order.  Rows of the last tile beyond N run as rows of zeros whose dY is zero.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "specmlp_train_core.hpp"
#include "mlp_tile.hpp"
#include "mlp_train_tail.hpp"

using namespace payne;
namespace sp = payne::specmlp;

namespace {

// ---- launch 1: the hidden layers' forward --------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(sp::kThreads) payne_specmlp_hidden_kernel(const float* __restrict__ x, long long ld_x, int N, int stride,
                                                                            const sp::SpecNet net) {
  extern __shared__ __attribute__((aligned(16))) float specmlp_act[];
  float* act = specmlp_act;
  const int tid = threadIdx.x, lane = tid & (sp::kWave - 1), wave = tid / sp::kWave;
  const long long row0 = (long long)blockIdx.x * sp::kTileRows;
  {  // the encoded input, zeros beyond D_in and beyond N; kept as layer 0's A_in
    const int d_in = net.L[0].n_in, K0 = sp::k_blocks(d_in) * sp::kKBlock, w0 = sp::pad32(d_in);
    for (int idx = tid; idx < sp::kTileRows * K0; idx += sp::kThreads) {
      const int r = idx / K0, k = idx - r * K0;
      float v = 0.0f;
      if (row0 + r < (long long)N && k < d_in) v = x[(size_t)(row0 + r) * (size_t)ld_x + (size_t)k];
      act[r * stride + k] = v;
      net.L[0].a_in[(size_t)(row0 + r) * (size_t)w0 + (size_t)k] = v;
    }
  }
  __syncthreads();
  const int part = tid & (sp::kParts - 1), row = tid / sp::kParts;
  const size_t grow = (size_t)(row0 + row);
  float* zr = act + row * stride;
  for (int l = 0; l + 1 < net.n_layers; ++l) {
    const sp::SpecLayer& L = net.L[l];
    mlp::tile_product<NT>(act, stride, L.wp, sp::k_blocks(L.n_in), sp::col_tiles(L.n_out), L.vec, lane, wave);
    sp::row_act_forward(zr, part, L.n_out, net.act, net.L[l + 1].a_in + grow * (size_t)sp::pad32(L.n_out));
    __syncthreads();
  }
}

// ---- launch 2: the output layer, the loss and dY ---------------------------------------------------------------------------
// t == NULL: Y only (payne_specmlp_train_predict).  train == 0: no dY, no bias part.
__global__ void __launch_bounds__(sp::kThreads) payne_specmlp_out_kernel(const float* __restrict__ t, long long ld_t, float* __restrict__ y,
                                                                         long long ld_y, int N, int stride, int train, float scale,
                                                                         const sp::SpecNet net) {
  extern __shared__ __attribute__((aligned(16))) float specmlp_out[];
  float* act = specmlp_out;
  double* part_loss = reinterpret_cast<double*>(act + sp::kTileRows * stride);
  const sp::SpecLayer& L = net.L[net.n_layers - 1];
  const int tid = threadIdx.x, lane = tid & (sp::kWave - 1), wave = tid / sp::kWave;
  const int tile = blockIdx.x, chunk = blockIdx.y;
  const long long row0 = (long long)tile * sp::kTileRows;
  const int d_out = L.n_out, npad = sp::pad32(d_out), kpad = sp::pad32(L.n_in), KB = sp::k_blocks(L.n_in);
  {  // A_last of the tile: [64][kpad] from the workspace (padding columns are zero there), 16 bytes a thread
    const int q = kpad / 4;
    const float* src = L.a_in + (size_t)row0 * (size_t)kpad;
    for (int idx = tid; idx < sp::kTileRows * q; idx += sp::kThreads) {
      const int r = idx / q, c = idx - r * q;
      *reinterpret_cast<float4*>(act + r * stride + 4 * c) = *reinterpret_cast<const float4*>(src + (size_t)r * (size_t)kpad + 4 * c);
    }
  }
  __syncthreads();
  const int ct = chunk * sp::kWaves + wave, nct = sp::col_tiles(d_out);
  mlp::TileAcc<1> acc;
  mlp::tile_zero(acc);
  if (ct < nct) {                                                   // (tile_mac's wave index: this wave's one column tile)
    mlp::tile_mac<1>(acc, act, stride, L.wp + sp::packed_index(ct, 0, 0, 0, KB), KB, 0, KB, 1, lane, 0);
  }
  __syncthreads();                                                  // A_last has been read; the image now takes the chunk's dY
  double sq = 0.0;
  if (ct < nct) {
    const int col = ct * sp::kTile + (lane & 31), lc = wave * sp::kTile + (lane & 31);
    const bool col_in = col < d_out;
    const float b = col_in ? L.vec[col] : 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = h * sp::kTile + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        const long long gr = row0 + r;
        float dy = 0.0f;
        if (col_in && gr < (long long)N) {
          const float yv = acc.v[0][h][i] + b;
          if (y) y[(size_t)gr * (size_t)ld_y + (size_t)col] = yv;
          if (t) dy = sp::elem_loss_grad(yv, t[(size_t)gr * (size_t)ld_t + (size_t)col], scale, &sq);
        }
        if (train) {
          L.dz[(size_t)gr * (size_t)npad + (size_t)col] = dy;
          act[r * stride + lc] = dy;
        }
      }
  }
  if (!t) return;
  part_loss[tid] = sq;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < sp::kThreads; ++i) s += part_loss[i];
    net.loss_slab[(size_t)tile * gridDim.y + chunk] = s;
  }
  if (!train) return;
  if (tid < sp::kOutChunk) {                                        // db's part: one thread a column, the tile's rows in index order
    const int col = chunk * sp::kOutChunk + tid;
    if (col < d_out) {
      float sum = 0.0f;
      for (int r = 0; r < sp::kTileRows; ++r) sum += act[r * stride + tid];
      L.slab[(size_t)tile * (size_t)npad + (size_t)col] = sum;
    }
  }
}

// ---- launch 3: backward through the hidden layers --------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(sp::kThreads) payne_specmlp_back_kernel(int stride, const sp::SpecNet net) {
  extern __shared__ __attribute__((aligned(16))) float specmlp_back[];
  float* act = specmlp_back;
  const int tid = threadIdx.x, lane = tid & (sp::kWave - 1), wave = tid / sp::kWave;
  const int tile = blockIdx.x, nl = net.n_layers;
  const size_t row0 = (size_t)tile * sp::kTileRows;
  {  // dA_last = dY W_out: dY through the image in chunks of at most 512 columns, one chain across the chunks
    const sp::SpecLayer& L = net.L[nl - 1];
    const int npad = sp::pad32(L.n_out), KB = sp::k_blocks(L.n_out), nct = sp::col_tiles(L.n_in);   // (dY is zero beyond D_out)
    mlp::TileAcc<NT> acc;
    mlp::tile_zero(acc);
    for (int c0 = 0; c0 < npad; c0 += sp::kBackChunk) {
      const int cw = npad - c0 < sp::kBackChunk ? npad - c0 : sp::kBackChunk, q = cw / 4;
      if (c0 > 0) __syncthreads();                                  // the chunk before has been read
      const float* src = L.dz + row0 * (size_t)npad + (size_t)c0;
      for (int idx = tid; idx < sp::kTileRows * q; idx += sp::kThreads) {
        const int r = idx / q, c = idx - r * q;
        *reinterpret_cast<float4*>(act + r * stride + 4 * c) = *reinterpret_cast<const float4*>(src + (size_t)r * (size_t)npad + 4 * c);
      }
      __syncthreads();
      const int kb0 = c0 / sp::kKBlock, nkb = KB - kb0 < cw / sp::kKBlock ? KB - kb0 : cw / sp::kKBlock;
      mlp::tile_mac<NT>(acc, act, stride, L.wt, KB, kb0, nkb, nct, lane, wave);
    }
    __syncthreads();                                                // before the image is overwritten with the result
    mlp::tile_store<NT>(acc, act, stride, nct, nullptr, lane, wave);
    __syncthreads();
  }
  const int part = tid & (sp::kParts - 1), row = tid / sp::kParts;
  const size_t grow = row0 + (size_t)row;
  float* zr = act + row * stride;
  for (int l = nl - 2; l >= 0; --l) {
    const sp::SpecLayer& L = net.L[l];
    const int n = L.n_out, npad = sp::pad32(n);
    sp::row_act_backward(zr, net.L[l + 1].a_in + grow * (size_t)npad, part, n, net.act, L.dz + grow * (size_t)npad);
    __syncthreads();
    for (int j = tid; j < n; j += sp::kThreads) {                   // db of the tile
      float sum = 0.0f;
      for (int r = 0; r < sp::kTileRows; ++r) sum += act[r * stride + j];
      L.slab[(size_t)tile * (size_t)npad + (size_t)j] = sum;
    }
    if (l > 0) mlp::tile_product<NT>(act, stride, L.wt, sp::k_blocks(L.n_out), sp::col_tiles(L.n_in), nullptr, lane, wave);
  }
}

template <int NT>
int launch_hidden(const sp::SpecNet& net, const float* x, int ld_x, int N, hipStream_t st) {
  const int stride = sp::hidden_stride(net, false);
  const size_t lds = (size_t)sp::kTileRows * (size_t)stride * sizeof(float);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(payne_specmlp_hidden_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return PAYNE_E_HIP;
  const unsigned blocks = (unsigned)((N + sp::kTileRows - 1) / sp::kTileRows);
  hipLaunchKernelGGL(payne_specmlp_hidden_kernel<NT>, dim3(blocks), dim3(sp::kThreads), lds, st, x, (long long)ld_x, N, stride, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

template <int NT>
int launch_back(const sp::SpecNet& net, int N, hipStream_t st) {
  const int stride = sp::hidden_stride(net, true);
  const size_t lds = (size_t)sp::kTileRows * (size_t)stride * sizeof(float);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(payne_specmlp_back_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return PAYNE_E_HIP;
  const unsigned blocks = (unsigned)((N + sp::kTileRows - 1) / sp::kTileRows);
  hipLaunchKernelGGL(payne_specmlp_back_kernel<NT>, dim3(blocks), dim3(sp::kThreads), lds, st, stride, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

int hidden_tiles(const sp::SpecNet& net) {
  int m = 0;
  for (int l = 0; l + 1 < net.n_layers; ++l) m = sp::max_of(m, sp::col_tiles(net.L[l].n_out));
  return m;
}

}  // namespace

// Called by payne_specmlp_train_step / _loss / _predict (mlp_api.hip) with checked arguments, 1 <= N <= the workspace's rows,
// on the handle's device.  Launches 1 and 2: the forward of N rows; with t the workgroups' parts of the loss are left in
// net.loss_slab, with train != 0 dY and the output bias's parts in the workspace, with y the outputs in y [N][ld_y].
int payne_specmlp_train_forward(const sp::SpecNet& net, const float* x, int ld_x, const float* t, int ld_t, float* y, int ld_y, int N,
                                int train, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = mlp::with_tiles_per_wave(hidden_tiles(net), [&](auto nt) { return launch_hidden<decltype(nt)::value>(net, x, ld_x, N, st); });
  if (rc) return rc;
  const int stride = sp::out_stride(net);
  const size_t lds = (size_t)sp::kTileRows * (size_t)stride * sizeof(float) + sp::kThreads * sizeof(double);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(payne_specmlp_out_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return PAYNE_E_HIP;
  const dim3 grid((unsigned)((N + sp::kTileRows - 1) / sp::kTileRows), (unsigned)sp::out_chunks(net.L[net.n_layers - 1].n_out));
  hipLaunchKernelGGL(payne_specmlp_out_kernel, grid, dim3(sp::kThreads), lds, st, t, (long long)ld_t, y, (long long)ld_y, N, stride, train,
                     sp::kLossGradScale, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

// Launches 3 to 5 for the N rows just passed with train != 0.
int payne_specmlp_train_backward(const sp::SpecNet& net, int N, const sp::RadamStep& rs, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = mlp::with_tiles_per_wave(hidden_tiles(net), [&](auto nt) { return launch_back<decltype(nt)::value>(net, N, st); });
  return rc ? rc : mlp::launch_dw_update(net, N, rs, st);
}

// acc = (first ? 0 : acc) + the workgroups' parts of the N rows just passed, in tile and chunk order; with out != NULL also *out = acc
int payne_specmlp_train_loss_sum(const sp::SpecNet& net, int N, double* acc, int first, double* out, void* stream) {
  const int parts = (N + sp::kTileRows - 1) / sp::kTileRows * sp::out_chunks(net.L[net.n_layers - 1].n_out);
  return mlp::launch_loss_sum(net, parts, acc, first, 0.0, out, reinterpret_cast<hipStream_t>(stream));
}
