// k_specjac.hip -- the spectral networks' output together with its Jacobian with respect to the labels (payne_specjac_eval), and
// the Fisher matrices of rows of such derivatives (payne_fisher_batch).  The arithmetic is specjac_core.hpp, which runs on the
// host too (tests/emul/specjac_emul.cpp).  The matrix product is mlp_tile.hpp's; this unit has the bias added to a tile's primal
// rows only.
//
//   payne_specjac_hidden_kernel  one 256-thread workgroup per S = 64 / (1 + D_in) stars, k_lnmlp.hip's tile and LDS image: fp32
//     [64][stride].  Row m * S + s is star s's primal (m = 0: the encoded labels) or its tangent of label m - 1 (the unit vector), so
//     the 1 + D_in rows of a star pass every layer's weights in one product, fetched once.  Per hidden layer the product (+ bias on
//     the rows below S), then one thread a (star, unit): a = act(z) and the star's D_in tangents times act'(z), in place.  The
//     image behind the last activation goes to the workspace.
//   payne_specjac_out_kernel     the output layer, thousands of columns wide: grid (tiles) x (chunks of 128 columns = four waves x
//     one 32-column tile), k_specmlp_train.hip's output launch.  The epilogue writes y = acc + b from the primal rows and
//     acc * scale_k from the tangent rows, inside N stars and D_out columns only.
//   payne_fisher_kernel          one workgroup a star; thread (i, j), i <= j, adds the pixels in index order in fp64; the K rows
//     pass the image 256 pixels at a time.
//   No atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "specjac_core.hpp"
#include "mlp_tile.hpp"

using namespace payne;
namespace sj = payne::specjac;

namespace {

// ---- launch 1: the hidden layers, primal and tangents ------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(sj::kThreads) payne_specjac_hidden_kernel(const double* __restrict__ x, long long ld_x, int N, int stride,
                                                                            const sj::JacNet net) {
  extern __shared__ __attribute__((aligned(16))) float specjac_act[];
  float* act = specjac_act;
  const int tid = threadIdx.x, lane = tid & (sj::kWave - 1), wave = tid / sj::kWave;
  const int d_in = net.L[0].n_in, S = sj::stars_per_tile(d_in);
  const long long star0 = (long long)blockIdx.x * S;
  for (int idx = tid; idx < sj::kTileRows * sj::kKBlock; idx += sj::kThreads) {     // the input image [64][8]
    const int r = idx / sj::kKBlock, k = idx - r * sj::kKBlock, m = r / S;
    const long long star = star0 + (r - m * S);
    float v = 0.0f;
    if (m <= d_in && star < (long long)N) v = sj::input_value(m, k, d_in, x + (size_t)star * (size_t)ld_x, net.xmin, net.xmax);
    act[r * stride + k] = v;
  }
  __syncthreads();
  for (int l = 0; l + 1 < net.n_layers; ++l) {
    const sj::JacLayer& L = net.L[l];
    mlp::tile_product<NT>(act, stride, L.w, sj::k_blocks(L.n_in), sj::col_tiles(L.n_out), L.b, lane, wave, S);
    for (int idx = tid; idx < S * L.n_out; idx += sj::kThreads) {   // one thread a (star, unit); the padding columns stay zero
      const int s = idx / L.n_out, j = idx - s * L.n_out;
      sj::unit_forward(act + s * stride + j, act + (S + s) * stride + j, S * stride, d_in, net.act);
    }
    __syncthreads();
  }
  {  // the image behind the last activation: [64][pad32(H)] to the workspace, 16 bytes a thread
    const int kpad = sj::pad32(net.L[net.n_layers - 1].n_in), q = kpad / 4;
    float* dst = net.a_last + (size_t)blockIdx.x * sj::kTileRows * (size_t)kpad;
    for (int idx = tid; idx < sj::kTileRows * q; idx += sj::kThreads) {
      const int r = idx / q, c = idx - r * q;
      *reinterpret_cast<float4*>(dst + (size_t)r * (size_t)kpad + 4 * c) = *reinterpret_cast<const float4*>(act + r * stride + 4 * c);
    }
  }
}

// ---- launch 2: the output layer ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(sj::kThreads) payne_specjac_out_kernel(float* __restrict__ y, long long ld_y, float* __restrict__ jac,
                                                                         long long ld_j, int N, int stride, const sj::JacNet net) {
  extern __shared__ __attribute__((aligned(16))) float specjac_out[];
  float* act = specjac_out;
  const sj::JacLayer& L = net.L[net.n_layers - 1];
  const int tid = threadIdx.x, lane = tid & (sj::kWave - 1), wave = tid / sj::kWave;
  const int d_in = net.L[0].n_in, d_out = L.n_out, kpad = sj::pad32(L.n_in), KB = sj::k_blocks(L.n_in);
  {  // the tile's image from the workspace
    const int q = kpad / 4;
    const float* src = net.a_last + (size_t)blockIdx.x * sj::kTileRows * (size_t)kpad;
    for (int idx = tid; idx < sj::kTileRows * q; idx += sj::kThreads) {
      const int r = idx / q, c = idx - r * q;
      *reinterpret_cast<float4*>(act + r * stride + 4 * c) = *reinterpret_cast<const float4*>(src + (size_t)r * (size_t)kpad + 4 * c);
    }
  }
  __syncthreads();
  const int ct = blockIdx.y * sj::kWaves + wave;
  if (ct >= sj::col_tiles(d_out)) return;
  mlp::TileAcc<1> acc;
  mlp::tile_zero(acc);
  mlp::tile_mac<1>(acc, act, stride, L.w + sj::packed_index(ct, 0, 0, 0, KB), KB, 0, KB, 1, lane, 0);   // (this wave's one column tile)
  const int col = ct * sj::kTile + (lane & 31);
  if (col >= d_out) return;
  const float b = L.b[col];
  const long long star0 = (long long)blockIdx.x * sj::stars_per_tile(d_in);
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      sj::store_output(acc.v[0][h][i], mlp::acc_row(h, i, lane), d_in, star0, N, col, b, net.scale, y, ld_y, jac, ld_j);
}

// ---- Fisher matrices -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(sj::kThreads) payne_fisher_kernel(const float* __restrict__ rows, long long ld, int K, int n,
                                                                    const double* __restrict__ w, double* __restrict__ F) {
  __shared__ float img[sj::kMaxFisherRows * (sj::kFisherChunk + 1)];
  __shared__ double wl[sj::kFisherChunk];
  const int tid = threadIdx.x, i = tid / K, j = tid - i * K;
  const bool mine = i < K && i <= j;
  const float* src = rows + (size_t)blockIdx.x * (size_t)K * (size_t)ld;
  const float* ri = img + (mine ? i : 0) * (sj::kFisherChunk + 1);
  const float* rj = img + (mine ? j : 0) * (sj::kFisherChunk + 1);
  double acc = 0.0;
  for (int c0 = 0; c0 < n; c0 += sj::kFisherChunk) {
    const int cw = n - c0 < sj::kFisherChunk ? n - c0 : sj::kFisherChunk;
    if (c0 > 0) __syncthreads();                                    // the chunk before has been read
    for (int idx = tid; idx < K * sj::kFisherChunk; idx += sj::kThreads) {
      const int r = idx / sj::kFisherChunk, p = idx - r * sj::kFisherChunk;
      if (p < cw) img[r * (sj::kFisherChunk + 1) + p] = src[(size_t)r * (size_t)ld + (size_t)(c0 + p)];
    }
    if (tid < cw) wl[tid] = w[c0 + tid];
    __syncthreads();
    if (mine)
      for (int p = 0; p < cw; ++p) {
        const double wv = wl[p];
        if (wv != 0.0) acc = sj::fisher_term(ri[p], rj[p], wv, acc);
      }
  }
  if (mine) {
    double* Fb = F + (size_t)blockIdx.x * (size_t)K * (size_t)K;
    Fb[i * K + j] = acc;
    Fb[j * K + i] = acc;
  }
}

template <int NT>
int prepare_hidden(size_t lds) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(payne_specjac_hidden_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds) == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

template <int NT>
int launch_hidden(const sj::JacNet& net, const double* x, int ld_x, int N, int stride, size_t lds, hipStream_t st) {
  const unsigned blocks = (unsigned)sj::tiles_of(N, net.L[0].n_in);
  hipLaunchKernelGGL(payne_specjac_hidden_kernel<NT>, dim3(blocks), dim3(sj::kThreads), lds, st, x, (long long)ld_x, N, stride, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

// the widest hidden layer's column tiles
int hidden_tiles(const sj::JacNet& net) {
  int m = 0;
  for (int l = 0; l + 1 < net.n_layers; ++l) m = sj::max_of(m, sj::col_tiles(net.L[l].n_out));
  return m;
}
size_t hidden_lds(const sj::JacNet& net) { return (size_t)sj::kTileRows * (size_t)sj::jac_hidden_stride(net) * sizeof(float); }
size_t out_lds(const sj::JacNet& net) { return (size_t)sj::kTileRows * (size_t)sj::jac_out_stride(net) * sizeof(float); }

}  // namespace

// Called once by payne_specjac_create on the handle's device: the two kernels this network launches may use their images' LDS.
int payne_specjac_prepare(const sj::JacNet& net) {
  const size_t lds = hidden_lds(net);
  const int rc = mlp::with_tiles_per_wave(hidden_tiles(net), [&](auto nt) { return prepare_hidden<decltype(nt)::value>(lds); });
  if (rc) return rc;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(payne_specjac_out_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)out_lds(net)) == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

// Called by payne_specjac_eval (mlp_api.hip) with checked arguments, 1 <= N <= the stars the workspace holds, on the handle's
// device: y [N][ld_y] (or NULL) and jac [N][D_in][ld_j] of the N stars x [N][ld_x].
int payne_specjac_launch(const sj::JacNet& net, const double* x, int ld_x, int N, float* y, int ld_y, float* jac, int ld_j, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int stride = sj::jac_hidden_stride(net);
  const size_t lds = hidden_lds(net);
  const int rc = mlp::with_tiles_per_wave(hidden_tiles(net), [&](auto nt) { return launch_hidden<decltype(nt)::value>(net, x, ld_x, N, stride, lds, st); });
  if (rc) return rc;
  const dim3 grid((unsigned)sj::tiles_of(N, net.L[0].n_in), (unsigned)sj::out_chunks(net.L[net.n_layers - 1].n_out));
  hipLaunchKernelGGL(payne_specjac_out_kernel, grid, dim3(sj::kThreads), out_lds(net), st, y, (long long)ld_y, jac, (long long)ld_j, N,
                     sj::jac_out_stride(net), net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

// Called by payne_fisher_batch with checked arguments, B >= 1, on the caller's device.
int payne_fisher_launch(const float* rows, int ld, int K, int n, int B, const double* w, double* F, void* stream) {
  hipLaunchKernelGGL(payne_fisher_kernel, dim3((unsigned)B), dim3(sj::kThreads), 0, reinterpret_cast<hipStream_t>(stream), rows,
                     (long long)ld, K, n, w, F);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}
