// k_lnmlp.hip -- payne_lnmlp_kernel: the photometric LayerNorm + SiLU networks of Payne/predict/photANN_new.py (MLP_v0, MLP_v1
// of Payne/train/NNmodels_new.py), every layer in one launch.  The per-row arithmetic is lnmlp_core.hpp, which runs on the
// host too (tests/emul/lnmlp_emul.cpp).
//
//   One 256-thread workgroup per 64 rows of x.  The rows' activations live in LDS, fp32 [64][stride], from the input
//   conversion to the last layer's output; stride = the widest padded row + 4 floats, so that the 16-byte operand reads of 16
//   rows and the 4-byte LayerNorm reads of 8 rows x 4 threads fall on different banks.
//   A layer: the product of the image with the layer's stored weights is mlp_tile.hpp's tile_product (wave w owns the 32-column
//   tiles w, w + 4, ..., NT of them at most, the template argument; a layer is at most 256 KiB, the same for every workgroup, so
//   it stays in L2).
//   After the last block: barrier (every wave has read the image), bias added and the tiles written over the image, barrier,
//   then four threads a row take LayerNorm's two sums over the row's true width and apply gain, bias and SiLU to every
//   fourth element in place, barrier.  After the last layer the image's first D_out columns go to y instead, through the
//   output conversion, rows below N only.
//   Rows of the last tile beyond N are evaluated as rows of zeros and not stored.  No atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "lnmlp_core.hpp"
#include "mlp_tile.hpp"

using namespace payne;

namespace {

template <int NT>
__global__ void __launch_bounds__(lnmlp::kThreads) payne_lnmlp_kernel(const double* __restrict__ x, long long ld_x, int N,
                                                                       float* __restrict__ y, long long ld_y, int stride,
                                                                       const lnmlp::NetArgs net) {
  extern __shared__ __attribute__((aligned(16))) float lnmlp_act[];
  float* act = lnmlp_act;
  const int tid = threadIdx.x, lane = tid & (lnmlp::kWave - 1), wave = tid / lnmlp::kWave;
  const long long row0 = (long long)blockIdx.x * lnmlp::kTileRows;

  {  // the input: fp64 -> (normalised) fp32, zeros beyond D_in and beyond N
    const int d_in = net.L[0].n_in, K0 = lnmlp::k_blocks(d_in) * lnmlp::kKBlock;
    for (int idx = tid; idx < lnmlp::kTileRows * K0; idx += lnmlp::kThreads) {
      const int r = idx / K0, k = idx - r * K0;
      float v = 0.0f;
      if (row0 + r < (long long)N && k < d_in)
        v = lnmlp::input_value(x[(size_t)(row0 + r) * (size_t)ld_x + (size_t)k], net.in_mid, net.in_std, k);
      act[r * stride + k] = v;
    }
  }
  __syncthreads();

  for (int l = 0; l < net.n_layers; ++l) {
    const lnmlp::LayerArgs L = net.L[l];
    const int KB = lnmlp::k_blocks(L.n_in), nct = lnmlp::col_tiles(L.n_out);
    const bool last = l + 1 == net.n_layers;
    mlp::tile_product<NT>(act, stride, L.w, KB, nct, L.b, lane, wave);

    if (last) {  // the image's first D_out columns to y through the output conversion, rows below N only
      const int n = L.n_out;
      for (int idx = tid; idx < lnmlp::kTileRows * n; idx += lnmlp::kThreads) {
        const int r = idx / n, j = idx - r * n;
        if (row0 + r < (long long)N)
          y[(size_t)(row0 + r) * (size_t)ld_y + (size_t)j] = lnmlp::output_value(act[r * stride + j], net.out_mid, net.out_std, j);
      }
      break;
    }

    {  // LayerNorm + SiLU in place: row tid / 4, every fourth element from tid % 4
      const int part = tid & (lnmlp::kParts - 1), n = L.n_out;
      float* zr = act + (tid / lnmlp::kParts) * stride;
      float s = lnmlp::partial_sum(zr, part, n);
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      const float mean = lnmlp::mean_of(s, n);
      float q = lnmlp::partial_sqdev(zr, part, n, mean);
      q += __shfl_xor(q, 1);
      q += __shfl_xor(q, 2);
      const float rstd = lnmlp::rstd_of(q, n);
      for (int j = part; j < n; j += lnmlp::kParts) zr[j] = lnmlp::ln_silu(zr[j], mean, rstd, L.gain[j], L.beta[j]);
    }
    __syncthreads();
  }
}

template <int NT>
int launch(const double* x, int ld_x, int N, float* y, int ld_y, const lnmlp::NetArgs& net, hipStream_t st) {
  const int stride = lnmlp::act_stride(net);
  const size_t lds = (size_t)lnmlp::kTileRows * (size_t)stride * sizeof(float);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(payne_lnmlp_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return PAYNE_E_HIP;
  const unsigned blocks = (unsigned)(((long long)N + lnmlp::kTileRows - 1) / lnmlp::kTileRows);
  hipLaunchKernelGGL(payne_lnmlp_kernel<NT>, dim3(blocks), dim3(lnmlp::kThreads), lds, st, x, (long long)ld_x, N, y, (long long)ld_y,
                     stride, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

}  // namespace

// Called by payne_lnmlp_eval (mlp_api.hip) with checked arguments, N >= 1, on the handle's device.
int payne_lnmlp_launch(const lnmlp::NetArgs& net, const double* x, int ld_x, int N, float* y, int ld_y, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int max_ct = 0;
  for (int l = 0; l < net.n_layers; ++l) {
    const int c = lnmlp::col_tiles(net.L[l].n_out);
    max_ct = c > max_ct ? c : max_ct;
  }
  return mlp::with_tiles_per_wave(max_ct, [&](auto nt) { return launch<decltype(nt)::value>(x, ld_x, N, y, ld_y, net, st); });
}
