// k_specmlp_train.hip -- one training step of the spectral networks (Payne/train/trainspec.py:422-444 on SMLP / LinNet of
// Payne/train/NNmodels.py): five launches.  The per-row arithmetic is specmlp_train_core.hpp, which runs on the host too
// (tests/emul/specmlp_train_emul.cpp).  The matrix product is written here again rather than shared with k_lnmlp_train.hip:
// this unit's product has to run on through several passes of the image (tile_mac / tile_store), that unit stays as it is.
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
//   payne_specmlp_dw_kernel      dW_l = dZ_l^T A_{l-1} for every layer in one launch, payne_lnmlp_dw_kernel's scheme: one
//     workgroup per 32 x 32 tile of dW, k = the batch rows, 16-row groups dealt round-robin to the four waves, the parts added
//     as (p0 + p1) + (p2 + p3).  1280 tiles for an output layer of 4096 x 300.
//   payne_specmlp_update_kernel  sums the slabs over the tiles in index order, applies RAdam to every parameter and writes the
//     three copies of the weights.  Padding is never touched and stays zero.
//   No atomics; every sum has a fixed order.  Rows of the last tile beyond N run as rows of zeros whose dY is zero.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "specmlp_train_core.hpp"

using namespace payne;
namespace sp = payne::specmlp;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
struct TileAcc {
  f32x16 v[NT][2];
};

template <int NT>
__device__ __forceinline__ void tile_zero(TileAcc<NT>& acc) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc.v[t][h][i] = 0.0f;
}

// acc += act[64][8 nkb inputs a row] times the k-blocks kb0 .. kb0 + nkb - 1 of the stored weights w (KB k-blocks a column tile),
// wave `wave` on the column tiles wave, wave + 4, ... below nct: the matrix steps of k_lnmlp.hip's layer product in its order.
// Reads the image only; no barrier.
template <int NT>
__device__ __forceinline__ void tile_mac(TileAcc<NT>& acc, const float* act, int stride, const float* __restrict__ w, int KB, int kb0,
                                         int nkb, int nct, int lane, int wave) {
  const float* a_lo = act + (lane & 31) * stride + 4 * (lane >> 5);
  const float* a_hi = a_lo + sp::kTile * stride;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + sp::kWaves * t;
    if (ct < nct) {
      const float* wp = w + sp::packed_index(ct, kb0, lane, 0, KB);
      f32x16 c0 = acc.v[t][0], c1 = acc.v[t][1];
      auto ld = [&](int kb, float4& lo, float4& hi, float4& wv) {
        lo = *reinterpret_cast<const float4*>(a_lo + kb * sp::kKBlock);
        hi = *reinterpret_cast<const float4*>(a_hi + kb * sp::kKBlock);
        wv = *reinterpret_cast<const float4*>(wp + (size_t)kb * (sp::kWave * 4));
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
      for (int kb = 0; kb < nkb; kb += 2) {                         // two blocks a turn, as in k_lnmlp.hip
        const bool two = kb + 1 < nkb;
        ld(two ? kb + 1 : kb, qlo, qhi, qw);
        __builtin_amdgcn_sched_barrier(0);
        steps(plo, phi, pw);
        __builtin_amdgcn_sched_barrier(0);
        ld(kb + 2 < nkb ? kb + 2 : kb, plo, phi, pw);
        __builtin_amdgcn_sched_barrier(0);
        if (two) steps(qlo, qhi, qw);
        __builtin_amdgcn_sched_barrier(0);
      }
      acc.v[t][0] = c0;
      acc.v[t][1] = c1;
    }
  }
}

// The accumulators (+ bias) into the image, columns 32 ct .. of act[64][stride].  The caller puts a barrier before (every wave
// has read the image) and after.
template <int NT>
__device__ __forceinline__ void tile_store(const TileAcc<NT>& acc, float* act, int stride, int nct, const float* __restrict__ bias,
                                           int lane, int wave) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + sp::kWaves * t;
    if (ct < nct) {
      const int col = ct * sp::kTile + (lane & 31);
      const float b = bias ? bias[col] : 0.0f;
      float* zc = act + 4 * (lane >> 5) * stride + col;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc.v[t][h][i];
          zc[(h * sp::kTile + (i & 3) + 8 * (i >> 2)) * stride] = bias ? v + b : v;
        }
    }
  }
}

// act[64][stride] times the stored weights w -> act[64][32 nct] (+ bias), in place.  Ends behind a barrier.
template <int NT>
__device__ __forceinline__ void tile_product(float* act, int stride, const float* __restrict__ w, int KB, int nct,
                                             const float* __restrict__ bias, int lane, int wave) {
  TileAcc<NT> acc;
  tile_zero(acc);
  tile_mac<NT>(acc, act, stride, w, KB, 0, KB, nct, lane, wave);
  __syncthreads();                                                  // every wave has read the image it is about to overwrite
  tile_store<NT>(acc, act, stride, nct, bias, lane, wave);
  __syncthreads();
}

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
    tile_product<NT>(act, stride, L.wp, sp::k_blocks(L.n_in), sp::col_tiles(L.n_out), L.vec, lane, wave);
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
  TileAcc<1> acc;
  tile_zero(acc);
  if (ct < nct) {                                                   // (tile_mac's wave index: this wave's one column tile)
    tile_mac<1>(acc, act, stride, L.wp + sp::packed_index(ct, 0, 0, 0, KB), KB, 0, KB, 1, lane, 0);
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
    TileAcc<NT> acc;
    tile_zero(acc);
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
      tile_mac<NT>(acc, act, stride, L.wt, KB, kb0, nkb, nct, lane, wave);
    }
    __syncthreads();                                                // before the image is overwritten with the result
    tile_store<NT>(acc, act, stride, nct, nullptr, lane, wave);
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
    if (l > 0) tile_product<NT>(act, stride, L.wt, sp::k_blocks(L.n_out), sp::col_tiles(L.n_in), nullptr, lane, wave);
  }
}

// ---- launch 4: the weight gradients ----------------------------------------------------------------------------------------
struct DwPlan {
  int first_tile[sp::kMaxLayers + 1];                               // layer l owns the blocks first_tile[l] .. first_tile[l + 1] - 1
};

__global__ void __launch_bounds__(sp::kThreads) payne_specmlp_dw_kernel(int rows, const DwPlan plan, const sp::SpecNet net) {
  __shared__ float part[sp::kWaves][16][sp::kWave];
  int l = 0;
  while ((int)blockIdx.x >= plan.first_tile[l + 1]) ++l;            // (the same in every lane)
  const sp::SpecLayer& L = net.L[l];
  const int local = (int)blockIdx.x - plan.first_tile[l], kt = sp::col_tiles(L.n_in);
  const int n0 = (local / kt) * sp::kTile, k0 = (local % kt) * sp::kTile;
  const int tid = threadIdx.x, lane = tid & (sp::kWave - 1), wave = tid / sp::kWave;
  const int ldz = sp::pad32(L.n_out), lda = sp::pad32(L.n_in);
  const float* dz = L.dz + (size_t)(lane >> 5) * (size_t)ldz + (size_t)(n0 + (lane & 31));
  const float* a = L.a_in + (size_t)(lane >> 5) * (size_t)lda + (size_t)(k0 + (lane & 31));
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  // wave w takes the 16-row groups w, w + 4, ... (rows is a multiple of 64); a group's operands are requested before the
  // matrix steps of the group before it are issued
  const int groups = rows / sp::kDwGroup;
  float d[8], v[8], dn[8], vn[8];
  auto ld = [&](int g, float* dd, float* vv) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      dd[u] = dz[(size_t)(g * sp::kDwGroup + 2 * u) * (size_t)ldz];
      vv[u] = a[(size_t)(g * sp::kDwGroup + 2 * u) * (size_t)lda];
    }
  };
  if (wave < groups) ld(wave, d, v);
  for (int g = wave; g < groups; g += sp::kWaves) {
    const int gn = g + sp::kWaves < groups ? g + sp::kWaves : g;
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
  for (int e = tid; e < 16 * sp::kWave; e += sp::kThreads) {        // the four waves' parts in a fixed order
    const int i = e / sp::kWave, ln = e % sp::kWave;
    const int n = n0 + (i & 3) + 8 * (i >> 2) + 4 * (ln >> 5), k = k0 + (ln & 31);
    if (n < L.n_out && k < L.n_in)
      L.gw[(size_t)n * (size_t)L.n_in + (size_t)k] = sp::combine_parts(part[0][i][ln], part[1][i][ln], part[2][i][ln], part[3][i][ln]);
  }
}

// ---- launch 5: the update ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) payne_specmlp_update_kernel(int tiles, const sp::RadamStep rs, const sp::SpecNet net) {
  const int l = blockIdx.y;
  const sp::SpecLayer& L = net.L[l];
  const int npad = sp::pad32(L.n_out), nw = L.n_in * L.n_out;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nw + npad; idx += gridDim.x * blockDim.x) {
    if (idx < nw) {
      const int n = idx / L.n_in, k = idx - n * L.n_in;
      const float w = sp::radam_update(L.wm[idx], L.gw[idx], L.mw + idx, L.vw + idx, rs);
      L.wm[idx] = w;
      L.wp[sp::packed_at(n, k, L.n_in)] = w;
      L.wt[sp::packed_t_at(n, k, L.n_out)] = w;
    } else {
      const int j = idx - nw;
      if (j >= L.n_out) continue;
      float g = 0.0f;
      for (int t = 0; t < tiles; ++t) g += L.slab[(size_t)t * (size_t)npad + (size_t)j];
      L.gvec[j] = g;
      L.vec[j] = sp::radam_update(L.vec[j], g, L.mvec + j, L.vvec + j, rs);
    }
  }
}

// acc = (first ? 0 : acc) + the workgroups' parts in tile and chunk order; with out != NULL also *out = acc
__global__ void payne_specmlp_loss_kernel(const double* __restrict__ slab, int parts, double* acc, int first, double* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = first ? 0.0 : *acc;
  for (int t = 0; t < parts; ++t) s += slab[t];
  *acc = s;
  if (out) *out = s;
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

// Called by payne_specmlp_train_step / _loss / _predict (payne_hip.hip) with checked arguments, 1 <= N <= the workspace's rows,
// on the handle's device.  Launches 1 and 2: the forward of N rows; with t the workgroups' parts of the loss are left in
// net.loss_slab, with train != 0 dY and the output bias's parts in the workspace, with y the outputs in y [N][ld_y].
int payne_specmlp_train_forward(const sp::SpecNet& net, const float* x, int ld_x, const float* t, int ld_t, float* y, int ld_y, int N,
                                int train, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int m = hidden_tiles(net);
  int rc = m <= sp::kWaves ? launch_hidden<1>(net, x, ld_x, N, st)
                           : m <= 2 * sp::kWaves ? launch_hidden<2>(net, x, ld_x, N, st) : launch_hidden<4>(net, x, ld_x, N, st);
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
  const int m = hidden_tiles(net);
  int rc = m <= sp::kWaves ? launch_back<1>(net, N, st) : m <= 2 * sp::kWaves ? launch_back<2>(net, N, st) : launch_back<4>(net, N, st);
  if (rc) return rc;
  const int tiles = (N + sp::kTileRows - 1) / sp::kTileRows;
  DwPlan plan;
  int total = 0, most = 0;
  for (int l = 0; l < sp::kMaxLayers + 1; ++l) {
    plan.first_tile[l] = total;
    if (l < net.n_layers) {
      total += sp::col_tiles(net.L[l].n_out) * sp::col_tiles(net.L[l].n_in);
      most = sp::max_of(most, net.L[l].n_in * net.L[l].n_out + sp::pad32(net.L[l].n_out));
    }
  }
  hipLaunchKernelGGL(payne_specmlp_dw_kernel, dim3((unsigned)total), dim3(sp::kThreads), 0, st, tiles * sp::kTileRows, plan, net);
  if (hipGetLastError() != hipSuccess) return PAYNE_E_HIP;
  hipLaunchKernelGGL(payne_specmlp_update_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)net.n_layers), dim3(256), 0, st, tiles, rs, net);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

int payne_specmlp_train_loss_sum(const sp::SpecNet& net, int N, double* acc, int first, double* out, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int parts = (N + sp::kTileRows - 1) / sp::kTileRows * sp::out_chunks(net.L[net.n_layers - 1].n_out);
  hipLaunchKernelGGL(payne_specmlp_loss_kernel, dim3(1), dim3(1), 0, st, net.loss_slab, parts, acc, first, out);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}
