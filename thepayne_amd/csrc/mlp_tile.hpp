// mlp_tile.hpp -- the 64-row matrix product of the MLP kernels (k_lnmlp.hip, k_lnmlp_train.hip, k_specmlp_train.hip, k_specjac.hip),
// device only.  A 256-thread workgroup holds 64 rows of activations in LDS, fp32 act[64][stride]; wave w owns the 32-column tiles
// w, w + 4, ... of the product (NT of them at most) for both 32-row halves: 2 NT accumulators of v_mfma_f32_32x32x2_f32, exact
// fp32, one tile column after the other.  Per block of 8 inputs a lane reads 16 bytes of each half's activations from LDS and 16
// bytes of the tile's weights from global memory (lnmlp_core.hpp's stored order), four matrix steps on each half; the blocks go
// two a turn, each one's operands requested before the other's matrix steps are issued, so a load has eight matrix steps to
// arrive behind.  The *_core.hpp headers do not include this one: they compile on the host too.
#pragma once
#include <type_traits>

#include "lnmlp_core.hpp"

namespace payne {
namespace mlp {

using namespace payne::lnmlp;

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
struct TileAcc {
  f32x16 v[NT][2];
};

// Column tiles a wave of a hidden launch: 1, 2 or 4, from the widest layer's column tiles.
inline int tiles_per_wave(int widest_col_tiles) { return widest_col_tiles <= kWaves ? 1 : widest_col_tiles <= 2 * kWaves ? 2 : 4; }
// f(std::integral_constant<int, NT>) for NT = tiles_per_wave(widest_col_tiles)
template <class F>
int with_tiles_per_wave(int widest_col_tiles, F&& f) {
  const int nt = tiles_per_wave(widest_col_tiles);
  return nt == 1 ? f(std::integral_constant<int, 1>{}) : nt == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 4>{});
}

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
// wave `wave` on the column tiles wave, wave + 4, ... below nct.  Reads the image only; no barrier.
// w carries no __restrict__ on purpose: with it the compiler moves block Q's weight load past the sched_barriers into the
// `if (two)` branch, right in front of its use, and every turn waits for a global load (5 % of payne_lnmlp_kernel's time).
template <int NT>
__device__ __forceinline__ void tile_mac(TileAcc<NT>& acc, const float* act, int stride, const float* w, int KB, int kb0,
                                         int nkb, int nct, int lane, int wave) {
  // this lane's operand rows: row (lane & 31) of either half, inputs 4 (lane >> 5) .. + 3 of a block
  const float* a_lo = act + (lane & 31) * stride + 4 * (lane >> 5);
  const float* a_hi = a_lo + kTile * stride;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + kWaves * t;
    if (ct < nct) {                                                 // (the same in every lane of the wave)
      const float* wp = w + packed_index(ct, kb0, lane, 0, KB);
      f32x16 c0 = acc.v[t][0], c1 = acc.v[t][1];
      auto ld = [&](int kb, float4& lo, float4& hi, float4& wv) {
        lo = *reinterpret_cast<const float4*>(a_lo + kb * kKBlock);
        hi = *reinterpret_cast<const float4*>(a_hi + kb * kKBlock);
        wv = *reinterpret_cast<const float4*>(wp + (size_t)kb * (kWave * 4));
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
      for (int kb = 0; kb < nkb; kb += 2) {                         // two blocks a turn, P and Q
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

// The tile row of accumulator element i of half h in this lane (the matrix instruction's result map: column on the lane, rows in
// the registers)
__device__ __forceinline__ int acc_row(int h, int i, int lane) { return h * kTile + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); }

// The accumulators into the image, columns 32 ct .. of act[64][stride]; bias (may be NULL) is added to the tile rows below
// bias_rows.  The caller puts a barrier before (every wave has read the image) and after.  One pointer a column tile, indexed by
// the compile-time part of acc_row times stride: with the row formed per element the NT = 4 kernels run out of registers.
template <int NT>
__device__ __forceinline__ void tile_store(const TileAcc<NT>& acc, float* act, int stride, int nct, const float* __restrict__ bias,
                                           int lane, int wave, int bias_rows = kTileRows) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ct = wave + kWaves * t;
    if (ct < nct) {
      const int col = ct * kTile + (lane & 31);
      const float b = bias ? bias[col] : 0.0f;
      float* zc = act + 4 * (lane >> 5) * stride + col;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc.v[t][h][i];
          zc[acc_row(h, i, 0) * stride] = bias && acc_row(h, i, lane) < bias_rows ? v + b : v;
        }
    }
  }
}

// act[64][stride] times the stored weights w -> act[64][32 nct] (+ bias on the rows below bias_rows), in place.  Ends behind a
// barrier.
template <int NT>
__device__ __forceinline__ void tile_product(float* act, int stride, const float* w, int KB, int nct,
                                             const float* __restrict__ bias, int lane, int wave, int bias_rows = kTileRows) {
  TileAcc<NT> acc;
  tile_zero(acc);
  tile_mac<NT>(acc, act, stride, w, KB, 0, KB, nct, lane, wave);
  __syncthreads();                                                  // every wave has read the image it is about to overwrite
  tile_store<NT>(acc, act, stride, nct, bias, lane, wave, bias_rows);
  __syncthreads();
}

}  // namespace mlp
}  // namespace payne
