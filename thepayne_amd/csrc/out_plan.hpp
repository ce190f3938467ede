// out_plan.hpp -- which kernel the output layer gets (plain C++: no device code, no HIP header; tests/test_out_plan.py builds it with
// g++ and checks it against the table of DESIGN section 1).  plan_out reads an OutFacts -- what a context knows of one of its nets --
// and the batch size, and names the kernel; payne_hip.hip's launch_out switches over that name and decides nothing.
#pragma once

#include <algorithm>

#include "../../include/payne_hip.h"

// payne_dense_big3_kernel's tile (dense_kernels.hpp); every other plane-operand and fp32-ring kernel works on 64 x 128 tiles
constexpr int B3_TM = 128, B3_TN = 256;

// The forms, each falling back to the one before it: the generic tile kernel | fp32 operands by LDS-DMA | three bf16 planes an
// operand, six products (equal hidden widths) | two fp16 planes, three products (activations calibrated on the label box).
enum class OutForm { Generic, F32Dma, Bf16x3, H2 };
// What the variant bits ask for; payne_ctx_create builds the fp16 planes for OutForm::H2 only.
static inline OutForm wanted_out_form(unsigned variant) {
  if (variant & PAYNE_V_OUT_GENERIC) return OutForm::Generic;
  if (variant & (PAYNE_V_OUT_F32 | PAYNE_V_OUT_BK64)) return OutForm::F32Dma;
  if (variant & (PAYNE_V_OUT_BF16X3 | PAYNE_V_OUT_PLANES)) return OutForm::Bf16x3;
  return OutForm::H2;
}

// One instantiation each (the template arguments as DESIGN's table spells them).
enum class OutKernel {
  GenericFused,      // payne_dense_kernel<64, 64, 32, true>: a two-layer net, labels and first layer fused in
  Generic,           // payne_dense_kernel<64, 64, 32, false>
  Dma32Nk10Ns4,      // payne_dense_dma_kernel<4, 32, 10, 4, true>
  Dma32Ns4,          // payne_dense_dma_kernel<4, 32, 0, 4, true>
  Dma32Ns3,          // payne_dense_dma_kernel<4, 32, 0, 3, false>
  Dma64Nk5,          // payne_dense_dma_kernel<4, 64, 5, 3, true>
  Dma64,             // payne_dense_dma_kernel<4, 64, 0, 3, true>
  Big3H2,            // payne_dense_big3_kernel<true>
  Big3,              // payne_dense_big3_kernel<false>
  Dma2hh5,           // payne_dense_dma2hh_kernel<5>
  Dma2h5x64,         // payne_dense_dma2h_kernel<5, 64>
  Dma2h10x32,        // payne_dense_dma2h_kernel<10, 32>
  Dma2h0x32,         // payne_dense_dma2h_kernel<0, 32>
  Dma3f10,           // payne_dense_dma3f_kernel<10>
  Dma3Nk10Ns4,       // payne_dense_dma3_kernel<10, 4, true>
  Dma3Ns4,           // payne_dense_dma3_kernel<0, 4, true>
  Dma3Ns2            // payne_dense_dma3_kernel<0, 2, false>
};

// What plan_out reads: the context's constants, one of its nets, and which operand sets were built.
struct OutFacts {
  unsigned variant = 0;
  int n_cu = 256, b_max = 0, ld_hid = 0, w_out_kp = 0, n1 = 0;
  int n_layers = 0, n_out = 0;        // the net: its layers and the output layer's rows
  bool spectral = false;              // the spectral net owns the operand copies (the continuum network: Generic)
  bool freq = false, sel = false;     // rows go out in the frequency domain; ... as rows of the resampled grid (n1 values) with the pixel fall-back
  bool dma_ok = false;                // hidden widths all equal: the activations' pad columns are zero
  float act_scale = 0.f;              // the last hidden layer's calibrated power of two (0: none)
  bool p3 = false;                    // three bf16 planes: the pixel rows' weights and the activations' buffer
  bool h2 = false, h2_freq = false;   // two fp16 planes of the pixel rows' weights / of the rows in the frequency domain
  bool pad = false, pad_freq = false; // the padded fp32 weights of either set
};

struct OutPlan {
  OutForm form = OutForm::Generic;
  OutKernel kernel = OutKernel::Generic;
  int grid_m = 0, grid_n = 0;         // tiles of the launch (64 x 128; Big3*: 128 x 256), every form but Generic
  bool sel = false;                   // rows of the resampled grid, or pixel rows if the batch's records say so
};

// The output layer's form whatever domain the rows go out in (rows in the frequency domain need Bf16x3 or better).
static inline OutForm out_form(const OutFacts& f) {
  OutForm o = wanted_out_form(f.variant);
  if (!(f.spectral && f.dma_ok && f.ld_hid >= f.w_out_kp)) return OutForm::Generic;       // hidden widths differ, the continuum network
  if (o >= OutForm::Bf16x3 && !f.p3) o = OutForm::F32Dma;
  if (o == OutForm::H2) {
    // (payne_dense_dma2h_kernel addresses an operand plane by 32-bit byte offsets: rows x pitch x 2 bytes below 2^31)
    const unsigned long long plane_w = 2ull * (unsigned long long)std::max(f.n_out, f.n1) * (unsigned long long)f.w_out_kp;
    const unsigned long long plane_x = 2ull * (unsigned long long)f.b_max * (unsigned long long)f.ld_hid;
    if (plane_w >= (1ull << 31) || plane_x >= (1ull << 31) || !f.h2 || !(f.act_scale > 0.f)) o = OutForm::Bf16x3;
  }
  return o;
}

// The output layer's kernel for a batch of B: every variant bit and every shape that bears on it is tested here and in out_form.
static inline OutPlan plan_out(const OutFacts& f, int B) {
  const unsigned v = f.variant;
  OutPlan o; o.sel = f.sel;
  const int n_launch = o.sel ? f.n1 : f.n_out;              // (rows of the resampled grid: n1 values)
  o.form = out_form(f);
  if (o.form == OutForm::H2 && f.freq && !f.h2_freq) o.form = OutForm::Bf16x3;
  if (o.form == OutForm::Generic) { o.kernel = f.n_layers == 2 ? OutKernel::GenericFused : OutKernel::Generic; return o; }
  o.grid_m = (B + 63) / 64; o.grid_n = (n_launch + 127) / 128;
  const bool own_cu = o.grid_m * o.grid_n <= f.n_cu;        // a compute unit for every tile: the deep / pipelined schedules
  const bool fixed = f.w_out_kp == 320 && !(v & PAYNE_V_OUT_ROLLED);   // 300-wide nets: the k-steps of the 320 padded columns counted at compile time
  if (o.form == OutForm::F32Dma) {
    if (f.w_out_kp % 64 == 0 && (v & PAYNE_V_OUT_BK64)) o.kernel = fixed ? OutKernel::Dma64Nk5 : OutKernel::Dma64;    // three 64-deep stages
    else if (own_cu) o.kernel = fixed ? OutKernel::Dma32Nk10Ns4 : OutKernel::Dma32Ns4;          // the pipelined schedule, four stages
    else o.kernel = OutKernel::Dma32Ns3;                    // many tiles per CU: two workgroups per CU, the plain schedule
    return o;
  }
  const bool h2 = o.form == OutForm::H2;
  // many whole 128 x 256 tiles (C5): persistent workgroups.  Everything else one 64 x 128 tile a workgroup -- whatever the batch, the
  // same products in the same order: a candidate's rows do not depend on how many others share its batch.
  if (B % B3_TM == 0 && n_launch % B3_TN == 0 && (B / B3_TM) * (n_launch / B3_TN) >= 2 * f.n_cu && !(v & PAYNE_V_OUT_SMALL_TILES) && !o.sel) {
    o.kernel = h2 ? OutKernel::Big3H2 : OutKernel::Big3;
    o.grid_m = B / B3_TM; o.grid_n = n_launch / B3_TN;
    return o;
  }
  if (h2) {
    // 300-wide nets: five 64-deep steps when every tile has a compute unit to itself (finished in two halves, the left half's rows
    // leaving under the right half's products, unless the whole tile is asked for), ten 32-deep ones otherwise; other widths, and
    // PAYNE_V_OUT_ROLLED: 32-deep steps counted at run time.  Same products in the same order in all four.
    if (!fixed) o.kernel = OutKernel::Dma2h0x32;
    else if (!own_cu) o.kernel = OutKernel::Dma2h10x32;
    else o.kernel = (v & PAYNE_V_OUT_WHOLE_TILE) ? OutKernel::Dma2h5x64 : OutKernel::Dma2hh5;
    return o;
  }
  // Bf16x3, one tile per CU at most, 300-wide: the weights as fp32 through the port, split into the planes on their way into LDS
  const bool split_w = fixed && own_cu && (f.freq ? f.pad_freq : f.pad) && !(v & PAYNE_V_OUT_PLANES) && (!o.sel || f.pad);
  if (!own_cu) o.kernel = OutKernel::Dma3Ns2;
  else if (split_w) o.kernel = OutKernel::Dma3f10;
  else o.kernel = fixed ? OutKernel::Dma3Nk10Ns4 : OutKernel::Dma3Ns4;
  return o;
}
