// lnmlp_train_core.hpp -- arithmetic of payne_lnmlp_train_step (k_lnmlp_train.hip): one training step of the photometric
// LayerNorm + SiLU networks as Payne/train/trainphot.py takes it (:343 MSELoss(reduction='mean'), :353 torch.optim.RAdam,
// :411-447 forward / backward / step) on MLP_v0 / MLP_v1 of Payne/train/NNmodels_new.py.  Written host/device like
// lnmlp_core.hpp, whose forward it reuses (dot_packed, the LayerNorm sums): the same source runs in the kernels and on the
// host (tests/emul/lnmlp_train_emul.cpp, also under ASan / UBSan).
//   forward   lnmlp_core.hpp's, in training mode: x_hat = (z - mean) * rstd and rstd are kept per hidden layer, and after the
//             SiLU of a block that carries a dropout a *= keep ? 1 / (1 - p) : 0.  With every p = 0 the bits are payne_lnmlp_eval's.
//   mask      keep(seed, step, layer, row, column, p): a counter-based hash, no state; 24 uniform bits compared with p.
//   loss      mean((y - t)^2): the fp32 residuals squared and summed in fp64, per row, then the rows of a 64-row tile, then
//             the tiles, each in index order.
//   backward  fp32.  dY = (y - t) * 2 / (N D_out); per Linear dW = dZ^T A_in (four fmaf chains, chain c over the 16-row groups
//             c, c + 4, ... of the batch in index order, added as (c0 + c1) + (c2 + c3)), db = sum_rows dZ, dA_in = dZ W
//             (dot_packed on the transposed stored copy); through dropout the forward's factor; SiLU: du = da s (1 + u (1 - s));
//             LayerNorm: dx_hat = du gain, dz = rstd (dx_hat - mean(dx_hat) - x_hat mean(dx_hat x_hat)), the two row means by
//             kParts threads in lnmlp_core.hpp's order; dgain = sum_rows du x_hat, dbeta = sum_rows du.  Sums over rows: the
//             rows of a tile in index order, then the tiles in index order.
//   RAdam     torch.optim.RAdam (betas, eps, no weight decay); what depends on t alone is computed on the host in fp64
//             (radam_scalars), as torch computes it in Python floats.
#pragma once
#include <stdint.h>

#include "lnmlp_core.hpp"

namespace payne {
namespace lnmlp {

constexpr int kDwGroup = 16;                     // rows of the batch a wave of the weight-gradient pass takes at a time

PAYNE_LNMLP_HD int pad32(int n) { return col_tiles(n) * kTile; }

// ---- dropout mask ---------------------------------------------------------------------------------------------------
PAYNE_LNMLP_HD uint64_t mix64(uint64_t z) {                       // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the part of the hash that is the same for a whole launch
PAYNE_LNMLP_HD uint64_t mask_stream(unsigned long long seed, unsigned long long step, int layer) {
  return mix64(mix64((uint64_t)seed + 0x9E3779B97F4A7C15ull * ((uint64_t)step + 1u)) ^ ((uint64_t)(uint32_t)layer + 1u));
}
PAYNE_LNMLP_HD bool keep_of(uint64_t stream, int row, int col, float p) {
  const uint64_t h = mix64(stream ^ (((uint64_t)(uint32_t)row << 32) | (uint64_t)(uint32_t)col));
  return (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f) >= p;  // 24 bits: exact in fp32
}
// Is the output `column` of hidden block `layer` kept in row `row` of the batch of step `step` (0 for a handle's first)?
PAYNE_LNMLP_HD bool keep(unsigned long long seed, unsigned long long step, int layer, int row, int col, float p) {
  return !(p > 0.0f) || keep_of(mask_stream(seed, step, layer), row, col, p);
}
PAYNE_LNMLP_HD float drop_factor(bool kept, float p) { return kept ? 1.0f / (1.0f - p) : 0.0f; }

// ---- forward, training mode -----------------------------------------------------------------------------------------
// Thread `part` of a row after the row's sums: x_hat to xh, LayerNorm + SiLU (+ dropout) in place and to a_out.
PAYNE_LNMLP_HD void row_ln_silu_train(float* zr, int part, int n, float mean, float rstd, const float* gain, const float* beta,
                                      float p, uint64_t stream, int row, float* xh, float* a_out) {
  for (int j = part; j < n; j += kParts) {
    const float z = zr[j];
    float a = ln_silu(z, mean, rstd, gain[j], beta[j]);
    if (p > 0.0f) a *= drop_factor(keep_of(stream, row, j, p), p);
    xh[j] = (z - mean) * rstd;
    zr[j] = a;
    a_out[j] = a;
  }
}

// ---- loss -----------------------------------------------------------------------------------------------------------
// One row: the fp32 residuals y - t squared and summed in fp64 in column order; y becomes dY = (y - t) * scale.
PAYNE_LNMLP_HD double row_loss_grad(float* y, const float* t, int d_out, float scale) {
  double acc = 0.0;
  for (int j = 0; j < d_out; ++j) {
    const float r = y[j] - t[j];
    acc += (double)r * (double)r;
    y[j] = r * scale;
  }
  return acc;
}
PAYNE_LNMLP_HD float loss_grad_scale(int N, int d_out) { return (float)(2.0 / ((double)N * (double)d_out)); }

// ---- backward -------------------------------------------------------------------------------------------------------
PAYNE_LNMLP_HD float silu_grad(float da, float u) {
  const float s = 1.0f / (1.0f + expf(-u));
  return da * s * (1.0f + u * (1.0f - s));
}
// Thread `part` of a row: d holds dA (the gradient behind the dropout), becomes du; the thread's parts of sum(dx_hat) and
// sum(dx_hat x_hat) in partial_sum's order.
PAYNE_LNMLP_HD void row_act_backward(float* d, const float* xh, const float* gain, const float* beta, int part, int n, float p,
                                     uint64_t stream, int row, float* s1, float* s2) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int i = 0;
  for (int j = part; j < n; j += kParts, ++i) {
    const float x = xh[j], g = gain[j];
    float da = d[j];
    if (p > 0.0f) da *= drop_factor(keep_of(stream, row, j, p), p);
    const float du = silu_grad(da, x * g + beta[j]);
    d[j] = du;
    const float dx = du * g;
    a[i & 3] += dx;
    b[i & 3] = fmaf(dx, x, b[i & 3]);
  }
  *s1 = (a[0] + a[1]) + (a[2] + a[3]);
  *s2 = (b[0] + b[1]) + (b[2] + b[3]);
}
// Thread `part` of a row: d holds du, becomes dz (also written to dz_out); m1, m2 the row means of dx_hat and dx_hat x_hat.
PAYNE_LNMLP_HD void row_ln_backward(float* d, const float* xh, const float* gain, int part, int n, float rstd, float m1, float m2,
                                    float* dz_out) {
  for (int j = part; j < n; j += kParts) {
    const float dz = rstd * (d[j] * gain[j] - m1 - xh[j] * m2);
    d[j] = dz;
    dz_out[j] = dz;
  }
}

// ---- RAdam ----------------------------------------------------------------------------------------------------------
struct RadamStep {
  float beta1, one_m_beta1, beta2, one_m_beta2, eps;
  float step1;                                                    // lr / (1 - beta1^t)
  float adapt;                                                    // the rectification term times sqrt(1 - beta2^t)
  int rect;                                                       // rho_t > 5
};
inline RadamStep radam_scalars(double lr, double beta1, double beta2, double eps, long long t) {
  const double b1t = pow(beta1, (double)t), b2t = pow(beta2, (double)t);
  const double bc1 = 1.0 - b1t, bc2 = 1.0 - b2t;
  const double rho_inf = 2.0 / (1.0 - beta2) - 1.0, rho_t = rho_inf - 2.0 * (double)t * b2t / bc2;
  RadamStep s;
  s.beta1 = (float)beta1;
  s.one_m_beta1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.one_m_beta2 = (float)(1.0 - beta2);
  s.eps = (float)eps;
  s.step1 = (float)(lr / bc1);
  s.rect = rho_t > 5.0;
  s.adapt = s.rect ? (float)(sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) * sqrt(bc2)) : 0.0f;
  return s;
}
PAYNE_LNMLP_HD float radam_update(float p, float g, float* m, float* v, const RadamStep& s) {
  const float mm = fmaf(s.beta1, *m, s.one_m_beta1 * g);
  const float vv = fmaf(s.beta2, *v, s.one_m_beta2 * g * g);
  *m = mm;
  *v = vv;
  return s.rect ? p - s.step1 * mm * s.adapt / (sqrtf(vv) + s.eps) : p - s.step1 * mm;
}

// Where W[n][k] ([n_out][n_in]) lives in the two stored copies: the forward's (pack_weights) and the transposed one, which is
// pack_weights of W^T and gives dA_in = dZ W through dot_packed.
PAYNE_LNMLP_HD size_t packed_at(int n, int k, int n_in) {
  return packed_index(n / kTile, k / kKBlock, (n % kTile) + 32 * ((k % kKBlock) / 4), k % 4, k_blocks(n_in));
}
PAYNE_LNMLP_HD size_t packed_t_at(int n, int k, int n_out) { return packed_at(k, n, n_out); }

// ---- one layer of the step as the kernels see it (device pointers; host pointers in the emulator) -----------------------
// vec, gvec, mvec, vvec: [3][pad32(n_out)] = bias, LayerNorm gain, LayerNorm bias (the last two unused on the output layer);
// a_in: the layer's input [rows][pad32(n_in)]; xh, dz: [rows][pad32(n_out)]; rs: [rows]; slab: [tiles][3][pad32(n_out)], a
// tile's sums over its rows of dz, du x_hat, du.  rows = tiles * 64.
struct TrainLayer {
  float *wm, *wp, *wt, *vec;
  float *gw, *gvec;
  float *mw, *vw, *mvec, *vvec;
  float *a_in, *xh, *rs, *dz, *slab;
  int n_in, n_out;
  float p;                                                        // dropout after this block, 0 = none
};
struct TrainNet {
  static constexpr int kHiddenVecs = 3;                           // per-column vectors of a hidden layer; the slabs' stride
  int n_layers;
  TrainLayer L[kMaxLayers];
  double* loss_slab;                                              // [tiles]
};
PAYNE_LNMLP_HD int train_stride(const TrainNet& net) {
  int m = k_blocks(net.L[0].n_in) * kKBlock;
  for (int l = 0; l < net.n_layers; ++l) {
    const int p = pad32(net.L[l].n_out);
    m = p > m ? p : m;
  }
  return pad32(m) + kRowPad;
}

}  // namespace lnmlp
}  // namespace payne
