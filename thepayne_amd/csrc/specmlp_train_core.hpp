// specmlp_train_core.hpp -- arithmetic of payne_specmlp_train_step (k_specmlp_train.hip): one training step of the spectral
// networks as Payne/train/trainspec.py takes it (:319 MSELoss(reduction='sum'), :328 torch.optim.RAdam, :422-444 forward /
// backward / step) on SMLP and LinNet of Payne/train/NNmodels.py.  Written host/device like lnmlp_train_core.hpp, whose
// constants, weight packing (pack_weights, packed_index, packed_at, pad32, k_blocks, col_tiles), RAdam rule (radam_scalars,
// radam_update) and part-combining order it reuses: the same source runs in the kernels and on the host
// (tests/emul/specmlp_train_emul.cpp, also under ASan / UBSan).
//   input     the rows arrive encoded ((x - xmin) / (xmax - xmin) - 0.5 in fp64, rounded once to fp32: NNmodels.py:109-113).
//   forward   fp32.  A hidden block is Linear (dot_packed's fmaf chain in the matrix instruction's k order, + bias) followed by
//             LeakyReLU(0.01) (SMLP) or a sigmoid (LinNet); the output layer is Linear alone.  Each block's output activation
//             is kept; it alone serves the backward: LeakyReLU's slope is 1 where a > 0, else 0.01 (torch's rule, z == 0
//             included); the sigmoid's derivative is a (1 - a).
//   loss      sum((y - t)^2): the fp32 residuals squared and summed in fp64; per (64-row tile, 128-column chunk) one part, a
//             thread's 32 elements first, the 256 threads in index order, then the parts in tile and chunk order.
//   backward  fp32.  dY = (y - t) * 2; per Linear dW = dZ^T A_in (lnmlp_train_core.hpp's four chains), db = sum_rows dZ (the
//             rows of a tile in index order, then the tiles in index order), dA_in = dZ W (dot_packed on the transposed
//             stored copy).  For the output layer K = pad32(D_out): dY passes the tile's image in chunks of at most 512
//             columns and one chain runs on through the chunks (dot_packed_range).
//   RAdam     lnmlp_train_core.hpp's, the learning rate a per-step value.
#pragma once
#include "lnmlp_train_core.hpp"

namespace payne {
namespace specmlp {

using namespace payne::lnmlp;

constexpr int kActLeaky = 0;                     // PAYNE_SPECMLP_LEAKY
constexpr int kActSigmoid = 1;                   // PAYNE_SPECMLP_SIGMOID
constexpr float kLeakySlope = 0.01f;             // nn.LeakyReLU()'s default
constexpr int kOutChunk = kWaves * kTile;        // output columns a workgroup of the output-layer launch takes: 128
constexpr int kBackChunk = kMaxWidth;            // columns of dY in the tile's image at a time: 512
constexpr int kMaxOut = 65536;

// ---- activations ------------------------------------------------------------------------------------------------------
PAYNE_LNMLP_HD float act_forward(float z, int kind) {
  return kind == kActSigmoid ? 1.0f / (1.0f + expf(-z)) : (z > 0.0f ? z : kLeakySlope * z);
}
// the derivative from the block's output a
PAYNE_LNMLP_HD float act_slope(float a, int kind) {
  return kind == kActSigmoid ? a * (1.0f - a) : (a > 0.0f ? 1.0f : kLeakySlope);
}
// Thread `part` of a row: z becomes a (also written to a_out), columns part, part + 4, ... below n.
PAYNE_LNMLP_HD void row_act_forward(float* zr, int part, int n, int kind, float* a_out) {
  for (int j = part; j < n; j += kParts) {
    const float a = act_forward(zr[j], kind);
    zr[j] = a;
    a_out[j] = a;
  }
}
// Thread `part` of a row: d holds dA, becomes dZ = dA act'(a) (also written to dz_out).
PAYNE_LNMLP_HD void row_act_backward(float* d, const float* a, int part, int n, int kind, float* dz_out) {
  for (int j = part; j < n; j += kParts) {
    const float dz = d[j] * act_slope(a[j], kind);
    d[j] = dz;
    dz_out[j] = dz;
  }
}

// ---- loss -------------------------------------------------------------------------------------------------------------
constexpr float kLossGradScale = 2.0f;           // d/dy of MSELoss(reduction='sum')
// One element: r = y - t in fp32; *sq += r^2 in fp64; returns dY.
PAYNE_LNMLP_HD float elem_loss_grad(float y, float t, float scale, double* sq) {
  const float r = y - t;
  *sq += (double)r * (double)r;
  return r * scale;
}

// ---- a chain over part of K ---------------------------------------------------------------------------------------------
// dot_packed over the k-blocks kb0 .. kb1 - 1 of KB, continuing the chain `acc`; a[0] is the input 8 kb0 (the chunk as it
// lies in the tile's image).
PAYNE_LNMLP_HD float dot_packed_range(const float* a, const float* w, int col, int kb0, int kb1, int KB, float acc) {
  const int ct = col / kTile, c = col % kTile;
  for (int kb = kb0; kb < kb1; ++kb)
    for (int s = 0; s < 4; ++s) {
      acc = fmaf(a[(kb - kb0) * kKBlock + s], w[packed_index(ct, kb, c, s, KB)], acc);
      acc = fmaf(a[(kb - kb0) * kKBlock + 4 + s], w[packed_index(ct, kb, c + 32, s, KB)], acc);
    }
  return acc;
}

// ---- one layer of the step as the kernels see it (device pointers; host pointers in the emulator) -------------------------
// vec, gvec, mvec, vvec: [pad32(n_out)], the bias; a_in: the layer's input [rows][pad32(n_in)] (a hidden block's output is
// the next layer's a_in); dz: [rows][pad32(n_out)] (the output layer's is dY); slab: [tiles][pad32(n_out)], a tile's sums over
// its rows of dz.  rows = tiles * 64.
struct SpecLayer {
  float *wm, *wp, *wt, *vec;
  float *gw, *gvec;
  float *mw, *vw, *mvec, *vvec;
  float *a_in, *dz, *slab;
  int n_in, n_out;
};
struct SpecNet {
  static constexpr int kHiddenVecs = 1;                             // per-column vectors of a hidden layer; the slabs' stride
  int n_layers;
  int act;
  SpecLayer L[kMaxLayers];
  double* loss_slab;                                                // [tiles][out_chunks]
};
PAYNE_LNMLP_HD int out_chunks(int d_out) { return (d_out + kOutChunk - 1) / kOutChunk; }
PAYNE_LNMLP_HD int max_of(int a, int b) { return a > b ? a : b; }
// floats per row of the hidden launches' image: the widest padded row they read or write, plus kRowPad
PAYNE_LNMLP_HD int hidden_stride(const SpecNet& net, bool backward) {
  int m = k_blocks(net.L[0].n_in) * kKBlock;
  for (int l = 0; l + 1 < net.n_layers; ++l) m = max_of(m, pad32(net.L[l].n_out));
  if (backward) {
    const int p = pad32(net.L[net.n_layers - 1].n_out);
    m = max_of(m, p < kBackChunk ? p : kBackChunk);
  }
  return pad32(m) + kRowPad;
}
// the output-layer launch's image: A_last [64][pad32(H) + 4], reused for the dY of the workgroup's 128 columns
PAYNE_LNMLP_HD int out_stride(const SpecNet& net) { return max_of(pad32(net.L[net.n_layers - 1].n_in), kOutChunk) + kRowPad; }

}  // namespace specmlp
}  // namespace payne
