// specjac_core.hpp -- arithmetic of payne_specjac_eval and payne_fisher_batch (k_specjac.hip): the spectral networks of
// Payne/predict/ystpred.py:18-58 (Net) and Payne/train/NNmodels.py (SMLP, LinNet) together with their Jacobian with respect to
// the labels, by a forward-mode pass through the dense layers.  Written host/device like specmlp_train_core.hpp, whose constants,
// weight packing and dot_packed chain it reuses: the same source runs in the kernels and on the host
// (tests/emul/specjac_emul.cpp, also under ASan / UBSan).
//   input    e_k = (x_k - xmin_k) / (xmax_k - xmin_k) - 0.5 in fp64, rounded once to fp32 (ystpred.py:47-50, NNmodels.py:109-113).
//   primal   z_0 = W_0 e + b_0, a_l = act(z_l), z_{l+1} = W_{l+1} a_l + b_{l+1}; y = z_last.  fp32, one output a dot_packed chain
//            + one addition of the bias.
//   tangent  for label k: tz_0 = W_0[:, k], ta_l = act'(z_l) * tz_l, tz_{l+1} = W_{l+1} ta_l (no bias); dy/de_k = tz_last and
//            dy/dx_k = dy/de_k * (float)(1 / (xmax_k - xmin_k)), the factor formed in fp64.  The kernel obtains tz_0 as the same
//            dot_packed chain on the unit vector of label k, which returns W_0[n][k] itself: 1 * w + 0 is exact, and so is every
//            0 * w' + w that follows for finite weights.
//   act'     LeakyReLU(0.01): 1 where z > 0, else 0.01 -- torch's rule, z == 0 included.  The reference's numpy leaky_relu
//            (ystpred.py:41-45) is 0 at z == 0 and so has slope 0 there; that is a set of measure zero.  Sigmoid: s (1 - s) from
//            the primal's fp32 s.
//   tile     a workgroup's 64-row image holds S = 64 / (1 + D_in) stars: row m * S + s is star s's primal (m = 0) or its tangent of
//            label m - 1.  Rows from (1 + D_in) * S on are zero.
//   Fisher   F[i][j] = sum_p (rows[i][p] * rows[j][p]) * w[p] in fp64, p in index order, pixels with w[p] == 0 skipped by a branch
//            (the rows may hold NaN there); computed for i <= j and mirrored.
#pragma once
#include "specmlp_train_core.hpp"

namespace payne {
namespace specjac {

using namespace payne::specmlp;

constexpr int kMaxLabels = 8;                    // D_in of a network payne_specjac_create accepts
constexpr int kMaxFisherRows = 16;               // K of payne_fisher_batch
constexpr int kFisherChunk = 256;                // pixels of the K rows in the workgroup's image at a time
constexpr unsigned kFlagEncoded = 1u;            // PAYNE_JAC_ENCODED

PAYNE_LNMLP_HD int stars_per_tile(int d_in) { return kTileRows / (1 + d_in); }
PAYNE_LNMLP_HD int tiles_of(int n_stars, int d_in) { return (n_stars + stars_per_tile(d_in) - 1) / stars_per_tile(d_in); }

PAYNE_LNMLP_HD float encode(double x, double xmin, double xmax) { return (float)((x - xmin) / (xmax - xmin) - 0.5); }
PAYNE_LNMLP_HD float label_scale(double xmin, double xmax) { return (float)(1.0 / (xmax - xmin)); }

// Row m * S + s of a tile's input image, column k (k below 8): the star's encoded labels, or the unit vector of label m - 1.
PAYNE_LNMLP_HD float input_value(int m, int k, int d_in, const double* x, const double* xmin, const double* xmax) {
  if (k >= d_in) return 0.0f;
  if (m == 0) return encode(x[k], xmin[k], xmax[k]);
  return k == m - 1 ? 1.0f : 0.0f;
}

// One hidden unit of one star: z becomes a, the d_in tangents tz_k (t[k * step]) become ta_k.
PAYNE_LNMLP_HD void unit_forward(float* z, float* t, int step, int d_in, int kind) {
  const float zv = *z;
  float a, slope;
  if (kind == kActSigmoid) {
    a = 1.0f / (1.0f + expf(-zv));
    slope = a * (1.0f - a);
  } else {
    a = zv > 0.0f ? zv : kLeakySlope * zv;
    slope = zv > 0.0f ? 1.0f : kLeakySlope;
  }
  *z = a;
  for (int k = 0; k < d_in; ++k) t[(size_t)k * (size_t)step] *= slope;
}

// What the kernels are given: device pointers (host pointers in the emulator).  w in lnmlp_core.hpp's stored order, b padded with
// zeros to pad32(n_out).  a_last: the tiles' images behind the last activation, [tiles * 64][pad32(n_in of the output layer)].
struct JacLayer {
  const float* w;
  const float* b;
  int n_in, n_out;
};
struct JacNet {
  int n_layers;
  int act;
  JacLayer L[kMaxLayers];
  double xmin[kMaxLabels], xmax[kMaxLabels];
  float scale[kMaxLabels];                                          // label_scale, or 1 under PAYNE_JAC_ENCODED
  float* a_last;
};

// floats per row of the hidden launch's image
PAYNE_LNMLP_HD int jac_hidden_stride(const JacNet& net) {
  int m = kKBlock;
  for (int l = 0; l + 1 < net.n_layers; ++l) m = max_of(m, pad32(net.L[l].n_out));
  return pad32(m) + kRowPad;
}
PAYNE_LNMLP_HD int jac_out_stride(const JacNet& net) { return pad32(net.L[net.n_layers - 1].n_in) + kRowPad; }

// Where the output layer's value `acc` of tile row r (star r % S of the tile, block m = r / S) and column col goes: y for m == 0
// (+ the bias), the tangent times its label's scale otherwise.  Rows that hold no star write nothing.
PAYNE_LNMLP_HD void store_output(float acc, int r, int d_in, long long star0, int N, int col, float bias, const float* scale, float* y,
                                 long long ld_y, float* jac, long long ld_j) {
  const int S = stars_per_tile(d_in), m = r / S;
  const long long star = star0 + (r - m * S);
  if (m > d_in || star >= (long long)N) return;
  if (m == 0) {
    if (y) y[(size_t)star * (size_t)ld_y + (size_t)col] = acc + bias;
  } else {
    jac[((size_t)star * (size_t)d_in + (size_t)(m - 1)) * (size_t)ld_j + (size_t)col] = acc * scale[m - 1];
  }
}

// ---- Fisher matrix ------------------------------------------------------------------------------------------------------
// One pixel's term of F[i][j]; the caller has found w != 0.
PAYNE_LNMLP_HD double fisher_term(float ai, float aj, double w, double acc) { return acc + ((double)ai * (double)aj) * w; }

}  // namespace specjac
}  // namespace payne
