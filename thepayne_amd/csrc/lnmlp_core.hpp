// lnmlp_core.hpp -- arithmetic of payne_lnmlp_eval (k_lnmlp.hip): the photometric networks of Payne/predict/photANN_new.py,
// Linear -> LayerNorm -> SiLU blocks and a closing Linear (MLP_v0 / MLP_v1 of Payne/train/NNmodels_new.py).  Written
// host/device so that the same source runs
//   * on gfx950 inside payne_lnmlp_kernel, and
//   * on the host (tests/emul/lnmlp_emul.cpp: one row at a time through row_forward) as the CPU-side check, also under
//     ASan / UBSan.
// Everything between the input and the output conversion is fp32.  One output of a Linear layer is an fp32 fmaf chain that
// starts at zero and takes the layer's inputs in the order of the matrix instruction's k-steps (dot_packed; the weights are
// stored in that order, pack_weights), then one addition of the bias.  LayerNorm follows nn.LayerNorm: the mean over the
// row's true width, the biased variance about that mean, eps = 1e-5; both sums are taken by kParts threads, each over every
// kParts-th element in kParts accumulators, and added up as a tree -- a fixed order, nothing that depends on timing.
#pragma once
#include <math.h>
#include <stddef.h>

#ifdef __HIPCC__
#define PAYNE_LNMLP_HD __host__ __device__ __forceinline__
#else
#define PAYNE_LNMLP_HD inline
#endif

namespace payne {
namespace lnmlp {

constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;         // one workgroup
constexpr int kTileRows = 64;                    // rows of x a workgroup evaluates: two 32-row matrix tiles
constexpr int kTile = 32;                        // the matrix instruction's tile (32 x 32 x 2)
constexpr int kKBlock = 8;                       // inputs per stored weight fragment: four k-steps of two
constexpr int kParts = kThreads / kTileRows;     // threads that share a row's LayerNorm sums
constexpr int kRowPad = 4;                       // floats between two rows of the LDS image beyond the padded width
constexpr int kMaxLayers = 8;
constexpr int kMaxIn = 32;
constexpr int kMaxWidth = 512;
constexpr float kEps = 1e-5f;

static_assert(kParts == 4, "the LayerNorm sums are written for four threads a row");

PAYNE_LNMLP_HD int k_blocks(int n_in) { return (n_in + kKBlock - 1) / kKBlock; }
PAYNE_LNMLP_HD int col_tiles(int n_out) { return (n_out + kTile - 1) / kTile; }

// The stored order of a layer's weights: [column tile][k-block][lane][4].  Lane l of a wave holds, for column tile ct and
// k-block kb, the four weights W[ct*32 + (l & 31)][8 kb + 4 (l >> 5) + s], s = 0..3: one 16-byte load per lane, 1 KiB
// contiguous per wave, and element s is the lane's operand of the block's k-step s (which therefore sums the inputs
// 8 kb + s and 8 kb + 4 + s).  Rows beyond n_out and columns beyond n_in are zero.
PAYNE_LNMLP_HD size_t packed_index(int ct, int kb, int lane, int s, int KB) {
  return (((size_t)ct * (size_t)KB + (size_t)kb) * kWave + (size_t)lane) * 4 + (size_t)s;
}
PAYNE_LNMLP_HD size_t packed_floats(int n_in, int n_out) { return (size_t)col_tiles(n_out) * k_blocks(n_in) * kWave * 4; }

inline void pack_weights(const float* w, int n_in, int n_out, float* out) {
  const int KB = k_blocks(n_in), CT = col_tiles(n_out);
  for (int ct = 0; ct < CT; ++ct)
    for (int kb = 0; kb < KB; ++kb)
      for (int lane = 0; lane < kWave; ++lane)
        for (int s = 0; s < 4; ++s) {
          const int n = ct * kTile + (lane & 31), k = kb * kKBlock + 4 * (lane >> 5) + s;
          out[packed_index(ct, kb, lane, s, KB)] = (n < n_out && k < n_in) ? w[(size_t)n * (size_t)n_in + (size_t)k] : 0.0f;
        }
}

// What the kernel is given: device pointers (host pointers in the emulator).  w in the stored order above; b, gain, beta
// padded with zeros to col_tiles(n_out) * 32 entries; gain == beta == NULL on the output layer.
struct LayerArgs {
  const float* w;
  const float* b;
  const float* gain;
  const float* beta;
  int n_in, n_out;
};
struct NetArgs {
  int n_layers;
  LayerArgs L[kMaxLayers];
  const double* in_mid;
  const double* in_std;
  const double* out_mid;
  const double* out_std;
};

// floats per row of the activation image: the widest padded row any layer reads or writes, plus kRowPad (a stride of 4 mod 32 banks)
PAYNE_LNMLP_HD int act_stride(const NetArgs& net) {
  int m = k_blocks(net.L[0].n_in) * kKBlock;
  for (int l = 0; l < net.n_layers; ++l) {
    const int p = col_tiles(net.L[l].n_out) * kTile;
    m = p > m ? p : m;
  }
  return (m + kTile - 1) / kTile * kTile + kRowPad;
}

// photANN_new.ANN.eval: x_i = (x - mid) / std in fp64, then .type(FloatTensor): one rounding to fp32
PAYNE_LNMLP_HD float input_value(double x, const double* mid, const double* sd, int k) {
  return (float)(mid ? (x - mid[k]) / sd[k] : x);
}
// y[ii] = y[ii] * std + mid: the fp32 output times an fp64 scalar, in fp64, stored to the fp32 array
PAYNE_LNMLP_HD float output_value(float y, const double* mid, const double* sd, int j) {
  return mid ? (float)((double)y * sd[j] + mid[j]) : y;
}

// One output of a Linear layer before the bias: column `col` (of the padded width) from the row's inputs `a` (padded with
// zeros to KB * 8), in the order the matrix instruction sums them.
PAYNE_LNMLP_HD float dot_packed(const float* a, const float* w, int col, int KB) {
  const int ct = col / kTile, c = col % kTile;
  float acc = 0.0f;
  for (int kb = 0; kb < KB; ++kb)
    for (int s = 0; s < 4; ++s) {
      acc = fmaf(a[kb * kKBlock + s], w[packed_index(ct, kb, c, s, KB)], acc);
      acc = fmaf(a[kb * kKBlock + 4 + s], w[packed_index(ct, kb, c + 32, s, KB)], acc);
    }
  return acc;
}

// Thread `part` of a row's kParts: the sum of z[part], z[part + 4], ... below n
PAYNE_LNMLP_HD float partial_sum(const float* z, int part, int n) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int i = 0;
  for (int j = part; j < n; j += kParts, ++i) a[i & 3] += z[j];
  return (a[0] + a[1]) + (a[2] + a[3]);
}
PAYNE_LNMLP_HD float partial_sqdev(const float* z, int part, int n, float mean) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int i = 0;
  for (int j = part; j < n; j += kParts, ++i) {
    const float d = z[j] - mean;
    a[i & 3] = fmaf(d, d, a[i & 3]);
  }
  return (a[0] + a[1]) + (a[2] + a[3]);
}
// the four threads' sums: (p0 + p1) + (p2 + p3), what two exchanges between neighbouring lanes give every one of them
PAYNE_LNMLP_HD float combine_parts(float p0, float p1, float p2, float p3) { return (p0 + p1) + (p2 + p3); }
PAYNE_LNMLP_HD float mean_of(float total, int n) { return total / (float)n; }
PAYNE_LNMLP_HD float rstd_of(float sqdev_total, int n) { return 1.0f / sqrtf(sqdev_total / (float)n + kEps); }
PAYNE_LNMLP_HD float silu(float z) { return z / (1.0f + expf(-z)); }
PAYNE_LNMLP_HD float ln_silu(float z, float mean, float rstd, float gain, float beta) {
  return silu((z - mean) * rstd * gain + beta);
}

// The whole network for one row on the host, in the kernel's order.  x: the row's D_in fp64 inputs; y: D_out fp32 outputs;
// buf: 2 * act_stride(net) floats of scratch.
inline void row_forward(const NetArgs& net, const double* x, float* y, float* buf) {
  const int stride = act_stride(net);
  float* a = buf;
  float* z = buf + stride;
  const int K0 = k_blocks(net.L[0].n_in) * kKBlock;
  for (int k = 0; k < K0; ++k) a[k] = k < net.L[0].n_in ? input_value(x[k], net.in_mid, net.in_std, k) : 0.0f;
  for (int l = 0; l < net.n_layers; ++l) {
    const LayerArgs& L = net.L[l];
    const int KB = k_blocks(L.n_in), n_pad = col_tiles(L.n_out) * kTile;
    if (l + 1 == net.n_layers) {
      for (int j = 0; j < L.n_out; ++j) y[j] = output_value(dot_packed(a, L.w, j, KB) + L.b[j], net.out_mid, net.out_std, j);
      return;
    }
    for (int j = 0; j < n_pad; ++j) z[j] = dot_packed(a, L.w, j, KB) + L.b[j];
    float p[kParts], q[kParts];
    for (int t = 0; t < kParts; ++t) p[t] = partial_sum(z, t, L.n_out);
    const float mean = mean_of(combine_parts(p[0], p[1], p[2], p[3]), L.n_out);
    for (int t = 0; t < kParts; ++t) q[t] = partial_sqdev(z, t, L.n_out, mean);
    const float rstd = rstd_of(combine_parts(q[0], q[1], q[2], q[3]), L.n_out);
    for (int j = 0; j < L.n_out; ++j) z[j] = ln_silu(z[j], mean, rstd, L.gain[j], L.beta[j]);
    float* t = a; a = z; z = t;
  }
}

}  // namespace lnmlp
}  // namespace payne
