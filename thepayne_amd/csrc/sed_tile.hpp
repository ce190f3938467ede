// sed_tile.hpp -- the fp64 matrix tile of the photometric nets (fastANN.eval, photANN.py:125-131: 6 -> H -> H -> 1, sigmoids, fp64
// on fp32 weights), written once for its two users: sed_tile (sed_core.hpp: the joint likelihood's magnitudes, riding in the
// hidden-layer launch) and sedfit_filter (k_sedfit.hip: the SED fit's magnitudes with tangent rows).  This file is the tile's home;
// its sizes (kSedCandsMax, kSedMaxH, the pitches) are at the head of sed_core.hpp, which includes it: include that.
//
// A workgroup of 256 threads (kSedThreads) holds one filter's net and up to 48 rows.  Both hidden layers run on v_mfma_f64_16x16x4_f64
// (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[i = (lane >> 4) + 4 v][j = lane & 15], v = 0..3): the rows
// of X are the rows (three 16-row tiles), the layer's outputs the columns; H <= 64 is at most four 16-column tiles, and wave w
// owns tile w (or none).  What is here: the LDS map, the request / commit pair of a filter's weights, the matrix products
// (sed_mfma), the sigmoid, layer 3's partial sums and the two ways of adding them.  What the users keep is what differs: where W1
// comes from, which rows carry a bias, and the pass between the products and the next layer.
#pragma once

typedef double sed_d4 __attribute__((ext_vector_type(4)));
typedef float sed_f4 __attribute__((ext_vector_type(4)));

// ---- LDS ---------------------------------------------------------------------------------------------------------------------------
// Byte offsets from the tile's base (16-byte aligned; every size is a multiple of 16).  A user places its own arrays behind `bytes`.
struct SedTileLds {
  static constexpr size_t X = 0;                                             // f64 [48][kSedPitchA]: a layer's input, then its output
  static constexpr size_t W2 = X + (size_t)kSedCandsMax * kSedPitchA * 8;    // f32 [H][kSedPitchW]: [k][h]
  static constexpr size_t W1 = W2 + (size_t)kSedMaxH * kSedPitchW * 4;       // f32 [8][kSedPitchW]: [d][h], rows 6, 7 zero (the user fills it)
  static constexpr size_t Bv = W1 + (size_t)8 * kSedPitchW * 4;              // f32 b1 | b2 | w3, kSedMaxH each
  static constexpr size_t Pt = Bv + (size_t)3 * kSedMaxH * 4;                // f64 [4][48]: the waves' partial sums of layer 3
  static constexpr size_t bytes = Pt + (size_t)4 * kSedCandsMax * 8;
};
struct SedTileView {
  double* X;
  float *W2, *W1, *Bv;
  double* Pt;
};
__device__ __forceinline__ SedTileView sed_tile_view(unsigned char* base) {
  return SedTileView{reinterpret_cast<double*>(base + SedTileLds::X), reinterpret_cast<float*>(base + SedTileLds::W2),
                     reinterpret_cast<float*>(base + SedTileLds::W1), reinterpret_cast<float*>(base + SedTileLds::Bv),
                     reinterpret_cast<double*>(base + SedTileLds::Pt)};
}

// ---- a filter's weights: request, then commit ----------------------------------------------------------------------------------------
// The W2 tile as H H / 4 16-byte pieces (four a thread at most; the threads beyond them ask for the last piece again) and b1 | b2 | w3
// through the first 192 threads.  w2t: the filter's [k][h], H x H; b1, b2, w3: the filter's [H].  The registers come back, so the
// caller decides what runs while the weights are on their way; sed_weights_commit stores them to W2 and Bv.
constexpr int kSedThreads = 256;
constexpr int kSedW2Pieces = kSedMaxH * kSedMaxH / 4 / kSedThreads;
struct SedWeights {
  sed_f4 w2[kSedW2Pieces];
  float v;
};
__device__ __forceinline__ SedWeights sed_weights_request(const float* w2t, int H, const float* b1, const float* b2, const float* w3) {
  const int tid = threadIdx.x, n4 = (H * H) >> 2;
  const sed_f4* w2g = reinterpret_cast<const sed_f4*>(w2t);
  SedWeights r;
#pragma unroll
  for (int q = 0; q < kSedW2Pieces; ++q) { const int i = tid + kSedThreads * q; r.w2[q] = w2g[i < n4 ? i : n4 - 1]; }
  r.v = 0.f;
  if (tid < 3 * kSedMaxH) {
    const int which = tid / kSedMaxH, h = tid - which * kSedMaxH;
    const float* src = which == 0 ? b1 : (which == 1 ? b2 : w3);
    r.v = src[h < H ? h : 0];
  }
  return r;
}
__device__ __forceinline__ void sed_weights_commit(const SedWeights& r, int H, const SedTileView& t) {
  const int tid = threadIdx.x, n4 = (H * H) >> 2, hq4 = H >> 2;
#pragma unroll
  for (int q = 0; q < kSedW2Pieces; ++q) {
    const int i = tid + kSedThreads * q;
    if (i < n4) { const int k = i / hq4, h4 = i - k * hq4; *reinterpret_cast<sed_f4*>(t.W2 + k * kSedPitchW + 4 * h4) = r.w2[q]; }
  }
  if (tid < 3 * kSedMaxH) t.Bv[tid] = r.v;
}

// ---- the matrix products ----------------------------------------------------------------------------------------------------------
// acc[mt] += A[16 mt .. 16 mt + 15][0 .. 4 ks_n) W[0 .. 4 ks_n)[16 nt .. 16 nt + 15], mt < MT, ks_n <= KS: A is f64 with row pitch
// pitchA, W f32 [k][kSedPitchW].  Every operand fragment is requested from LDS before the first matrix instruction (KS steps: KS
// (1 + MT) values a lane; a step beyond ks_n asks for step 0 again and is not multiplied).  The caller has initialised acc (the
// bias, or zero) and writes the epilogue; D[16 mt + lk + 4 v][16 nt + li] = acc[mt][v].
template <int MT, int KS>
__device__ __forceinline__ void sed_mfma(const double* A, int pitchA, const float* W, int ks_n, int nt, int li, int lk, sed_d4* acc) {
  float bfr[KS];
  double afr[MT][KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int k0 = 4 * (ks < ks_n ? ks : 0);
    bfr[ks] = W[(k0 + lk) * kSedPitchW + 16 * nt + li];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) afr[mt][ks] = A[(16 * mt + li) * pitchA + k0 + lk];
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (ks < ks_n) {
      const double bfrag = (double)bfr[ks];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[mt][ks], bfrag, acc[mt], 0, 0, 0);
    }
  }
}

// ---- the sigmoid -------------------------------------------------------------------------------------------------------------------
// 1 / (1 + exp(-z)) in fp64 (photANN.py:125-131 through numpy) for N values at once: exp by 2^n * 2^f (|f| <= 1/2, degree-13
// Taylor polynomial of exp(f ln 2): truncation < 5e-18, n ln 2 subtracted from -z in two parts), the quotient by v_rcp_f64 +
// two Newton steps; relative error ~3e-16.  NaN stays NaN, z -> -inf gives 0, +inf gives 1.  Written step by step ACROSS
// the N values: one value's chain is ~35 dependent fp64 instructions (and libm's exp + an IEEE division ~3x that); a wave
// alone on its SIMD runs such a chain at its latency, N chains side by side at its issue rate (measured in sed_tile:
// twelve sigmoids one after the other 5 000 cycles).
template <int N>
__device__ __forceinline__ void sed_sigmoid_n(double* z) {
  double n[N], g[N], p[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double t = z[i] * -1.4426950408889634;                        // -z log2(e)
    const double tc = (t > 1000.0) ? 1000.0 : ((t < -1000.0) ? -1000.0 : t);   // (comparisons are false for NaN: it passes)
    n[i] = __builtin_rint(tc);
    const double zz = (tc == t) ? z[i] : tc * -0.6931471805599453;  // z as clamped (t only picks n: its rounding must not reach g)
    g[i] = fma(n[i], -0.6931471803691238, -zz);                   // -z - n ln2, ln2 in two parts (Cody-Waite): |g| <= 0.3466 + 1e-13
  }
#pragma unroll
  for (int i = 0; i < N; ++i) g[i] = fma(n[i], -1.9082149292705877e-10, g[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = fma(1.6059043836821613e-10, g[i], 2.08767569878681e-09);   // 1/13!, 1/12!
  constexpr double C[11] = {2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
                            0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664,
                            0.16666666666666666, 0.5, 1.0};       // 1/11! .. 1/1!
#pragma unroll
  for (int k = 0; k < 11; ++k)
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = fma(p[i], g[i], C[k]);
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = fma(p[i], g[i], 1.0);
  double d[N], r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = 1.0 + __builtin_ldexp(p[i], (int)n[i]);   // 1 + exp(-z), exp in [2^-1000, 2^1000] (NaN stays NaN)
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = __builtin_amdgcn_rcp(d[i]);
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = fma(fma(-d[i], r[i], 1.0), r[i], r[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) z[i] = r[i];
}
__device__ __forceinline__ double sed_sigmoid(double z) { sed_sigmoid_n<1>(&z); return z; }

// ---- layer 3 (photANN.py:129-131) -----------------------------------------------------------------------------------------------------
// Wave w sums the units h = 16 w .. 16 w + 15 of row `row` (the wave's lane) into Pt[w][row]: sixteen fma in ascending h, zero from a
// wave that owns no column tile.  A barrier follows before anyone adds the four.
__device__ __forceinline__ void sed_layer3_partials(const SedTileView& t, int row, int wave, bool on) {
  if (row < kSedCandsMax) {
    double part = 0.0;
    if (on) {
#pragma unroll
      for (int q = 0; q < 16; ++q) part = fma((double)t.Bv[2 * kSedMaxH + 16 * wave + q], t.X[row * kSedPitchA + 16 * wave + q], part);
    }
    t.Pt[wave * kSedCandsMax + row] = part;
  }
}
// The four partial sums of a row, in wave order.  The two users add them in different orders, and their frozen bits hold each to its own:
//   sed_row_sum_onto  (((b + P0) + P1) + P2) + P3: sed_tile starts from the bias b3;
//   sed_row_sum       ((P0 + P1) + P2) + P3: the SED fit's tangent rows have no bias, so every row is summed alike and the value
//                     row's b3 is added to the sum.
__device__ __forceinline__ double sed_row_sum_onto(const double* Pt, int r, double b) {
  for (int w = 0; w < 4; ++w) b += Pt[w * kSedCandsMax + r];
  return b;
}
__device__ __forceinline__ double sed_row_sum(const double* Pt, int r) {
  return ((Pt[r] + Pt[kSedCandsMax + r]) + Pt[2 * kSedCandsMax + r]) + Pt[3 * kSedCandsMax + r];
}
