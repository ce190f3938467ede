// sed_core.hpp -- photometry: FastPayneSEDPredict.sed (Payne/predict/predictsed.py:75-103, photANN.py:95-131,
// highred.py:4-25) as device functions shared by the two forms that ship:
//   * payne_sed_kernel (sed_kernel.hpp): one wave per (candidate, filter) -- the stand-alone entry points
//     (payne_sed_batch, payne_bc_batch) and likelihoods without a hidden-layer launch;
//   * sed_tile (below): one 256-thread workgroup per (filter, block of 64 candidates), run by workgroups appended to the
//     hidden-layer launch on compute units its 160 GEMM tiles leave idle -- the joint likelihood's photometry then costs
//     no launch of its own (C3: 9.1 us as a launch between the dense kernels and the post kernel).
// The head of this file is plain C++, host / device: the tile's sizes and the arithmetic of a row (label encoding, high-Av offset,
// magnitude terms), written once for these kernels, for the SED fit (sedfit_core.hpp, k_sedfit.hip) and for the host programs of
// tests/ (test_phot_shapes.py's planner, tests/emul/sedfit_emul.cpp).  The fp64 matrix tile itself is sed_tile.hpp.
// Arithmetic: fp64 on fp32 weights, as numpy promotes them (photANN.py:125-131).
#pragma once
#include <math.h>
#include <stddef.h>

#ifdef __HIPCC__
#define PAYNE_SED_HD __host__ __device__ inline
#else
#define PAYNE_SED_HD inline
#endif

// ---- tile form: sizes, and how many candidates a tile takes (plain C++: tests/test_phot_shapes.py builds this part with g++)
constexpr int kSedCandsMax = 48;
constexpr int kSedMaxH = 64;
constexpr int kSedPitchA = kSedMaxH + 2;      // doubles: row stride 132 dwords = 4 banks (mod 64): the 16 rows of an A fragment hit 16 bank quads
constexpr int kSedPitchW = kSedMaxH + 16;     // floats: k rows 80 dwords apart = 16 banks (mod 32): the k = 0..3 rows of a B fragment do not collide
PAYNE_SED_HD bool sed_tile_ok(int H) { return H >= 16 && H <= kSedMaxH && (H & 15) == 0; }
PAYNE_SED_HD int sed_padded_width(int H) { return (H + 15) & ~15; }   // the next width the tile takes (the SED fit pads with zero weights)
// Candidates per photometric tile for a batch of B and F filters: as few as keeps F x blocks within `slots`, the workgroup slots the
// hidden-layer launch's other workgroups leave free (none or fewer: one block over the whole batch) -- a multiple of 16 in
// 16 .. kSedCandsMax; the launch then has F * ceil(B / cb) tiles.
PAYNE_SED_HD int sed_tile_cands(int B, int F, int slots) {
  const int nblk = slots >= F ? slots / F : 1;
  const int cb = ((B + nblk - 1) / nblk + 15) & ~15;
  return cb < 16 ? 16 : (cb > kSedCandsMax ? kSedCandsMax : cb);
}
// w2 [F][h][k] as fastANN stacks it -> [F][k][h] in rows of Hp >= H values (lanes, h, read consecutive addresses); dst holds F Hp Hp
// values, and what lies beyond H stays as it was.
inline void sed_transpose_w2(int F, int H, int Hp, const float* src, float* dst) {
  for (int f = 0; f < F; ++f)
    for (int h = 0; h < H; ++h)
      for (int k = 0; k < H; ++k) dst[((size_t)f * Hp + k) * Hp + h] = src[((size_t)f * H + h) * H + k];
}

// ---- a row's arithmetic (plain C++) ------------------------------------------------------------------------------------------
constexpr double kSedRv = 3.1;                // the Rv of a theta row (never honoured: likelihood.py:104-106), and of the nets at Av >= 5
// av >= 5 (or NaN): the nets are evaluated at av = 0, rv = 3.1 and the high-Av table corrects (predictsed.py:86-90)
PAYNE_SED_HD bool sed_hi_av(double av) { return !(av < 5.0); }
// The six encoded labels (x - xmin) / (xmax - xmin), photANN.py:118-120 (no -0.5); lab = Teff, logg, feh, afe.
PAYNE_SED_HD void sed_encode(const double* lab, double av, double rv, bool hi, const double* xmin, const double* xden, double* xs) {
  const double x[6] = {lab[0], lab[1], lab[2], lab[3], hi ? 0.0 : av, hi ? kSedRv : rv};
  for (int d = 0; d < 6; ++d) xs[d] = (x[d] - xmin[d]) / xden[d];
}
// highred.py:19-25 for the filter whose row of the table is c [5] (NULL: the filter has none, NaN): BC(av, rv) = BC(0, 3.1) - offset,
// offset = c0 + c1 av slope, slope = c2 + c3 rv + c4 rv^2.
PAYNE_SED_HD double sed_hiav_slope(const double* c, double rv) { return c[2] + c[3] * rv + c[4] * (rv * rv); }
PAYNE_SED_HD double sed_hiav_offset(const double* c, double av, double rv) {
  return c ? (c[0] + c[1] * av * sed_hiav_slope(c, rv)) : __builtin_nan("");
}
// The magnitude formulae are (a1 - BC) + a2 with a1, a2 functions of the row alone (predictsed.py:92-103): from luminosity and
// distance, or from log(A); a theta row's luminosity (genmod.py:126).  The association is the expressions'.
PAYNE_SED_HD void sed_terms_dist(double logl, double dist, double& a1, double& a2) { a1 = -2.5 * logl + 4.74; a2 = 5.0 * log10(dist) - 5.0; }
PAYNE_SED_HD void sed_terms_scaled(double logA, double logt, double& a1, double& a2) { a1 = 5.0 * logA - 10.0 * (logt - log10(5770.0)) - 0.26; a2 = 0.0; }
PAYNE_SED_HD double sed_theta_logl(double logr, double logt) { return 2.0 * logr + 4.0 * (logt - log10(5770.0)); }

#ifdef __HIPCC__
#include <type_traits>

#include "sed_tile.hpp"

struct PhotTables {
  int F, H;
  const float *w1, *b1, *w2t, *b2, *w3, *b3;   // w2t: [F][k][h] (transposed for coalesced lanes)
  double xmin[6], xden[6];
  const double* hiav;                           // device [F][5] or null
};

// What one (candidate) row asks of every filter: the six encoded labels and the magnitude formula's scalars.
struct SedRow {
  double xs[6];                 // sed_encode
  double logt, av, rv, logl, dist, logA;
  bool hi;                      // sed_hi_av
};
// mode 0: in = [logt,logg,feh,afe,av,rv,logl,dist,logA] (sed kwargs, NaN = absent)
// mode 1: in = theta row; phot block at column `off` = [logA | logR, Dist, Av, Rv]
// mode 2: in = [Teff,logg,feh,afe,av,rv]; output = the bolometric corrections themselves
//         (fastANN.eval, photANN.py:125-131: no high-Av branch, no magnitude formula)
__device__ __forceinline__ SedRow sed_row(const PhotTables& P, const double* r, int mode, int off, int photscale) {
  const double nan = __builtin_nan("");
  SedRow s;
  s.logl = nan; s.dist = nan; s.logA = nan;
  if (mode == 0) {
    s.logt = r[0]; s.av = r[4]; s.rv = r[5]; s.logl = r[6]; s.dist = r[7]; s.logA = r[8];
  } else if (mode == 2) {
    s.logt = nan; s.av = r[4]; s.rv = r[5];
  } else {
    s.logt = log10(r[0]);                                         // genmod.py:124,172
    s.av = r[off + 2]; s.rv = kSedRv;
    if (photscale) s.logA = r[off];                               // genphot_scaled, genmod.py:157-187
    else { s.logl = sed_theta_logl(r[off], s.logt); s.dist = r[off + 1]; }   // genphot
  }
  // predictsed.py:84 evaluates 10**logt; for a theta row logt IS log10(Teff) (genmod.py:124,172), and Teff differs from
  // 10**log10(Teff) by an ulp or two (1e-15 of the encoded label): the row's own value is used, not a pow() per candidate
  const double lab[4] = {mode == 0 ? pow(10.0, s.logt) : r[0], r[1], r[2], r[3]};
  s.hi = (mode != 2) && sed_hi_av(s.av);
  sed_encode(lab, s.av, s.rv, s.hi, P.xmin, P.xden, s.xs);
  return s;
}
// bolometric correction of filter f -> magnitude (predictsed.py:92-103, highred.py:19-25): which formula a row's scalars select.
__device__ __forceinline__ void sed_mag_terms(const SedRow& s, double& a1, double& a2) {
  const double nan = __builtin_nan("");
  if (!(s.logl != s.logl) && !(s.dist != s.dist)) sed_terms_dist(s.logl, s.dist, a1, a2);
  else if (!(s.logA != s.logA)) sed_terms_scaled(s.logA, s.logt, a1, a2);
  else { a1 = nan; a2 = nan; }
}
__device__ __forceinline__ double sed_bc_hi(const PhotTables& P, bool hi, double av, double rv, int f, double BC) {
  if (hi) BC = BC - sed_hiav_offset(P.hiav ? P.hiav + 5 * f : nullptr, av, rv);
  return BC;
}
__device__ __forceinline__ double sed_mag(const PhotTables& P, const SedRow& s, int f, int mode, double BC) {
  BC = sed_bc_hi(P, s.hi, s.av, s.rv, f, BC);
  if (mode == 2) return BC;
  double a1, a2;
  sed_mag_terms(s, a1, a2);
  return (a1 - BC) + a2;
}

// ---- tile form -------------------------------------------------------------------------------------------
// One workgroup of 256 threads: filter f, candidates c0 .. c0 + cb - 1 of a theta batch (mode 1), cb <= 48, on sed_tile.hpp's tile:
// candidates are the rows (up to three 16-row tiles), fp32 weights promoted on the way into the operand as numpy promotes them.
// Every global value the tile needs is requested in one batch at its start; a single wave issues an instruction every ~5 cycles
// whatever it is, so sixteen fp64 fma per lane cost what ONE matrix instruction costs.
//   LDS: SedTileLds (X: encoded labels, then layer-1 outputs, then layer-2 outputs) | Mt [48][2] f64, the rows' magnitude terms
constexpr size_t sed_tile_lds_bytes() { return SedTileLds::bytes + (size_t)2 * kSedCandsMax * 8; }

__device__ inline void sed_tile(const PhotTables& P, const double* __restrict__ theta, int ld, int off, int photscale, int B,
                                int f, int c0, int cb, double* __restrict__ mags, unsigned char* smem,
                                unsigned long long* st = nullptr /* diagnostic build: cycle stamps of this tile */) {
#define SED_STAMP(k) do { if (st && threadIdx.x == 0) st[k] = __builtin_amdgcn_s_memtime(); } while (0)
  SED_STAMP(0);
  const int H = P.H, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SedTileView t = sed_tile_view(smem);
  double* X = t.X;
  float* W1 = t.W1;
  double* Mt = reinterpret_cast<double*>(smem + SedTileLds::bytes);         // [48][2] magnitude terms
  // ---- requests: the W2 tile and the three vectors, W1, this thread's theta row
  const SedWeights wr = sed_weights_request(P.w2t + (size_t)f * H * H, H, P.b1 + f * H, P.b2 + f * H, P.w3 + f * H);
  float w1reg[2];                                                           // W1 is [h][6] in memory: 6 H <= 384 values
#pragma unroll
  for (int q = 0; q < 2; ++q) { const int i = tid + 256 * q; w1reg[q] = P.w1[(size_t)f * H * 6 + (i < 6 * H ? i : 0)]; }
  const float b3 = P.b3[f];
  // rows: wave 0 encodes the labels (what the first layer waits for), wave 1 works out the magnitude formula's terms
  // (two fp64 logarithms) for the same rows meanwhile; both read the row themselves
  const int rt = tid & 63;
  const int c = c0 + rt;
  const bool rowt = rt < kSedCandsMax && wave < 2, live = rt < cb && c < B;
  const double* rowp = theta + (size_t)(live ? c : (c0 < B ? c0 : B - 1)) * ld;
  // (wave 1's terms -- a log10 or two a row -- are worked out HERE, while the weight tile is still on its way: behind the
  //  operands' barrier they sat in front of the first layer's own barrier, 2 700 of that layer's 5 500 cycles)
  double xs[6], av = 0.0; bool hi = false;
  double mt1 = 0.0, mt2 = 0.0;
  if (rowt && wave == 0) {                                                  // (no logarithm: the labels need none, mode 1 takes Teff itself)
    av = rowp[off + 2];
    hi = sed_hi_av(av);
    sed_encode(rowp, av, kSedRv, hi, P.xmin, P.xden, xs);
  }
  if (rowt && wave == 1) {
    const SedRow s = sed_row(P, rowp, 1, off, photscale);
    sed_mag_terms(s, mt1, mt2);
  }
  SED_STAMP(1);
  // ---- commit to LDS
  if (rowt && wave == 0) {
#pragma unroll
    for (int d = 0; d < 6; ++d) X[rt * kSedPitchA + d] = xs[d];
    X[rt * kSedPitchA + 6] = 0.0; X[rt * kSedPitchA + 7] = 0.0;             // k padding of the first layer (K = 6 -> 8)
  }
  sed_weights_commit(wr, H, t);
#pragma unroll
  for (int q = 0; q < 2; ++q) { const int i = tid + 256 * q; if (i < 6 * H) { const int h = i / 6, d = i - 6 * h; W1[d * kSedPitchW + h] = w1reg[q]; } }
  if (tid < 2 * kSedMaxH) W1[(6 + tid / kSedMaxH) * kSedPitchW + (tid % kSedMaxH)] = 0.f;
  if (rowt && wave == 1) { Mt[2 * rt] = mt1; Mt[2 * rt + 1] = mt2; }
  __syncthreads();
  SED_STAMP(3);
  const int mt_n = (cb + 15) >> 4, nt_n = H >> 4;                           // row tiles (<= 3), column tiles (<= 4)
  const int li = lane & 15, lk = lane >> 4;
  // one layer: X[.][0..K) -> sigmoid(X W + b) back into X[.][0..H); every wave reads all of X before anyone writes.
  // H <= 64: at most four 16-column tiles, wave w owns tile w (or none).
  const bool on = wave < nt_n;
  const int nt = on ? wave : 0;
  // (MT = the tile's row tiles, a compile-time copy per count: a 16-candidate tile reads a third of the fragments and runs four
  //  sigmoid chains a lane instead of twelve -- as one body sized for 48 candidates every tile paid for three)
  auto layer = [&](auto mtc, const float* Wl, int K, const float* bias) {
    constexpr int MT = decltype(mtc)::value;
    sed_d4 acc[MT];
    const double bz = (double)bias[16 * nt + li];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (sed_d4){bz, bz, bz, bz};
    if (on) sed_mfma<MT, kSedMaxH / 4>(X, kSedPitchA, Wl, K >> 2, nt, li, lk, acc);
    __syncthreads();
    if (on) {
      double y[4 * MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) y[4 * mt + v] = acc[mt][v];
      sed_sigmoid_n<4 * MT>(y);                                             // 4 MT chains side by side
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int v = 0; v < 4; ++v) X[(16 * mt + lk + 4 * v) * kSedPitchA + 16 * nt + li] = y[4 * mt + v];
      }
    }
    __syncthreads();
  };
  auto layers = [&](auto mtc) {
    layer(mtc, W1, 8, t.Bv);                                                // photANN.py:127
    SED_STAMP(4);
    layer(mtc, t.W2, H, t.Bv + kSedMaxH);                                   // :128
  };
  if (mt_n == 1) layers(std::integral_constant<int, 1>{});
  else if (mt_n == 2) layers(std::integral_constant<int, 2>{});
  else layers(std::integral_constant<int, 3>{});
  SED_STAMP(6);
  // ---- layer 3 (:129-131): the waves' partial sums of row `rt`, wave 0 adds the four
  sed_layer3_partials(t, rt, wave, on);
  __syncthreads();
  if (wave == 0 && live) {
    const double bc = sed_bc_hi(P, hi, av, kSedRv, f, sed_row_sum_onto(t.Pt, rt, (double)b3));
    mags[(size_t)c * P.F + f] = (Mt[2 * rt] - bc) + Mt[2 * rt + 1];
  }
  SED_STAMP(5);
#undef SED_STAMP
}
#endif  // __HIPCC__
