// normal_tile.hpp -- one star's weighted normal equations as one 16 x 16 fp64 tile, and the scaled Cholesky solve behind it: shared
// by payne_lmfit_update, payne_lmfit_update_poly (k_lmfit.hip, lmfit_core.hpp) and payne_contfit_batch (k_contfit.hip,
// contfit_core.hpp).  Plain C++, host / device: the same source runs in the kernels and on the host (tests/emul/*_emul.cpp, also
// under ASan / UBSan); the device-only parts are under __HIPCC__.  Nothing here indexes a private array: every array is the caller's
// (LDS or global memory in a kernel), so the kernels have no scratch.
//   tile     R [rows <= 16][n] in fp64, whatever the caller forms a row from; G = R diag(w) R^T, G[i][j] for i, j < rows, the rest
//            of the 16 x 16 tile zero.
//   pixels   in groups of 16.  Lane (i = lane & 15, q = lane >> 4) of a wave holds pixels p0 + 4 q .. p0 + 4 q + 3 of row i and
//            feeds them to four consecutive v_mfma_f64_16x16x4_f64: instruction t sums pixels p0 + 4 k + t, k = 0..3
//            (A[i][k = q] = R[i][p], B[k = q][j = i] = R[i][p] w[p], the same lane's value times w, so nothing is transposed).
//            D[i = (lane >> 4) + 4 v][j = lane & 15], v = 0..3, is G.  The sixteen lanes of one q hold the same four pixels.
//   stripes  wave v of the workgroup's four owns the groups [v * gpw, (v + 1) * gpw), gpw = ceil(groups / 4); the four partial
//            tiles meet in LDS and are added in wave order, ((part0 + part1) + part2) + part3.
//   zero w   a pixel that does not count (beyond n, w == 0, a row the lane does not have, a pixel the caller drops) has both
//            operands replaced by zero by a select: the rows may hold NaN there.
//   host     tile_sums_host walks wave, group, t, q in that order.  (The matrix instruction's own order of the four products of
//            one instruction is the hardware's; on the host they are added k = 0..3.)
//   solve    scaled_solve: S = diag(A_kk^-1/2), Cholesky of S A S with a constant diagonal, x = S u.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define PAYNE_HD __host__ __device__ inline
#else
#define PAYNE_HD inline
#endif

namespace payne {
namespace ntile {

constexpr int kTile = 16;                         // rows and columns of G's tile
constexpr int kTileSize = kTile * kTile;
constexpr int kGroup = 16;                        // pixels of four matrix instructions
constexpr int kWave = 64, kWaves = 4, kThreads = kWave * kWaves;

// (Not v - v == 0: where v is a product the device compiler contracts the difference into fma(a, b, -v), the product's rounding
// error, which is not zero.)
PAYNE_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

PAYNE_HD int groups_of(int n) { return (n + kGroup - 1) / kGroup; }
PAYNE_HD int groups_per_wave(int n) { return (groups_of(n) + kWaves - 1) / kWaves; }
// the pixel that lane quarter q hands to instruction t of group `grp`
PAYNE_HD int pixel_of(int grp, int q, int t) { return kGroup * grp + 4 * q + t; }

// The pair a lane hands to the matrix instruction; `counts` = the pixel is inside n, has w != 0, is kept and the lane's row is one of R's.
PAYNE_HD void operand_pair(double r, double w, bool counts, double* a, double* b) {
  *a = counts ? r : 0.0;
  *b = counts ? r * w : 0.0;
}

// The tile on the host in the kernels' pixel order: G [16][16] of one star with `rows` rows.  row(p, r) is asked for every pixel
// inside n with w != 0, in the walk's order: it fills r [rows], row i of R at pixel p, and says whether the pixel is kept.
template <class Row>
inline void tile_sums_host(const double* w, int n, int rows, Row row, double* G) {
  for (int e = 0; e < kTileSize; ++e) G[e] = 0.0;
  const int gpw = groups_per_wave(n), groups = groups_of(n);
  double acc[kTileSize], a[kTile], b[kTile];
  for (int v = 0; v < kWaves; ++v) {
    for (int e = 0; e < kTileSize; ++e) acc[e] = 0.0;
    for (int grp = v * gpw; grp < (v + 1) * gpw && grp < groups; ++grp)
      for (int t = 0; t < 4; ++t)
        for (int q = 0; q < 4; ++q) {
          const int p = pixel_of(grp, q, t);
          if (!(p < n && w[p < n ? p : 0] != 0.0) || !row(p, a)) continue;   // (both operands zero: the sums do not change)
          for (int i = 0; i < rows; ++i) operand_pair(a[i], w[p], true, &a[i], &b[i]);
          for (int i = 0; i < rows; ++i)
            for (int j = 0; j < rows; ++j) acc[i * kTile + j] += a[i] * b[j];
        }
    for (int i = 0; i < rows; ++i)
      for (int j = 0; j < rows; ++j) {
        const int e = i * kTile + j;
        G[e] = v == 0 ? acc[e] : G[e] + acc[e];
      }
  }
}

// M [K][K] symmetric positive definite (the lower triangle is read and overwritten by its Cholesky factor), u [K] the right-hand
// side, overwritten by the solution.  False when a pivot is not positive.
PAYNE_HD bool cholesky_solve(double* M, double* u, int K) {
  for (int j = 0; j < K; ++j) {
    double d = M[j * K + j];
    for (int k = 0; k < j; ++k) d -= M[j * K + k] * M[j * K + k];
    if (!(d > 0.0) || !finite(d)) return false;
    d = sqrt(d);
    M[j * K + j] = d;
    for (int i = j + 1; i < K; ++i) {
      double s = M[i * K + j];
      for (int k = 0; k < j; ++k) s -= M[i * K + k] * M[j * K + k];
      M[i * K + j] = s / d;
    }
  }
  for (int i = 0; i < K; ++i) {                                     // L y = u
    double s = u[i];
    for (int k = 0; k < i; ++k) s -= M[i * K + k] * u[k];
    u[i] = s / M[i * K + i];
  }
  for (int i = K - 1; i >= 0; --i) {                                // L^T x = y
    double s = u[i];
    for (int k = i + 1; k < K; ++k) s -= M[k * K + i] * u[k];
    u[i] = s / M[i * K + i];
  }
  return true;
}

// x of (S A S + (diag - 1) I) u = S b, x = S u, with S = diag(A_kk^-1/2): A [K][lda] (the lower triangle and the diagonal are
// read), b [K] with stride ldb, `diag` the scaled matrix's constant diagonal.  work holds K * K + 2 K doubles: the scaled matrix,
// S, and x in work[K * K + K ..].  False: a diagonal element or a pivot is not positive, or x is not finite.
PAYNE_HD bool scaled_solve(const double* A, int lda, const double* b, int ldb, double diag, int K, double* work) {
  double* M = work;
  double* S = work + K * K;
  double* u = S + K;
  for (int k = 0; k < K; ++k) {
    const double d = A[k * lda + k];
    if (!(d > 0.0) || !finite(d)) return false;
    S[k] = 1.0 / sqrt(d);
  }
  for (int i = 0; i < K; ++i) {
    for (int j = 0; j < i; ++j) M[i * K + j] = A[i * lda + j] * S[i] * S[j];
    M[i * K + i] = diag;
    u[i] = b[i * ldb] * S[i];
  }
  if (!cholesky_solve(M, u, K)) return false;
  for (int k = 0; k < K; ++k) {
    u[k] *= S[k];
    if (!finite(u[k])) return false;
  }
  return true;
}

#if defined(__HIPCC__)
// ---- device only ------------------------------------------------------------------------------------------------------------
typedef double d4 __attribute__((ext_vector_type(4)));

// The loop, its loads and the callables a kernel hands it (PAYNE_TILE_CALLABLE behind a lambda's parameter list) are inlined before
// anything is optimised, so that the compiler meets one loop body, as if written out in the kernel.  Inlined piece by piece it
// folds the widening of a guarded fp32 load into the branch that loads it: conversions that then run ahead of the matrix
// instructions instead of between them (measured: 1 % of payne_lmfit_update_poly's launch; NOTES.md, 2026-10-21).
#define PAYNE_TILE_INLINE __device__ __forceinline__
#define PAYNE_TILE_CALLABLE __attribute__((always_inline))

// Four consecutive values from p (a multiple of four, p < n); `whole`: all four may be read.  <VEC>: one 16-byte load (two for fp64)
// where `whole`, and then a value beyond n is whatever the row holds there; otherwise element by element, the same values in the
// same places and zero beyond n.  No caller lets a pixel beyond n count.  (Not zeroed after the wide load: a select there needs the
// loaded value inside the branch that loads it, which makes every guarded load of a group wait for the one before.)
template <bool VEC>
PAYNE_TILE_INLINE void load4(const float* __restrict__ base, int p, int n, bool whole, float* v) {
  if (VEC && whole) {
    const float4 a = *reinterpret_cast<const float4*>(base + p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = p + t < n ? base[p + t] : 0.0f;
  }
}
template <bool VEC>
PAYNE_TILE_INLINE void load4(const double* __restrict__ base, int p, int n, bool whole, double* v) {
  if (VEC && whole) {
    const double2 a = *reinterpret_cast<const double2*>(base + p), b = *reinterpret_cast<const double2*>(base + p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = p + t < n ? base[p + t] : 0.0;
  }
}

// The wave's partial tile: its stripe of pixel groups, four matrix instructions a group in the order t = 0..3.  group(p) is asked
// once a group for the lane's four pixels p .. p + 3 (p = pixel_of(grp, lane >> 4, 0), which may be beyond n): it loads them and
// returns pixel(t, &r, &w) -> counts, asked once a pixel right before its matrix instruction: row i = lane & 15 of R there, the
// weight, whether the pixel counts.  (Two steps: a group's loads are issued together, and what a pixel costs on the vector pipeline
// sits between the four matrix instructions, each of which waits for the one before.)
template <class Group>
PAYNE_TILE_INLINE d4 wave_sums(int n, Group group) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int gpw = groups_per_wave(n), groups = groups_of(n);
  const int g0 = wave * gpw, g1 = g0 + gpw < groups ? g0 + gpw : groups;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int grp = g0; grp < g1; ++grp) {
    const auto pixel = group(pixel_of(grp, lane >> 4, 0));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double r, w, av, bv;
      const bool counts = pixel(t, &r, &w);
      operand_pair(r, w, counts, &av, &bv);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
  }
  return acc;
}

// The four waves' partial tiles into tile [256]: each wave stores its own to part, publish() is a workgroup barrier (or something
// that holds one), and thread e adds element e in wave order.  A barrier follows: every thread may read tile.
template <class Publish>
PAYNE_TILE_INLINE void sum_waves(const d4& acc, double (*part)[kTileSize], double* tile, Publish publish) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
  for (int v = 0; v < 4; ++v) part[wave][((lane >> 4) + 4 * v) * kTile + (lane & 15)] = acc[v];
  publish();
  tile[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  __syncthreads();
}
#endif

}  // namespace ntile

// The tile's size under the name it had first: the emulator programs of both fits (tests/emul/lmfit_emul.cpp, lmfit_poly_emul.cpp,
// contfit_emul.cpp) size their G arrays by payne::lmfit::kTileSize, and their sources are the same before and after the tile moved here.
namespace lmfit {
using ntile::kTile;
using ntile::kTileSize;
}  // namespace lmfit
}  // namespace payne
