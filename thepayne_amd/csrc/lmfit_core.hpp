// lmfit_core.hpp -- arithmetic of payne_lmfit_* (k_lmfit.hip): batched Levenberg-Marquardt, one star's normal equations as one
// 16 x 16 tile and the per-star step behind them.  Plain C++, host / device: the same source runs in the kernels and on the host
// (tests/emul/lmfit_emul.cpp, also under ASan / UBSan).  Nothing here indexes a private array: every array is the caller's (LDS or
// global memory in the kernel), so the kernel has no scratch.  The emulator's workspace is filled with NaN before every star, as
// LDS holds whatever the workgroup before left there.
//   tile     R = [rows 1..K ; flux - row 0] in fp64, [K + 1][n]; G = R diag(w) R^T, G[i][j] for i, j <= K, the rest of the 16 x 16
//            tile zero.  A = G[:K][:K] = J^T W J, g = G[:K][K] = J^T W r, chi^2 = G[K][K].
//   pixels   in groups of 16.  Lane (i = lane & 15, q = lane >> 4) of a wave holds pixels p0 + 4 q .. p0 + 4 q + 3 of row i (16 bytes of
//            fp32) and feeds them to four consecutive matrix instructions: instruction t sums pixels p0 + 4 k + t, k = 0..3
//            (A[i][k] = R[i][p], B[k][j] = R[j][p] w[p], the same lane's value times w).  Wave v of the workgroup's four owns the
//            groups [v * gpw, (v + 1) * gpw), gpw = ceil(groups / 4); the four partial tiles are added in wave order.
//   poly     payne_lmfit_update_poly: the same tile for a model times a Chebyshev series whose coefficients are the last P parameters,
//            R = [p dm/dtheta ; m T_j ; flux - m p] formed from the caller's 1 + Km rows (below: series4, operand_poly,
//            tile_sums_poly_host; tests/emul/lmfit_poly_emul.cpp).  The series' recurrence is the one contfit_core.hpp uses.
//   zero w   a pixel with w == 0 (or beyond n) has both operands replaced by zero by a select: the rows may hold NaN there.
//   step     update_star below: decide, solve, next trial, stop (include/payne_hip.h states the rules).
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/payne_hip.h"

#if defined(__HIPCC__)
#define PAYNE_LMFIT_HD __host__ __device__ inline
#else
#define PAYNE_LMFIT_HD inline
#endif

namespace payne {
namespace lmfit {

constexpr int kMaxK = PAYNE_LMFIT_MAX_K;
constexpr int kTile = 16;                         // rows and columns of G's tile
constexpr int kTileSize = kTile * kTile;
constexpr int kGroup = 16;                        // pixels of four matrix instructions
constexpr int kWave = 64, kWaves = 4, kThreads = kWave * kWaves;
constexpr int kWorkDoubles = 2 * kMaxK * kMaxK + 3 * kMaxK;   // update_star's workspace: the scaled matrix, S, u; the star's A, g

PAYNE_LMFIT_HD payne_lmfit_opts default_opts() { return payne_lmfit_opts{1e-3, 10.0, 10.0, 1e-12, 1e8, 1e-3, 50}; }

// (Not v - v == 0: where v is a product the device compiler contracts the difference into fma(a, b, -v), the product's rounding
// error, which is not zero.)
PAYNE_LMFIT_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

PAYNE_LMFIT_HD bool opts_ok(const payne_lmfit_opts& o) {
  return finite(o.lambda0) && finite(o.down) && finite(o.up) && finite(o.lambda_min) && finite(o.lambda_max) && finite(o.xtol) &&
         o.lambda_min >= 0.0 && o.lambda_max >= o.lambda_min && o.lambda0 >= o.lambda_min && o.lambda0 <= o.lambda_max && o.down >= 1.0 &&
         o.up >= 1.0 && o.xtol >= 0.0 && o.maxiter >= 1;
}

// ---- the sums ---------------------------------------------------------------------------------------------------------------
PAYNE_LMFIT_HD int groups_of(int n) { return (n + kGroup - 1) / kGroup; }
PAYNE_LMFIT_HD int groups_per_wave(int n) { return (groups_of(n) + kWaves - 1) / kWaves; }
// the pixel that lane quarter q hands to instruction t of group `grp`
PAYNE_LMFIT_HD int pixel_of(int grp, int q, int t) { return kGroup * grp + 4 * q + t; }

// Row i of R at one pixel from the fp32 values there: `a` of rows[1 + i] for i < K, of row 0 (the model) for i == K, where f is the flux.
PAYNE_LMFIT_HD double operand(int i, int K, float a, float f) { return i < K ? (double)a : (double)f - (double)a; }

// The pair a lane hands to the matrix instruction; `counts` = the pixel is inside n, has w != 0 and the lane's row is one of R's.
PAYNE_LMFIT_HD void operand_pair(double r, double w, bool counts, double* a, double* b) {
  *a = counts ? r : 0.0;
  *b = counts ? r * w : 0.0;
}

// The tile on the host in the kernel's pixel order: G [16][16] of one star.  (The matrix instruction's own order of the four
// products of one instruction is the hardware's; here they are added k = 0..3.)
inline void tile_sums_host(const float* rows, long long ld, const float* flux, const double* w, int n, int K, double* G) {
  for (int e = 0; e < kTileSize; ++e) G[e] = 0.0;
  const int gpw = groups_per_wave(n), groups = groups_of(n);
  for (int i = 0; i <= K; ++i)
    for (int j = 0; j <= K; ++j) {
      double total = 0.0;
      for (int v = 0; v < kWaves; ++v) {
        double acc = 0.0;
        for (int grp = v * gpw; grp < (v + 1) * gpw && grp < groups; ++grp)
          for (int t = 0; t < 4; ++t)
            for (int q = 0; q < 4; ++q) {
              const int p = pixel_of(grp, q, t);
              const bool counts = p < n && w[p < n ? p : 0] != 0.0;
              const size_t pc = counts ? (size_t)p : 0;
              double ai, bi, aj, bj;
              operand_pair(operand(i, K, rows[(size_t)(i < K ? 1 + i : 0) * (size_t)ld + pc], flux[pc]), w[pc], counts, &ai, &bi);
              operand_pair(operand(j, K, rows[(size_t)(j < K ? 1 + j : 0) * (size_t)ld + pc], flux[pc]), w[pc], counts, &aj, &bj);
              acc += ai * bj;
            }
        total = v == 0 ? acc : total + acc;
      }
      G[i * kTile + j] = total;
    }
}

// ---- Chebyshev series (contfit_core.hpp uses these under its own names) -----------------------------------------------------
// The three-term recurrence, written once: T_k = 2 x T_k-1 - T_k-2.
PAYNE_LMFIT_HD double cheb_next(double x, double t1, double t0) { return fma(2.0 * x, t1, -t0); }

// T_i(x).
PAYNE_LMFIT_HD double cheb(int i, double x) {
  if (i == 0) return 1.0;
  double t0 = 1.0, t1 = x;
  for (int k = 2; k <= i; ++k) {
    const double t2 = cheb_next(x, t1, t0);
    t0 = t1;
    t1 = t2;
  }
  return t1;
}

// T_i at four abscissae, the same values: one loop for the four, and a trip count (P) that every lane of a wave shares -- the lanes
// differ only in the step they keep.  (Four calls of cheb are four loops whose length differs from lane to lane; measured, NOTES.md.)
PAYNE_LMFIT_HD void cheb4(int i, int P, const double* x, double* T) {
  double t0[4], t1[4];
  for (int t = 0; t < 4; ++t) {
    t0[t] = 1.0;
    t1[t] = x[t];
    T[t] = i == 0 ? 1.0 : x[t];
  }
  for (int k = 2; k < P; ++k)
    for (int t = 0; t < 4; ++t) {
      const double t2 = cheb_next(x[t], t1[t], t0[t]);
      t0[t] = t1[t];
      t1[t] = t2;
      T[t] = k == i ? t2 : T[t];
    }
}

// p(x) = sum_j c_j T_j(x), j ascending, on the same recurrence.
PAYNE_LMFIT_HD double poly_value(const double* c, int P, double x) {
  double s = c[0];
  if (P > 1) s = fma(c[1], x, s);
  double t0 = 1.0, t1 = x;
  for (int k = 2; k < P; ++k) {
    const double t2 = cheb_next(x, t1, t0);
    s = fma(c[k], t2, s);
    t0 = t1;
    t1 = t2;
  }
  return s;
}

// poly_value at four abscissae, the same values: each coefficient is read once for the four.
PAYNE_LMFIT_HD void poly4(const double* c, int P, const double* x, double* pv) {
  double t0[4], t1[4];
  const double c0 = c[0], c1 = P > 1 ? c[1] : 0.0;
  for (int t = 0; t < 4; ++t) {
    t0[t] = 1.0;
    t1[t] = x[t];
    pv[t] = P > 1 ? fma(c1, x[t], c0) : c0;
  }
  for (int k = 2; k < P; ++k) {
    const double ck = c[k];
    for (int t = 0; t < 4; ++t) {
      const double t2 = cheb_next(x[t], t1[t], t0[t]);
      pv[t] = fma(ck, t2, pv[t]);
      t0[t] = t1[t];
      t1[t] = t2;
    }
  }
}

// ---- the sums with a continuum polynomial (payne_lmfit_update_poly) -----------------------------------------------------------
// K = Km + P parameters: Km of the caller's model m, then the P Chebyshev coefficients c of p(x) = sum_j c_j T_j(x) that multiplies
// it.  The rows of R at one pixel, from the fp32 values of the caller's 1 + Km rows, the flux f and x, in fp64:
//   i < Km        p dm/dtheta_i       one rounded product
//   Km <= i < K   m T_{i-Km}(x)       one rounded product
//   i == K        f - m p             one fma
// A lane of row i therefore needs one series in x: p (row i < Km or i == K), or T_j, which is the series of the unit vector e_j --
// fma(1, T_j, 0) = T_j and fma(0, T_k, s) = s are exact while every T_k is finite, which |x| <= 1 ensures.  So every lane runs
// poly_value's loop on its own coefficients, P - 2 steps whatever its row, and the values are poly_value's and cheb's.
// j: the lane's T_j, or -1 where it wants p.
PAYNE_LMFIT_HD int series_index(int i, int Km, int K) { return i >= Km && i < K ? i - Km : -1; }
PAYNE_LMFIT_HD double series_coef(const double* c, int j, int k) { return j < 0 ? c[k] : (k == j ? 1.0 : 0.0); }

// The lane's series at one abscissa.
PAYNE_LMFIT_HD double series_value(const double* c, int j, int P, double x) {
  double s = series_coef(c, j, 0);
  if (P > 1) s = fma(series_coef(c, j, 1), x, s);
  double t0 = 1.0, t1 = x;
  for (int k = 2; k < P; ++k) {
    const double t2 = cheb_next(x, t1, t0);
    s = fma(series_coef(c, j, k), t2, s);
    t0 = t1;
    t1 = t2;
  }
  return s;
}

// series_value at four abscissae, the same values (poly4's loop).
PAYNE_LMFIT_HD void series4(const double* c, int j, int P, const double* x, double* sv) {
  double t0[4], t1[4];
  const double c0 = series_coef(c, j, 0), c1 = P > 1 ? series_coef(c, j, 1) : 0.0;
  for (int t = 0; t < 4; ++t) {
    t0[t] = 1.0;
    t1[t] = x[t];
    sv[t] = P > 1 ? fma(c1, x[t], c0) : c0;
  }
  for (int k = 2; k < P; ++k) {
    const double ck = series_coef(c, j, k);
    for (int t = 0; t < 4; ++t) {
      const double t2 = cheb_next(x[t], t1[t], t0[t]);
      sv[t] = fma(ck, t2, sv[t]);
      t0[t] = t1[t];
      t1[t] = t2;
    }
  }
}

// Row i of R at one pixel: `a` of rows[1 + i] for i < Km, of row 0 (the model) otherwise; s the lane's series there.
PAYNE_LMFIT_HD double operand_poly(int i, int K, float a, float f, double s) { return i < K ? (double)a * s : fma(-(double)a, s, (double)f); }

// The tile on the host in the kernel's pixel order (tile_sums_host): G [16][16] of one star.  rows [1 + Km][ld], c [P], x [n].
inline void tile_sums_poly_host(const float* rows, long long ld, const float* flux, const double* w, const double* x, int n, int Km, int P,
                                const double* c, double* G) {
  const int K = Km + P;
  for (int e = 0; e < kTileSize; ++e) G[e] = 0.0;
  const int gpw = groups_per_wave(n), groups = groups_of(n);
  double acc[kTileSize];
  for (int v = 0; v < kWaves; ++v) {
    for (int e = 0; e < kTileSize; ++e) acc[e] = 0.0;
    for (int grp = v * gpw; grp < (v + 1) * gpw && grp < groups; ++grp)
      for (int t = 0; t < 4; ++t)
        for (int q = 0; q < 4; ++q) {
          const int p = pixel_of(grp, q, t);
          if (!(p < n && w[p < n ? p : 0] != 0.0)) continue;         // (both operands zero: the sums do not change)
          double a[kTile], b[kTile];
          for (int i = 0; i <= K; ++i) {
            const float ai = rows[(size_t)(i < Km ? 1 + i : 0) * (size_t)ld + (size_t)p];
            operand_pair(operand_poly(i, K, ai, flux[p], series_value(c, series_index(i, Km, K), P, x[p])), w[p], true, &a[i], &b[i]);
          }
          for (int i = 0; i <= K; ++i)
            for (int j = 0; j <= K; ++j) acc[i * kTile + j] += a[i] * b[j];
        }
    for (int i = 0; i <= K; ++i)
      for (int j = 0; j <= K; ++j) {
        const int e = i * kTile + j;
        G[e] = v == 0 ? acc[e] : G[e] + acc[e];
      }
  }
}

// ---- one star's state -------------------------------------------------------------------------------------------------------
// The handle's arrays, one entry (or block) a star.
struct State {
  double* x_best;      // [B][K]
  double* x_trial;     // [B][K]
  double* A;           // [B][K][K]  the stored normal matrix, at x_best
  double* g;           // [B][K]     the stored gradient J^T W r
  double* chisq;       // [B]        of x_best
  double* lambda;      // [B]
  int* status;         // [B]
  int* niter;          // [B]        evaluations so far
  unsigned* at_bound;  // [B]
};
struct Box {
  double lo[kMaxK], hi[kMaxK];
};

// v clipped into [lo, hi]; sets bit k of *mask where it was.
PAYNE_LMFIT_HD double clip_one(double v, double lo, double hi, int k, unsigned* mask) {
  if (v < lo) { v = lo; *mask |= 1u << k; }
  if (v > hi) { v = hi; *mask |= 1u << k; }
  return v;
}

PAYNE_LMFIT_HD void begin_star(const State& st, size_t b, int K, const double* x0, const Box& box, double lambda0) {
  unsigned mask = 0u;
  for (int k = 0; k < K; ++k) {
    const double v = clip_one(x0[k], box.lo[k], box.hi[k], k, &mask);
    st.x_trial[b * (size_t)K + k] = v;
    st.x_best[b * (size_t)K + k] = v;
    st.g[b * (size_t)K + k] = 0.0;
  }
  for (int e = 0; e < K * K; ++e) st.A[b * (size_t)(K * K) + e] = 0.0;
  st.at_bound[b] = mask;
  st.chisq[b] = 0.0;
  st.lambda[b] = lambda0;
  st.status[b] = PAYNE_LMFIT_RUNNING;
  st.niter[b] = 0;
}

// M [K][K] symmetric positive definite (the lower triangle is read and overwritten by its Cholesky factor), u [K] the right-hand
// side, overwritten by the solution.  False when a pivot is not positive.
PAYNE_LMFIT_HD bool cholesky_solve(double* M, double* u, int K) {
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

// delta of (S A S + lambda I) u = S g, delta = S u, left in work[K * K + K ..]; work holds K * K + 2 K doubles.  False: singular.
PAYNE_LMFIT_HD bool damped_step(const double* A, const double* g, double lambda, int K, double* work) {
  double* M = work;
  double* S = work + K * K;
  double* u = S + K;
  for (int k = 0; k < K; ++k) {
    const double d = A[k * K + k];
    if (!(d > 0.0) || !finite(d)) return false;
    S[k] = 1.0 / sqrt(d);
  }
  for (int i = 0; i < K; ++i) {
    for (int j = 0; j < i; ++j) M[i * K + j] = A[i * K + j] * S[i] * S[j];
    M[i * K + i] = 1.0 + lambda;
    u[i] = g[i] * S[i];
  }
  if (!cholesky_solve(M, u, K)) return false;
  for (int k = 0; k < K; ++k) {
    u[k] *= S[k];
    if (!finite(u[k])) return false;
  }
  return true;
}

// The step of star b behind its tile G [16][16] (evaluated at the star's x_trial).  work holds kWorkDoubles: damped_step's M, S, u,
// then the star's matrix and gradient, which the solve reads from there -- nothing this thread writes to the handle's arrays is
// read back from them.
PAYNE_LMFIT_HD void update_star(const State& st, size_t b, int K, const double* G, const payne_lmfit_opts& o, const Box& box, double* work) {
  if (st.status[b] != PAYNE_LMFIT_RUNNING) return;
  double* xb = st.x_best + b * (size_t)K;
  double* xt = st.x_trial + b * (size_t)K;
  double* A = st.A + b * (size_t)(K * K);
  double* g = st.g + b * (size_t)K;
  double* u = work + K * K + K;                                     // damped_step's delta; then the next trial
  double* As = work + K * K + 2 * K;
  double* gs = As + K * K;
  const double chisq_t = G[K * kTile + K];
  const int evals = st.niter[b] + 1;
  const bool first = evals == 1;
  st.niter[b] = evals;
  if (first && !finite(chisq_t)) {                                  // (x_trial is x_best since begin)
    st.chisq[b] = chisq_t;
    st.status[b] = PAYNE_LMFIT_NAN;
    return;
  }
  const bool accept = first || (finite(chisq_t) && chisq_t <= st.chisq[b]);
  const double lambda_tried = st.lambda[b];
  double lambda;
  if (accept) {
    for (int i = 0; i < K; ++i) {
      for (int j = i; j < K; ++j) {                                 // the upper triangle, mirrored
        const double v = G[i * kTile + j];
        As[i * K + j] = As[j * K + i] = v;
        A[i * K + j] = A[j * K + i] = v;
      }
      gs[i] = g[i] = G[i * kTile + K];
    }
    st.chisq[b] = chisq_t;
    lambda = lambda_tried / o.down;
    lambda = lambda > o.lambda_min ? lambda : o.lambda_min;
  } else {
    for (int e = 0; e < K * K; ++e) As[e] = A[e];
    for (int k = 0; k < K; ++k) gs[k] = g[k];
    lambda = lambda_tried * o.up;
    lambda = lambda < o.lambda_max ? lambda : o.lambda_max;
  }
  st.lambda[b] = lambda;
  int status = PAYNE_LMFIT_RUNNING;
  if (!damped_step(As, gs, lambda, K, work)) {
    status = PAYNE_LMFIT_SINGULAR;
  } else {
    unsigned mask = 0u;
    double dmax = 0.0;
    for (int k = 0; k < K; ++k) {
      const double base = accept ? xt[k] : xb[k];
      const double v = clip_one(base + u[k], box.lo[k], box.hi[k], k, &mask);
      const double d = fabs(v - base) * sqrt(As[k * K + k]);
      dmax = d > dmax ? d : dmax;
      u[k] = v;
    }
    st.at_bound[b] = mask;
    if (accept && dmax < o.xtol) status = PAYNE_LMFIT_CONVERGED;
    else if (!accept && lambda_tried >= o.lambda_max) status = PAYNE_LMFIT_STALLED;
    else if (evals >= o.maxiter) status = PAYNE_LMFIT_MAXITER;
  }
  st.status[b] = status;
  for (int k = 0; k < K; ++k) {                                     // a finished star's x_trial is its x_best
    const double base = accept ? xt[k] : xb[k];
    if (accept) xb[k] = base;
    xt[k] = status == PAYNE_LMFIT_RUNNING ? u[k] : base;
  }
}

}  // namespace lmfit
}  // namespace payne
