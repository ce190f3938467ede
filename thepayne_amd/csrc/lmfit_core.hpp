// lmfit_core.hpp -- arithmetic of payne_lmfit_* (k_lmfit.hip): batched Levenberg-Marquardt, the rows of one star's normal equations
// and the per-star step behind them.  Plain C++, host / device: the same source runs in the kernels and on the host
// (tests/emul/lmfit_emul.cpp, lmfit_poly_emul.cpp, also under ASan / UBSan).  Nothing here indexes a private array: every array is the
// caller's (LDS or global memory in the kernel), so the kernel has no scratch.  The emulator's workspace is filled with NaN before
// every star, as LDS holds whatever the workgroup before left there.
//   tile     normal_tile.hpp's, of R = [rows 1..K ; flux - row 0] in fp64, [K + 1][n] (operand): A = G[:K][:K] = J^T W J,
//            g = G[:K][K] = J^T W r, chi^2 = G[K][K].  The pixel groups, the operand map, the select for w == 0 and the wave-order
//            sum are described there, once.
//   poly     payne_lmfit_update_poly: the same tile for a model times a Chebyshev series (cheb_series.hpp) whose coefficients are
//            the last P parameters, R = [p dm/dtheta ; m T_j ; flux - m p] formed from the caller's 1 + Km rows (operand_poly).
//   step     update_star below: decide, solve (normal_tile.hpp: scaled_solve), next trial, stop (include/payne_hip.h states the rules).
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/payne_hip.h"
#include "cheb_series.hpp"
#include "normal_tile.hpp"

namespace payne {
namespace lmfit {

namespace nt = payne::ntile;
using nt::finite;

constexpr int kMaxK = PAYNE_LMFIT_MAX_K;
constexpr int kWorkDoubles = 2 * kMaxK * kMaxK + 3 * kMaxK;   // update_star's workspace: the scaled matrix, S, u; the star's A, g

PAYNE_HD payne_lmfit_opts default_opts() { return payne_lmfit_opts{1e-3, 10.0, 10.0, 1e-12, 1e8, 1e-3, 50}; }

PAYNE_HD bool opts_ok(const payne_lmfit_opts& o) {
  return finite(o.lambda0) && finite(o.down) && finite(o.up) && finite(o.lambda_min) && finite(o.lambda_max) && finite(o.xtol) &&
         o.lambda_min >= 0.0 && o.lambda_max >= o.lambda_min && o.lambda0 >= o.lambda_min && o.lambda0 <= o.lambda_max && o.down >= 1.0 &&
         o.up >= 1.0 && o.xtol >= 0.0 && o.maxiter >= 1;
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------
// Row i of R at one pixel from the fp32 values there: `a` of rows[1 + i] for i < K, of row 0 (the model) for i == K, where f is the flux.
PAYNE_HD double operand(int i, int K, float a, float f) { return i < K ? (double)a : (double)f - (double)a; }

// With a continuum polynomial, K = Km + P parameters: Km of the caller's model m, then the P Chebyshev coefficients c of
// p(x) = sum_j c_j T_j(x) that multiplies it.  The rows of R at one pixel, from the fp32 values of the caller's 1 + Km rows, the flux
// f and x, in fp64:
//   i < Km        p dm/dtheta_i       one rounded product
//   Km <= i < K   m T_{i-Km}(x)       one rounded product
//   i == K        f - m p             one fma
// A lane of row i therefore needs one series in x (cheb_series.hpp): p, or T_j.  j: the lane's T_j, or -1 where it wants p.
PAYNE_HD int series_index(int i, int Km, int K) { return i >= Km && i < K ? i - Km : -1; }

// Row i of R at one pixel: `a` of rows[1 + i] for i < Km, of row 0 (the model) otherwise; s the lane's series there.
PAYNE_HD double operand_poly(int i, int K, float a, float f, double s) { return i < K ? (double)a * s : fma(-(double)a, s, (double)f); }

// The tile on the host in the kernel's pixel order: G [16][16] of one star.  rows [1 + K][ld].
inline void tile_sums_host(const float* rows, long long ld, const float* flux, const double* w, int n, int K, double* G) {
  nt::tile_sums_host(w, n, K + 1, [&](int p, double* r) {
    for (int i = 0; i <= K; ++i) r[i] = operand(i, K, rows[(size_t)(i < K ? 1 + i : 0) * (size_t)ld + (size_t)p], flux[p]);
    return true;
  }, G);
}

// The same with a continuum polynomial.  rows [1 + Km][ld], c [P], x [n].
inline void tile_sums_poly_host(const float* rows, long long ld, const float* flux, const double* w, const double* x, int n, int Km, int P,
                                const double* c, double* G) {
  const int K = Km + P;
  nt::tile_sums_host(w, n, K + 1, [&](int p, double* r) {
    for (int i = 0; i <= K; ++i)
      r[i] = operand_poly(i, K, rows[(size_t)(i < Km ? 1 + i : 0) * (size_t)ld + (size_t)p], flux[p],
                          chebs::series_value(c, series_index(i, Km, K), P, x[p]));
    return true;
  }, G);
}

// With Kp parameters that the spectrum does not see (payne_lmfit_update_phot; lmfit_phot_core.hpp adds their block), K = Km + Kp + P:
// they sit between the model's and the coefficients', rows Km .. Km + Kp - 1 of the tile are none of R's (a lane there is not live:
// both operands zero by the select), the series of row i >= Km + Kp is series_index(i, Km + Kp, K), and the lane's row of the caller's
// 1 + Km is row_of(i, Km) as before.
PAYNE_HD bool has_row(int i, int Km, int Kp, int K) { return i <= K && !(i >= Km && i < Km + Kp); }
PAYNE_HD int row_of(int i, int Km) { return i < Km ? 1 + i : 0; }

// The tile with that gap on the host.  rows [1 + Km][ld]; P == 0: the plain model (operand), c and x are not read.
inline void tile_sums_gap_host(const float* rows, long long ld, const float* flux, const double* w, const double* x, int n, int Km, int Kp,
                               int P, const double* c, double* G) {
  const int K = Km + Kp + P;
  nt::tile_sums_host(w, n, K + 1, [&](int p, double* r) {
    for (int i = 0; i <= K; ++i) {
      const float a = rows[(size_t)row_of(i, Km) * (size_t)ld + (size_t)p];
      if (!has_row(i, Km, Kp, K)) r[i] = 0.0;
      else if (P > 0) r[i] = operand_poly(i, K, a, flux[p], chebs::series_value(c, series_index(i, Km + Kp, K), P, x[p]));
      else r[i] = operand(i, K, a, flux[p]);
    }
    return true;
  }, G);
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
PAYNE_HD double clip_one(double v, double lo, double hi, int k, unsigned* mask) {
  if (v < lo) { v = lo; *mask |= 1u << k; }
  if (v > hi) { v = hi; *mask |= 1u << k; }
  return v;
}

PAYNE_HD void begin_star(const State& st, size_t b, int K, const double* x0, const Box& box, double lambda0) {
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

// The step of star b behind its tile G [16][16] (evaluated at the star's x_trial).  work holds kWorkDoubles: scaled_solve's M, S, u,
// then the star's matrix and gradient, which the solve reads from there -- nothing this thread writes to the handle's arrays is
// read back from them.
PAYNE_HD void update_star(const State& st, size_t b, int K, const double* G, const payne_lmfit_opts& o, const Box& box, double* work) {
  if (st.status[b] != PAYNE_LMFIT_RUNNING) return;
  double* xb = st.x_best + b * (size_t)K;
  double* xt = st.x_trial + b * (size_t)K;
  double* A = st.A + b * (size_t)(K * K);
  double* g = st.g + b * (size_t)K;
  double* u = work + K * K + K;                                     // scaled_solve's delta of (S A S + lambda I) u = S g; then the next trial
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
  if (!nt::scaled_solve(As, K, gs, 1, 1.0 + lambda, K, work)) {
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
