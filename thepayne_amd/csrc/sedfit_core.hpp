// sedfit_core.hpp -- arithmetic of payne_sedfit_* (k_sedfit.hip): the photometric magnitudes of GenMod.genphot / genphot_scaled with
// their derivatives in the likelihood's own parameters, and the Levenberg-Marquardt fit of a star's magnitudes that needs nothing
// else.  Plain C++, host / device: the same source runs in the kernels and on the host (tests/emul/sedfit_emul.cpp, also under
// ASan / UBSan).  Nothing here indexes a private array: every array is the caller's.
//   parameters  dist rows [Teff, logg, FeH, aFe, logR, Dist, Av], scaled rows [Teff, logg, FeH, aFe, logA, Av] (sed_row, mode 1; Rv is
//               3.1 as the likelihood has it).  Teff, logg, FeH, aFe and Av are inputs 0..4 of the per-filter nets and can carry a
//               tangent; the others enter the magnitude formula alone.
//   net         fastANN.eval (6 -> H -> H -> 1, sigmoids, fp64 on fp32 weights) in forward mode, xs the encoded labels:
//                 z1 = W1 xs + b1, a1 = s(z1), a1'_d = a1 (1 - a1) (W1[:, d] / (xmax_d - xmin_d))
//                 z2 = W2 a1 + b2, a2 = s(z2), a2'_d = a2 (1 - a2) (W2 a1'_d)
//                 BC = w3 a2 + b3,             dBC/dx_d = w3 a2'_d
//               The quotient W1[:, d] / (xmax_d - xmin_d) is a table (tangent_weight): the handle forms it once.  net_forward is
//               the scalar form; the kernels run the two matrix products of a block of stars on the fp64 matrix instruction.
//   chain       row_terms, mag_grad: the magnitude formulae of sed_core.hpp (its label encoding, magnitude terms and high-Av offset are
//               called here, not restated) and d m / d parameter.  At Av >= 5
//               the nets are evaluated at Av = 0 and dBC/dAv is the table's -c1 (c2 + c3 Rv + c4 Rv^2).  Where the magnitude is NaN
//               (a NaN label, a filter without a row in the table at Av >= 5) every derivative is NaN.
//   fit         R = [d m / d theta_free ; obs - m], G = R diag(w) R^T over the filters in ascending order (tile_add, one fma an
//               element and filter; w == 0: the filter is ignored whatever it holds), Gaussian priors on top (add_priors), then
//               lmfit_core.hpp's update_star unchanged.
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/payne_hip.h"
#include "lmfit_core.hpp"
#include "sed_core.hpp"

namespace payne {
namespace sedfit {

namespace lm = payne::lmfit;
using lm::finite;
using lm::kTile;

constexpr int kMaxK = PAYNE_SEDFIT_MAX_K;        // parameters of a dist row; a scaled row has six
constexpr int kNetIn = 6;                        // inputs of a net: Teff, logg, FeH, aFe, Av, Rv
constexpr int kMaxTan = 5;                       // ... of which Rv never carries a tangent
constexpr int kMaxH = kSedMaxH;                  // the widest net (the tile's width; a name the host programs use)
constexpr double kLn10 = 2.302585092994046;

PAYNE_HD int n_pars(int photscale) { return photscale ? 6 : 7; }
// the net input that parameter p of a row is, or -1
PAYNE_HD int net_input(int photscale, int p) { return p < 4 ? p : (p == n_pars(photscale) - 1 ? 4 : -1); }
PAYNE_HD int stars_per_tile(int Kn) { return kSedCandsMax / (1 + Kn); }   // (star, tangent) rows of a tile

// Which parameters are fitted: free parameter k is parameter par[k] of the row (ascending); Kn of them are net inputs, tangent
// t = 0 .. Kn - 1 is net input tan_in[t], and tan_of[p] is the tangent of parameter p (-1: none).
struct Plan {
  int photscale, P, K, Kn;
  int par[kMaxK], tan_in[kMaxTan], tan_of[kMaxK];
};
PAYNE_HD bool make_plan(int photscale, unsigned free_mask, Plan* pl) {
  const int P = n_pars(photscale);
  pl->photscale = photscale; pl->P = P; pl->K = 0; pl->Kn = 0;
  for (int t = 0; t < kMaxTan; ++t) pl->tan_in[t] = 0;
  for (int p = 0; p < kMaxK; ++p) { pl->par[p] = 0; pl->tan_of[p] = -1; }
  if ((photscale != 0 && photscale != 1) || free_mask == 0u || (free_mask >> P) != 0u) return false;
  for (int p = 0; p < P; ++p) {
    if (!((free_mask >> p) & 1u)) continue;
    pl->par[pl->K++] = p;
    const int d = net_input(photscale, p);
    if (d >= 0) { pl->tan_of[p] = pl->Kn; pl->tan_in[pl->Kn++] = d; }
  }
  return true;
}

// payne_sedfit_run's checks of what the host holds: lo, hi [K] in the order of the free parameters.
PAYNE_HD int check_run(int photscale, unsigned free_mask, const double* lo, const double* hi, const payne_lmfit_opts* opts) {
  Plan pl;
  if (!make_plan(photscale, free_mask, &pl) || !lo || !hi) return PAYNE_E_INVALID;
  if (opts && !lm::opts_ok(*opts)) return PAYNE_E_INVALID;
  for (int k = 0; k < pl.K; ++k) {
    if (!finite(lo[k]) || !finite(hi[k]) || !(lo[k] < hi[k])) return PAYNE_E_INVALID;
    if (net_input(photscale, pl.par[k]) == 4 && !(hi[k] < 5.0)) return PAYNE_E_INVALID;   // the model jumps at Av = 5
  }
  return PAYNE_OK;
}

// ---- the nets -------------------------------------------------------------------------------------------------------------------
// One filter's net as fastANN stacks it: w1 [H][6], b1 [H], w2 [H][H] (w2[h][k]), b2 [H], w3 [H], b3.
struct Net {
  int H;
  const float *w1, *b1, *w2, *b2, *w3;
  float b3;
};

// A row's encoded labels (sed_core.hpp: sed_encode) and what the high-Av branch needs.
struct Row {
  double xs[kNetIn];
  double av;
  bool hi;
};
PAYNE_HD void encode(const double* pars, int photscale, const double* xmin, const double* xden, Row* r) {
  r->av = pars[n_pars(photscale) - 1];
  r->hi = sed_hi_av(r->av);
  sed_encode(pars, r->av, kSedRv, r->hi, xmin, xden, r->xs);
}

// W1[h][d] / (xmax_d - xmin_d): what a unit tangent of input d is behind the first layer's product.
PAYNE_HD double tangent_weight(float w1_hd, double xden_d) { return (double)w1_hd / xden_d; }

// (the host's sigmoid; the kernels use sed_core.hpp's sed_sigmoid_n)
inline double sigmoid_host(double z) { return 1.0 / (1.0 + exp(-z)); }

// The scalar forward-mode pass (host): BC and dBC/dx for the Kn tangents tan_in[t] (derivatives with respect to the labels themselves).
// work holds 2 H (1 + Kn) doubles.
inline void net_forward(const Net& n, const double* xs, const double* xden, int Kn, const int* tan_in, double* work, double* bc, double* dbc) {
  const int H = n.H;
  double* a1 = work;                  // [H], then d1 [Kn][H]
  double* a2 = work + (size_t)H * (1 + Kn);
  for (int h = 0; h < H; ++h) {
    double z = (double)n.b1[h];
    for (int d = 0; d < kNetIn; ++d) z = fma((double)n.w1[h * kNetIn + d], xs[d], z);
    const double a = sigmoid_host(z), sp = a * (1.0 - a);
    a1[h] = a;
    for (int t = 0; t < Kn; ++t) a1[(size_t)H * (1 + t) + h] = sp * tangent_weight(n.w1[h * kNetIn + tan_in[t]], xden[tan_in[t]]);
  }
  for (int h = 0; h < H; ++h) {
    double z = (double)n.b2[h];
    for (int k = 0; k < H; ++k) z = fma((double)n.w2[(size_t)h * H + k], a1[k], z);
    const double a = sigmoid_host(z), sp = a * (1.0 - a);
    a2[h] = a;
    for (int t = 0; t < Kn; ++t) {
      double zt = 0.0;
      for (int k = 0; k < H; ++k) zt = fma((double)n.w2[(size_t)h * H + k], a1[(size_t)H * (1 + t) + k], zt);
      a2[(size_t)H * (1 + t) + h] = sp * zt;
    }
  }
  double s = (double)n.b3;
  for (int k = 0; k < H; ++k) s = fma((double)n.w3[k], a2[k], s);
  *bc = s;
  for (int t = 0; t < Kn; ++t) {
    double st = 0.0;
    for (int k = 0; k < H; ++k) st = fma((double)n.w3[k], a2[(size_t)H * (1 + t) + k], st);
    dbc[t] = st;
  }
}

// ---- the chain rule -------------------------------------------------------------------------------------------------------------
// What the magnitudes of a row share over the filters (sed_core.hpp's a1, a2 for a theta row, and the two derivatives that cost a
// division): two logarithms and two quotients a row, not a filter.  m = (a1 - BC) + a2.
struct RowTerms {
  double a1, a2, dteff, ddist;
};
PAYNE_HD void row_terms(int photscale, const double* pars, RowTerms* t) {
  const double logt = log10(pars[0]);                               // genmod.py:124,172
  if (photscale) {
    sed_terms_scaled(pars[4], logt, t->a1, t->a2);                  // genphot_scaled, predictsed.py:99-101
    t->ddist = 0.0;
  } else {
    sed_terms_dist(sed_theta_logl(pars[4], logt), pars[5], t->a1, t->a2);
    t->ddist = 5.0 / (pars[5] * kLn10);
  }
  t->dteff = 10.0 / (pars[0] * kLn10);
}

// The magnitude of one filter and its derivatives with respect to all P parameters of the row.  t: the row's terms; av: its Av;
// bc: the net's output; dbc [5]: its derivatives with respect to net inputs 0..4 (an entry that is not needed may hold anything: it
// reaches only its own column); hi: the row's Av >= 5; c: the filter's row [5] of the high-Av table or NULL.  dm [P].
PAYNE_HD void mag_grad(int photscale, const RowTerms& t, double av, double bc, const double* dbc, bool hi, const double* c, double* m, double* dm) {
  const double nan = __builtin_nan("");
  const int P = n_pars(photscale);
  double dav = dbc[4];
  if (hi) {                                                         // highred.py:19-25
    bc = bc - sed_hiav_offset(c, av, kSedRv);
    dav = c ? -(c[1] * sed_hiav_slope(c, kSedRv)) : nan;
  }
  const double mag = (t.a1 - bc) + t.a2;
  *m = mag;
  dm[0] = -dbc[0] - t.dteff;
  for (int p = 1; p < 4; ++p) dm[p] = -dbc[p];
  if (photscale) {
    dm[4] = 5.0;
  } else {
    dm[4] = -5.0;
    dm[5] = t.ddist;
  }
  dm[P - 1] = -dav;
  if (mag != mag)
    for (int p = 0; p < P; ++p) dm[p] = nan;
}

// ---- the fit --------------------------------------------------------------------------------------------------------------------
// One element of G behind one counting filter.
PAYNE_HD double tile_add(double g, double ri, double rj, double w) { return fma(ri * w, rj, g); }

// R [K + 1] of one filter from the magnitude and its derivatives.
PAYNE_HD void residual_row(const Plan& pl, double m, const double* dm, double obs, double* R) {
  for (int k = 0; k < pl.K; ++k) R[k] = dm[pl.par[k]];
  R[pl.K] = obs - m;
}

PAYNE_HD bool has_prior(double sigma) { return finite(sigma) && sigma > 0.0; }

// Gaussian priors of one star on its tile G [.][16]: x the point G was evaluated at, mu, sigma [K] (NULL: none).
PAYNE_HD void add_priors(double* G, int K, const double* x, const double* mu, const double* sigma) {
  if (!mu || !sigma) return;
  for (int k = 0; k < K; ++k) {
    if (!has_prior(sigma[k])) continue;
    const double iv = 1.0 / (sigma[k] * sigma[k]), d = mu[k] - x[k];
    G[k * kTile + k] += iv;
    G[k * kTile + K] = fma(d, iv, G[k * kTile + K]);
    G[K * kTile + K] = fma(d * d, iv, G[K * kTile + K]);
  }
}

// The filters that count, and whether they and the priors can determine K parameters.
PAYNE_HD int count_filters(const double* w, int F) {
  int n = 0;
  for (int f = 0; f < F; ++f) n += w[f] != 0.0 ? 1 : 0;
  return n;
}
PAYNE_HD bool too_few(int nfilt, int K, const double* sigma) {
  int n = nfilt;
  if (sigma)
    for (int k = 0; k < K; ++k) n += has_prior(sigma[k]) ? 1 : 0;
  return n < K;
}

// update_star's workspace for K parameters, and a star's tile: rows 0 .. K of a 16-column tile.
PAYNE_HD int work_doubles(int K) { return 2 * K * K + 3 * K; }
PAYNE_HD int tile_doubles(int K) { return (K + 1) * kTile; }

}  // namespace sedfit
}  // namespace payne
