// contfit_core.hpp -- arithmetic of payne_contfit_batch (k_contfit.hip): per star the Chebyshev coefficients c that minimise
// sum_p w_p (f_p - m_p sum_j c_j T_j(x_p))^2 for a given model row m, with optional kappa-sigma clipping, and the spectrum divided by
// that polynomial.  Plain C++, host / device: the same source runs in the kernel and on the host (tests/emul/contfit_emul.cpp, also
// under ASan / UBSan).  Every array is the caller's (LDS or global memory in the kernel); the emulator fills its workspace with NaN
// before every star, as LDS holds whatever the workgroup before left there.
//   counting a pixel counts if it is inside n and w != 0; any other pixel is replaced by zeros by a select, whatever it holds.
//   rows     R [P + 1][n] in fp64: R_j = m T_j(x) (one rounded product) for j < P, R_P = f, T_j from cheb_series.hpp.
//            G = R diag(w_kept) R^T is normal_tile.hpp's tile: its pixel groups, wave stripes, operand pair and wave-order sum.
//   solve    solve_star: normal_tile.hpp's scaled_solve on G (unit diagonal), and
//            chi^2 = e^T G e with e = (c, -1), i.e. G[P][P] - 2 c.b + c^T A c, summed row by row in fp64.  (Not a second pass over
//            the residuals: without clipping the kernel reads every pixel once.  The form is second-order in c's error; what it
//            loses is the sums' rounding, n 2^-52 sum_ij |e_i e_j| sum_p |R_i R_j| w.)
//   clipping keeps: z = sqrt(w) fma(-m, p(x), f) over every counting pixel, kept iff -kappa_lo s <= z <= kappa_hi s, s = clip_scale.
//   outputs  out_pixel: f / p rounded to fp32 and (w p) p; zero where p <= 0 or is not finite.
//   order    fit_star_host below is the kernel's sequence of passes, statement by statement.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

#include "../../include/payne_hip.h"
#include "cheb_series.hpp"
#include "normal_tile.hpp"

namespace payne {
namespace contfit {

namespace nt = payne::ntile;

constexpr int kMaxP = PAYNE_CONTFIT_MAX_P;
constexpr int kMaxClip = PAYNE_CONTFIT_MAX_NCLIP;
constexpr int kMaxN = PAYNE_CONTFIT_MAX_N;            // the clipping mask is a bit set in LDS
constexpr int kWorkDoubles = kMaxP * kMaxP + 2 * kMaxP;   // solve_star's workspace: the scaled matrix, S, u
constexpr int kChunk = 4;                             // pixels a thread takes at a time in the residual and output passes

PAYNE_HD bool opts_ok(const payne_contfit_opts& o) {
  return o.P >= 1 && o.P <= kMaxP && o.nclip >= 0 && o.nclip <= kMaxClip && o.kappa_lo > 0.0 && o.kappa_hi > 0.0;
}
PAYNE_HD int mask_words(int n) { return (n + 31) / 32; }
PAYNE_HD bool finite_f(float v) { return nt::finite((double)v); }
PAYNE_HD bool failed(int status) { return status != PAYNE_CONTFIT_OK && status != PAYNE_CONTFIT_NONPOSITIVE; }

// The Chebyshev series (cheb_series.hpp) under this namespace, as the kernel and the emulator name it.
using chebs::cheb;
using chebs::cheb4;
using chebs::poly_value;
using chebs::poly4;

// Row i of R at one pixel.
PAYNE_HD double row_value(int i, int P, float m, float f, double x) { return i < P ? (double)m * cheb(i, x) : (double)f; }
// The same from T = T_i(x) (cheb4).
PAYNE_HD double row_from(int i, int P, float m, float f, double T) { return i < P ? (double)m * T : (double)f; }

// What the first sums pass checks of a counting pixel.
PAYNE_HD bool pixel_finite(float f, float m, double w) { return finite_f(f) && finite_f(m) && nt::finite(w); }

// The tile of one star on the host in the kernel's pixel order; mask == NULL: every counting pixel is kept.  *count = the counting
// pixels, *bad = one of them is not finite.
inline void tile_sums_host(const float* flux, const double* w, const float* model, const double* x, int n, int P, const unsigned* mask,
                           double* G, int* count, bool* bad) {
  int cnt = 0;
  bool nan = false;
  nt::tile_sums_host(w, n, P + 1, [&](int p, double* r) {
    ++cnt;
    nan = nan || !pixel_finite(flux[p], model[p], w[p]);
    if (mask && !((mask[p >> 5] >> (p & 31)) & 1u)) return false;
    for (int i = 0; i <= P; ++i) r[i] = row_value(i, P, model[p], flux[p], x[p]);
    return true;
  }, G);
  *count = cnt;
  *bad = nan;
}

// The coefficients behind the tile G [16][16] of `kept` pixels: c [P], *chisq.  work holds kWorkDoubles.  Returns the status:
// NAN (the first pass met a value that is not finite), TOO_FEW, SINGULAR or OK; c and *chisq are written only with OK.
PAYNE_HD int solve_star(const double* G, int P, int kept, bool bad, double* work, double* c, double* chisq) {
  if (bad) return PAYNE_CONTFIT_NAN;
  if (kept < P) return PAYNE_CONTFIT_TOO_FEW;
  if (!nt::scaled_solve(G, nt::kTile, G + P, nt::kTile, 1.0, P, work)) return PAYNE_CONTFIT_SINGULAR;
  const double* u = work + P * P + P;
  double total = 0.0;                                               // e^T G e, e = (c, -1); the upper triangle, mirrored
  for (int i = 0; i <= P; ++i) {
    const double ei = i < P ? u[i] : -1.0;
    double row = 0.5 * ei * G[i * nt::kTile + i];
    for (int j = i + 1; j <= P; ++j) row += (j < P ? u[j] : -1.0) * G[i * nt::kTile + j];
    total += 2.0 * ei * row;
  }
  if (!nt::finite(total)) return PAYNE_CONTFIT_SINGULAR;
  for (int k = 0; k < P; ++k) c[k] = u[k];
  *chisq = total;
  return PAYNE_CONTFIT_OK;
}

// The clipping scale s.
PAYNE_HD double clip_scale(double chisq, int kept, int P, int rescale) {
  if (!rescale) return 1.0;
  const int dof = kept - P > 1 ? kept - P : 1;
  return sqrt((chisq > 0.0 ? chisq : 0.0) / (double)dof);
}

// Is a counting pixel kept?  pv = p(x) there; lo = kappa_lo s, hi = kappa_hi s.
PAYNE_HD bool keeps(float f, float m, double w, double pv, double lo, double hi) {
  const double z = sqrt(w) * fma(-(double)m, pv, (double)f);
  return z >= -lo && z <= hi;
}

// One pixel of the output rows.  True: a counting pixel whose polynomial is not positive (or not finite).
PAYNE_HD bool out_pixel(float f, double w, double pv, bool counts, bool dropped, float* fo, double* wo) {
  const bool ok = pv > 0.0 && nt::finite(pv);
  *fo = ok ? (float)((double)f / pv) : 0.0f;
  *wo = ok && counts && !dropped ? (w * pv) * pv : 0.0;
  return counts && !ok;
}

// What the host walk leaves for the tests: per solve the tile [16][16] and the kept pixels [n].
struct HostTrace {
  std::vector<double> G;
  std::vector<unsigned char> kept;
};

// One star on the host, pass by pass as payne_contfit_kernel takes them.  model == NULL: the star's model index is out of range.
// G [256], work [kWorkDoubles], coef_lds [kMaxP] and mask [mask_words(n)] are the workspace (LDS in the kernel).  coef [P], chisq,
// npix, status, rounds: the star's results; flux_out / w_out [n] or NULL.
inline void fit_star_host(const float* flux, const double* w, const float* model, const double* x, int n, const payne_contfit_opts& o,
                          double* G, double* work, double* coef_lds, unsigned* mask, double* coef, double* chisq, int* npix, int* status,
                          int* rounds, float* flux_out, double* w_out, HostTrace* trace) {
  const int P = o.P;
  int st = model ? PAYNE_CONTFIT_OK : PAYNE_CONTFIT_BAD_MODEL, solves = 0, kept = 0;
  double chi = 0.0;
  bool masked = false;
  const int chunks = (n + kChunk - 1) / kChunk;
  if (model) {
    for (int round = 0;; ++round) {
      int cnt = 0;
      bool bad = false;
      tile_sums_host(flux, w, model, x, n, P, round > 0 ? mask : nullptr, G, &cnt, &bad);
      if (round == 0) kept = cnt;
      st = solve_star(G, P, kept, round == 0 && bad, work, coef_lds, &chi);
      if (st != PAYNE_CONTFIT_OK) break;
      ++solves;
      if (trace) {
        trace->G.insert(trace->G.end(), G, G + nt::kTileSize);
        for (int p = 0; p < n; ++p) trace->kept.push_back(w[p] != 0.0 && (!masked || ((mask[p >> 5] >> (p & 31)) & 1u)) ? 1 : 0);
      }
      if (round == o.nclip) break;
      const double s = clip_scale(chi, kept, P, o.rescale), lo = o.kappa_lo * s, hi = o.kappa_hi * s;
      int now = 0, changed = 0;
      for (int c = 0; c < chunks; c += 8) {                          // eight threads' chunks are one word
        unsigned word = 0u, old = 0u;
        for (int p = kChunk * c; p < kChunk * c + 32 && p < n; ++p) {
          const bool counts = w[p] != 0.0;
          const bool keep = counts && keeps(flux[p], model[p], w[p], poly_value(coef_lds, P, x[p]), lo, hi);
          word |= (keep ? 1u : 0u) << (p & 31);
          old |= (counts ? 1u : 0u) << (p & 31);
          now += keep ? 1 : 0;
        }
        if (masked) old = mask[c >> 3];
        for (int k = 0; k < 8; ++k) changed += ((old >> (4 * k)) & 15u) != ((word >> (4 * k)) & 15u) ? 1 : 0;
        mask[c >> 3] = word;
      }
      masked = true;
      if (!changed) break;
      kept = now;
    }
  }
  const bool fail = failed(st);
  bool nonpos = false;
  for (int p = 0; p < n; ++p) {
    float fo = flux[p];
    double wo = 0.0;
    if (!fail) {
      const bool counts = w[p] != 0.0;
      const bool dropped = o.drop_clipped && masked && !((mask[p >> 5] >> (p & 31)) & 1u);
      nonpos = out_pixel(flux[p], w[p], poly_value(coef_lds, P, x[p]), counts, dropped, &fo, &wo) || nonpos;
    }
    if (flux_out) flux_out[p] = fo;
    if (w_out) w_out[p] = wo;
  }
  if (!fail && nonpos) st = PAYNE_CONTFIT_NONPOSITIVE;
  for (int k = 0; k < P; ++k) coef[k] = fail ? (double)NAN : coef_lds[k];
  *chisq = fail ? (double)NAN : chi;
  *npix = kept;
  *status = st;
  *rounds = solves;
}

}  // namespace contfit
}  // namespace payne
