// lmfit_phot_core.hpp -- the photometric block of payne_lmfit_update_phot (k_lmfit.hip): what a star's magnitudes and Gaussian priors
// add to its spectral normal equations before the step is taken.  Plain C++, host / device: the same source runs in the kernel and on
// the host (tests/emul/lmfit_phot_emul.cpp, also under ASan / UBSan).  A header of its own because sedfit_core.hpp, whose tile_add and
// add_priors are called here and not restated, itself includes lmfit_core.hpp.  Nothing here indexes a private array.
//   parameters  K = Km + Kp + P: the spectral model's, those only the photometry sees, the Chebyshev coefficients (lmfit_core.hpp:
//               has_row).  sed_col[k]: the column of payne_sedfit_jac's dmags [F][ncol] that parameter k is, or -1 for none.
//   block       R_k = dmags[f][sed_col[k]] (0 where sed_col[k] == -1), R_K = obs_f - mag_f; element (i, j), i <= j <= K, of the block
//               is g = 0, then g = tile_add(g, R_i, R_j, pw_f) over the filters with pw_f != 0 in ascending order (phot_element): the
//               upper triangle, which is what update_star reads.  A filter with pw == 0 is not read past its weight.
//   priors      add_priors on that block at the star's x_trial; then tile[i][j] = tile[i][j] + g, one addition (add_block).
#pragma once
#include "sedfit_core.hpp"

namespace payne {
namespace lmfit {

constexpr int kPhotMaxF = 64;                     // filters of a star: the kernel stages them in LDS
constexpr int kPhotMaxCol = PAYNE_SEDFIT_MAX_K;   // columns of dmags: 7, or 6 for scaled rows

struct PhotMap {
  int ncol, Kp;
  int sed_col[kMaxK];
};

// What payne_lmfit_update_phot checks of the values the host holds, in the header's order.  K is the handle's.
PAYNE_HD int check_phot(int K, int Km, int Kp, int P, int F, int ncol, const int* sed_col, const Box& box, bool has_mu, bool has_sigma) {
  if (P < 0 || Kp < 0 || Km < 0 || Km + Kp + P != K) return PAYNE_E_INVALID;
  if (F < 0 || (ncol != 6 && ncol != 7) || !sed_col || has_mu != has_sigma) return PAYNE_E_INVALID;
  for (int k = 0; k < K; ++k) {
    const int c = sed_col[k];
    if (c < -1 || c >= ncol) return PAYNE_E_INVALID;
    if (k >= Km && k < Km + Kp && c < 0) return PAYNE_E_INVALID;    // nothing would see the parameter
    if (k >= Km + Kp && c != -1) return PAYNE_E_INVALID;            // a coefficient
    if (c == ncol - 1 && !(box.hi[k] < 5.0)) return PAYNE_E_INVALID;   // the model jumps at Av = 5
  }
  return F > kPhotMaxF ? PAYNE_E_UNSUPPORTED : PAYNE_OK;
}

PAYNE_HD double phot_residual(double obs, double mag) { return obs - mag; }

// Row k of the photometric R at one filter: dm [ncol] its derivatives, res its residual.
PAYNE_HD double phot_operand(const PhotMap& m, int k, int K, const double* dm, double res) {
  return k == K ? res : (m.sed_col[k] >= 0 ? dm[m.sed_col[k]] : 0.0);
}

// Element (i, j) of the block: dm [F][ncol], res, pw [F].
PAYNE_HD double phot_element(const PhotMap& m, int i, int j, int K, int F, const double* dm, const double* res, const double* pw) {
  double g = 0.0;
  for (int f = 0; f < F; ++f) {
    if (pw[f] == 0.0) continue;
    const double* d = dm + (size_t)f * (size_t)m.ncol;
    g = sedfit::tile_add(g, phot_operand(m, i, K, d, res[f]), phot_operand(m, j, K, d, res[f]), pw[f]);
  }
  return g;
}

// The priors on the block pt [16][16] at x, then the block into the tile: the upper triangle, column K included.
PAYNE_HD void add_block(double* tile, double* pt, int K, const double* x, const double* mu, const double* sigma) {
  sedfit::add_priors(pt, K, x, mu, sigma);
  for (int i = 0; i <= K; ++i)
    for (int j = i; j <= K; ++j) tile[i * kTile + j] = tile[i * kTile + j] + pt[i * kTile + j];
}

// One star's block on the host: mags, obs, pw [F], dmags [F][ncol]; pt [16][16] and res [F] are the caller's.
inline void phot_block_host(const PhotMap& m, int K, int F, const double* mags, const double* dmags, const double* obs, const double* pw,
                            double* res, double* pt) {
  for (int f = 0; f < F; ++f) res[f] = phot_residual(obs[f], mags[f]);
  for (int e = 0; e < kTileSize; ++e) pt[e] = 0.0;
  for (int i = 0; i <= K; ++i)
    for (int j = i; j <= K; ++j) pt[i * kTile + j] = phot_element(m, i, j, K, F, dmags, res, pw);
}

}  // namespace lmfit
}  // namespace payne
