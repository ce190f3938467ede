// lmfit_pair_core.hpp -- arithmetic of payne_lmfit_update_pair (k_lmfit.hip): the rows of one star's normal equations for a spectrum
// that is the sum of two components A and B with a light ratio q, times a Chebyshev series.  Plain C++, host / device: the same
// source runs in the kernel and on the host (tests/emul/lmfit_pair_emul.cpp, also under ASan / UBSan).  Nothing here indexes a private
// array.
//   model       p(x) [(1 - q) m_A + q m_B]: m_A, m_B the components' models (row 0 of the caller's two row blocks), p = sum_j c_j T_j(x)
//               (cheb_series.hpp), p == 1 with P == 0.
//   parameters  K = Kl + 1 + P: Kl that the components see, then q, then the P coefficients.  Parameter k < Kl is derivative row
//               ia[k] of A's block and row ib[k] of B's, -1 for "this component does not see it" (PairMap).  At least one is >= 0; both
//               are for a parameter the components share.
//   rows        at one pixel, in fp64, from the fp32 values a (A's block) and b (B's block), omq = 1 - q rounded once a star:
//                 mix = fma(cb, (double)b, ca * (double)a)              one rounded product, one fma
//                 R_i = mix * s for i < K,  R_K = fma(-mix, s, (double)f)   one rounded product; one fma
//               with, for row i,
//                 i < Kl        a = A's row 1 + ia[i], b = B's row 1 + ib[i] (0.0f where the index is -1: nothing is read),
//                               (ca, cb) = (omq, q), s = p                  p [(1 - q) dm_A + q dm_B]
//                 i == Kl       a = m_A, b = m_B, (ca, cb) = (-1, 1), s = p   p (m_B - m_A): the difference is exact in the fma
//                 Kl < i < K    a = m_A, b = m_B, (ca, cb) = (omq, q), s = T_{i - Kl - 1}(x)
//                 i == K        a = m_A, b = m_B, (ca, cb) = (omq, q), s = p   f - p [(1 - q) m_A + q m_B]
//               s is series_value(c, j, P, x) of cheb_series.hpp (j = -1: p), and exactly 1.0 with P == 0 (c and x are not read), so that
//               the product and the fma by s change nothing there.
#pragma once
#include "lmfit_core.hpp"

namespace payne {
namespace lmfit {

struct PairMap {
  int ia[kMaxK], ib[kMaxK];
};

// What payne_lmfit_update_pair checks of the values the host holds, in the header's order.  K is the handle's.
PAYNE_HD int check_pair_counts(int K, int Kl, int P, int Ka, int Kb) {
  return Kl < 0 || P < 0 || Kl + 1 + P != K || Ka < 0 || Kb < 0 ? PAYNE_E_INVALID : PAYNE_OK;
}
PAYNE_HD int check_pair(int K, int Kl, int P, int Ka, int Kb, const int* ia, const int* ib) {
  if (check_pair_counts(K, Kl, P, Ka, Kb) != PAYNE_OK) return PAYNE_E_INVALID;
  if (Kl > 0 && (!ia || !ib)) return PAYNE_E_INVALID;
  for (int k = 0; k < Kl; ++k) {
    if (ia[k] < -1 || ia[k] >= Ka || ib[k] < -1 || ib[k] >= Kb) return PAYNE_E_INVALID;
    if (ia[k] < 0 && ib[k] < 0) return PAYNE_E_INVALID;             // nothing would see the parameter
  }
  return PAYNE_OK;
}

// The map as the kernel takes it; the entries from Kl on are -1.
PAYNE_HD PairMap pair_map(int Kl, const int* ia, const int* ib) {
  PairMap m;
  for (int k = 0; k < kMaxK; ++k) {
    m.ia[k] = k < Kl ? ia[k] : -1;
    m.ib[k] = k < Kl ? ib[k] : -1;
  }
  return m;
}

// The row of a component's block that row i of R reads: 1 + its derivative, 0 (the model) from Kl on, -1 for none.
PAYNE_HD int pair_row_of(int i, int Kl, const int* idx) { return i < Kl ? (idx[i] >= 0 ? 1 + idx[i] : -1) : 0; }

// j of the lane's series: T_j for a coefficient's row, -1 (p) elsewhere.
PAYNE_HD int pair_series_index(int i, int Kl, int K) { return i > Kl && i < K ? i - Kl - 1 : -1; }

// The weights (ca, cb) of row i.
PAYNE_HD void pair_weights(int i, int Kl, double omq, double q, double* ca, double* cb) {
  *ca = i == Kl ? -1.0 : omq;
  *cb = i == Kl ? 1.0 : q;
}

// Row i of R at one pixel.
PAYNE_HD double operand_pair_mix(int i, int K, double ca, double cb, float a, float b, float f, double s) {
  const double mix = fma(cb, (double)b, ca * (double)a);
  return i < K ? mix * s : fma(-mix, s, (double)f);
}

// The tile on the host in the kernel's pixel order: G [16][16] of one star.  rows_a [1 + Ka][ld], rows_b [1 + Kb][ld]; q the star's
// trial ratio, c [P] its coefficients, x [n] (c and x are not read with P == 0).
inline void tile_sums_pair_host(const float* rows_a, const float* rows_b, long long ld, const float* flux, const double* w, const double* x,
                                int n, int Kl, int P, const PairMap& map, double q, const double* c, double* G) {
  const int K = Kl + 1 + P;
  const double omq = 1.0 - q;
  nt::tile_sums_host(w, n, K + 1, [&](int p, double* r) {
    for (int i = 0; i <= K; ++i) {
      const int ra = pair_row_of(i, Kl, map.ia), rb = pair_row_of(i, Kl, map.ib);
      const float a = ra >= 0 ? rows_a[(size_t)ra * (size_t)ld + (size_t)p] : 0.0f;
      const float b = rb >= 0 ? rows_b[(size_t)rb * (size_t)ld + (size_t)p] : 0.0f;
      double ca, cb;
      pair_weights(i, Kl, omq, q, &ca, &cb);
      const double s = P > 0 ? chebs::series_value(c, pair_series_index(i, Kl, K), P, x[p]) : 1.0;
      r[i] = operand_pair_mix(i, K, ca, cb, a, b, flux[p], s);
    }
    return true;
  }, G);
}

}  // namespace lmfit
}  // namespace payne
