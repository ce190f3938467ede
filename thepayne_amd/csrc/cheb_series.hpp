// cheb_series.hpp -- Chebyshev series on one recurrence, written once: payne_contfit_batch's rows m T_j(x) and polynomial
// (contfit_core.hpp) and payne_lmfit_update_poly's rows (lmfit_core.hpp).  Plain C++, host / device.
//   T_0 = 1, T_1 = x, T_k = fma(2 x, T_k-1, -T_k-2); p(x) = sum_j c_j T_j(x), j ascending, one fma a term.
//   A series is named by (c, j): j < 0 is the series of the coefficients c; j >= 0 is T_j, the series of the unit vector e_j --
//   fma(1, T_j, 0) = T_j and fma(0, T_k, s) = s are exact while every T_k is finite, which |x| <= 1 ensures.  So lanes that want p
//   and lanes that want T_j run one loop of P - 2 steps, and the values are poly_value's and cheb's.
#pragma once
#include <math.h>

#include "normal_tile.hpp"

namespace payne {
namespace chebs {

PAYNE_HD double cheb_next(double x, double t1, double t0) { return fma(2.0 * x, t1, -t0); }

// T_i(x).
PAYNE_HD double cheb(int i, double x) {
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
// differ only in the step they keep.  (Four calls of cheb are four loops whose length differs from lane to lane; measured, NOTES.md.
// Kept beside series4 with j = i: it keeps a step by a select where series4 multiplies by zero or one.)
PAYNE_HD void cheb4(int i, int P, const double* x, double* T) {
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

PAYNE_HD double series_coef(const double* c, int j, int k) { return j < 0 ? c[k] : (k == j ? 1.0 : 0.0); }

// The series (c, j) of P terms at one abscissa.
PAYNE_HD double series_value(const double* c, int j, int P, double x) {
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

// series_value at four abscissae, the same values: each coefficient is read once for the four.
PAYNE_HD void series4(const double* c, int j, int P, const double* x, double* sv) {
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

// p(x) = sum_j c_j T_j(x), at one abscissa and at four.
PAYNE_HD double poly_value(const double* c, int P, double x) { return series_value(c, -1, P, x); }
PAYNE_HD void poly4(const double* c, int P, const double* x, double* pv) { series4(c, -1, P, x, pv); }

}  // namespace chebs
}  // namespace payne
