// tmatch_poly_core.hpp -- arithmetic of payne_tmatch_match_poly (k_tmatch_poly.hip): the template search of tmatch_core.hpp with a
// Chebyshev series of P <= 8 coefficients minimised out per (star, template) pair,
//     chi^2[s][t] = min_c sum_p w_sp (f_sp - m_tp sum_j c_j T_j(x_p))^2,
// the chi^2 that payne_contfit_batch and payne_lmfit_update_poly minimise, in their basis (cheb_series.hpp) and abscissa.  Plain C++,
// host / device: the same source runs in the kernels and on the host (tests/emul/tmatch_poly_emul.cpp, also under ASan / UBSan).
// Nothing here indexes a private array: every array is the caller's (LDS or global memory in the kernels), so the kernels have no
// scratch.  The pixel steps, the groups of four, the staging maps, c0 and the top-k lists are tmatch_core.hpp's.
//   sums     per pair, over the star's counting pixels (inside n, w != 0):  c0 = sum (w f) f  (tmatch_core.hpp's, unchanged),
//            b_j = sum (w f T_j(x)) m for j < P,  S_q = sum (w T_q(x)) m^2 for q <= 2 P - 2: 3 P - 1 matrix products N x M over n.
//            THE BASIS FACTORS ARE ON THE STAR SIDE: the star's operands are a1 T_j and a2 T_q (a1 = w f, a2 = w, each product rounded
//            once; zero by a select where the pixel does not count, whatever flux, w and x hold there), the template's are m and
//            m^2 (widened first, so both are exact; zero by a select where the value is not finite or beyond n).  A workgroup forms
//            its 16 stars' operands once a step and its 64 templates share them.
//   order    operand `op` (b_j: op = j; S_q: op = P + q) has its own accumulator, which starts at +0; group g of a step hands pixels
//            32 step + 4 g + k, k = 0..3, to one matrix instruction an operand, a chain of four fused multiply-adds.
//   solve    A_jk = (S_{j+k} + S_{|j-k|}) / 2 (T_j T_k = (T_{j+k} + T_{|j-k|}) / 2; the halving is exact), A c = b by
//            normal_tile.hpp's scaled_solve with a unit diagonal.  The lower triangle is formed inside scaled_solve's own matrix
//            area, which it scales in place (it reads an element before it writes the same one).
//            chi^2 = c0 + sum_j c_j (sum_k A_jk c_k - 2 b_j), j and k ascending, one fma a term: second order in the error of c,
//            so no condition number enters the error bound.  P = 1 is the free amplitude: c0 - b_0^2 / S_0 in this form.
//   NaN      a pair is NaN (chi^2 and coefficients) when a template value is not finite at a counting pixel (tmatch_core.hpp's
//            pair_poisoned), when the star has fewer than P counting pixels (an integer count), when scaled_solve refuses (a
//            template that is zero at every counting pixel, sums that are not finite), or when c0 is NaN.  A NaN in the flux or
//            in w at a counting pixel reaches every sum.  NaN is never listed, so a star without counting pixels lists nothing
//            (idx -1, chi^2 +inf) -- UNLIKE payne_tmatch_match, which lists chi^2 = 0 for it.
//   lists    tmatch_core.hpp's, per chunk of kChunk = 64 templates and merged in chunk order; every entry carries its P
//            coefficients, and the merge remembers where each entry came from.  A listed template whose polynomial is not positive
//            at some counting pixel stays listed; bit 0 of its flags says whether p(x_p) > 0 at all of them (poly_value).
//   kernels  ONE INSTANTIATION PER P (1 .. 8): the 3 P - 1 accumulators are statically indexed registers.
#pragma once
#include <math.h>
#include <stddef.h>

#include "cheb_series.hpp"
#include "normal_tile.hpp"
#include "tmatch_core.hpp"

namespace payne {
namespace tmatch_poly {

namespace tq = payne::tmatch;

constexpr int kMaxPoly = PAYNE_TMATCH_MAX_POLY;
constexpr int kStars = 16;                          // stars of a workgroup's tile
constexpr int kChunk = 64;                          // templates of a workgroup's tile = of one partial top-k list: 16 a wave
constexpr int kStarRegs = kStars * tq::kStep / tq::kThreads;      // 2: star pixels a thread stages per step
constexpr int kTemplRegs = kChunk * tq::kStep / tq::kThreads;     // 8: template values a thread stages per step
constexpr int kPitchChi = kChunk + 1;
constexpr int kMergeStars = 32;                     // stars of one workgroup of the merge launch

constexpr int ops_of(int P) { return 3 * P - 1; }
constexpr int work_doubles(int P) { return P * P + 2 * P; }                     // scaled_solve's
constexpr int area_doubles(int P) { return ops_of(P) + work_doubles(P); }       // a pair's sums, then the solve's work; odd for every P
// pairs solved at a time by a workgroup (of its 256 threads): what keeps the areas beside the coefficient tile inside the LDS
constexpr int solvers_of(int P) { return P <= 2 ? 256 : (P <= 6 ? 128 : 64); }

PAYNE_TMATCH_HD int tiles_of(int N) { return (N + kStars - 1) / kStars; }
PAYNE_TMATCH_HD int chunks_of(int M) { return (M + kChunk - 1) / kChunk; }
// accumulators: register reg of wave v, lane `lane`
PAYNE_TMATCH_HD int acc_star(int reg, int lane) { return 4 * reg + (lane >> 4); }
PAYNE_TMATCH_HD int acc_template(int wave, int lane) { return 16 * wave + (lane & 15); }

// The star's 3 P - 1 operands at one pixel from star_operands' a1, a2: ops[op * stride].  x is read only where the pixel counts.
PAYNE_TMATCH_HD void star_basis(double a1, double a2, bool counts, double x, int P, double* ops, int stride) {
  double t0 = 1.0, t1 = x;
  for (int q = 0; q <= 2 * P - 2; ++q) {
    double T = q == 0 ? 1.0 : x;
    if (q >= 2) {
      T = chebs::cheb_next(x, t1, t0);
      t0 = t1;
      t1 = T;
    }
    if (q < P) ops[q * stride] = counts ? a1 * T : 0.0;
    ops[(P + q) * stride] = counts ? a2 * T : 0.0;
  }
}
PAYNE_TMATCH_HD bool pixel_counts(double w, bool inside) { return inside && w != 0.0; }

PAYNE_TMATCH_HD void template_operands(float m, double* b1, double* b2) {
  const double md = tq::finite32(m) ? (double)m : 0.0;
  *b1 = md;
  *b2 = md * md;
}

// One pair behind its sums: sums[op * ld] (b_j at j, S_q at P + q), the star's c0 and count of counting pixels, `poisoned` from
// pair_poisoned.  work holds work_doubles(P).  Writes c[j * ldc], j < P, and returns chi^2; all NaN by the rules above.
PAYNE_TMATCH_HD double pair_solve(const double* sums, int ld, int P, double c0, int count, bool poisoned, double* work, double* c, int ldc) {
  const double* b = sums;
  const double* S = sums + (size_t)P * ld;
  bool ok = !poisoned && count >= P;
  if (ok) {
    for (int i = 0; i < P; ++i)
      for (int j = 0; j <= i; ++j) work[i * P + j] = 0.5 * (S[(i + j) * ld] + S[(i - j) * ld]);
    ok = ntile::scaled_solve(work, P, b, ld, 1.0, P, work);
  }
  if (!ok) {
    for (int j = 0; j < P; ++j) c[j * ldc] = (double)NAN;
    return (double)NAN;
  }
  const double* u = work + P * P + P;
  double q = 0.0;
  for (int j = 0; j < P; ++j) {
    double row = 0.0;
    for (int k = 0; k < P; ++k) row = fma(0.5 * (S[(j + k) * ld] + S[(j > k ? j - k : k - j) * ld]), u[k], row);
    q = fma(u[j], fma(-2.0, b[j * ld], row), q);
    c[j * ldc] = u[j];
  }
  const double chi = c0 + q;
  if (chi != chi)
    for (int j = 0; j < P; ++j) c[j * ldc] = (double)NAN;
  return chi;
}

// ---- lists that remember where an entry came from ----------------------------------------------------------------------------------
PAYNE_TMATCH_HD void list_insert_from(double* c, int* idx, int* src, int k, double v, int t, int from) {
  if (v != v) return;
  if (idx[k - 1] >= 0 && !(v < c[k - 1])) return;
  int pos = k - 1;
  while (pos > 0 && (idx[pos - 1] < 0 || v < c[pos - 1])) {
    c[pos] = c[pos - 1];
    idx[pos] = idx[pos - 1];
    src[pos] = src[pos - 1];
    --pos;
  }
  c[pos] = v;
  idx[pos] = t;
  src[pos] = from;
}
// tmatch_core.hpp's merge_chunks; src[j] = ch * k + i names entry i of chunk ch's list (-1: an empty slot).
PAYNE_TMATCH_HD void merge_chunks_from(double* c, int* idx, int* src, int k, const double* part_c, const int* part_i, int chunks, int N, int s) {
  tq::list_clear(c, idx, k);
  for (int j = 0; j < k; ++j) src[j] = -1;
  for (int ch = 0; ch < chunks; ++ch) {
    const size_t at = tq::part_at(ch, N, s, k);
    for (int j = 0; j < k && part_i[at + j] >= 0; ++j) list_insert_from(c, idx, src, k, part_c[at + j], part_i[at + j], ch * k + j);
  }
}
PAYNE_TMATCH_HD size_t src_at(int src, int N, int s, int k) { return tq::part_at(src / k, N, s, k) + (size_t)(src % k); }

// Bit 0: p(x_p) > 0 at every counting pixel of the star.
PAYNE_TMATCH_HD int positive_flag(const double* c, int P, const double* w, const double* x, int n) {
  for (int p = 0; p < n; ++p)
    if (w[p] != 0.0 && !(chebs::poly_value(c, P, x[p]) > 0.0)) return 0;
  return 1;
}
// One entry of the merged list: its coefficients from the chunk lists' (NaN for an empty slot) and its flags.
PAYNE_TMATCH_HD int finish_entry(int src, const double* part_coef, int N, int s, int k, int P, const double* w, const double* x, int n, double* coef) {
  if (src < 0) {
    for (int j = 0; j < P; ++j) coef[j] = (double)NAN;
    return 0;
  }
  const double* from = part_coef + src_at(src, N, s, k) * (size_t)P;
  for (int j = 0; j < P; ++j) coef[j] = from[j];
  return positive_flag(coef, P, w, x, n);
}

// ---- one star's row on the host in the kernel's own order ---------------------------------------------------------------------------
// row [M], coef [M][P]; work holds (ops_of(P) + 1) * steps_of(n) * kStep + area_doubles(P) doubles.
inline void row_host(const float* templates, long long ld_t, int M, const float* flux, const double* w, const double* x, int n, int P, double* row,
                     double* coef, double* work) {
  const int steps = tq::steps_of(n), np = steps * tq::kStep, nops = ops_of(P);
  double* ops = work;                                               // [nops][np]
  double* a2s = work + (size_t)nops * np;                           // the staged weight operand, for pair_poisoned
  double* area = a2s + np;
  int count = 0;
  double part[tq::kStep];
  for (int j = 0; j < tq::kStep; ++j) part[j] = 0.0;
  for (int p = 0; p < np; ++p) {
    double a1, a2, fz;
    const bool inside = p < n;
    tq::star_operands(inside ? flux[p] : 0.0f, inside ? w[p] : 0.0, inside, &a1, &a2, &fz);
    const bool counts = pixel_counts(inside ? w[p] : 0.0, inside);
    count += counts ? 1 : 0;
    star_basis(a1, a2, counts, counts ? x[p] : 0.0, P, ops + p, np);
    part[p % tq::kStep] = tq::c0_add(a1, fz, part[p % tq::kStep]);   // (steps in order within one partial sum)
    a2s[p] = a2;
  }
  double c0 = 0.0;
  for (int j = 0; j < tq::kStep; ++j) c0 += part[j];
  for (int t = 0; t < M; ++t) {
    const float* m = templates + (size_t)t * (size_t)ld_t;
    for (int op = 0; op < nops; ++op) area[op] = 0.0;
    bool poisoned = false;
    for (int st = 0; st < steps; ++st)
      for (int g = 0; g < tq::groups_in_step(n, st); ++g) {
        double b1[tq::kGroup], b2[tq::kGroup];
        for (int k = 0; k < tq::kGroup; ++k) {
          const int p = tq::pixel_of(st, g, k);
          const float mv = p < n ? m[p] : 0.0f;
          template_operands(mv, &b1[k], &b2[k]);
          poisoned = poisoned || tq::pair_poisoned(a2s[p], mv);
        }
        for (int op = 0; op < nops; ++op)
          for (int k = 0; k < tq::kGroup; ++k) area[op] = fma(ops[(size_t)op * np + tq::pixel_of(st, g, k)], op < P ? b1[k] : b2[k], area[op]);
      }
    row[t] = pair_solve(area, 1, P, c0, count, poisoned, area + nops, coef + (size_t)t * P, 1);
  }
}

// The call on the host, as the two launches do.  all may be NULL.  part_c / part_i hold chunks_of(M) * N * topk entries, part_coef P
// times as many; work as row_host's plus M * (P + 1) doubles (the row and its coefficients).
inline void match_poly_host(const float* templates, long long ld_t, int M, const float* flux, const double* w, long long ld_f, int N, int n,
                            const double* x, int P, int topk, int* idx, double* chisq, double* coef, int* flags, double* all, long long ld_a,
                            double* part_c, int* part_i, double* part_coef, double* work) {
  const int chunks = chunks_of(M);
  double* row = work + (size_t)(ops_of(P) + 1) * tq::steps_of(n) * tq::kStep + area_doubles(P);
  double* rcoef = row + M;
  for (int s = 0; s < N; ++s) {
    row_host(templates, ld_t, M, flux + (size_t)s * (size_t)ld_f, w + (size_t)s * (size_t)ld_f, x, n, P, row, rcoef, work);
    for (int ch = 0; ch < chunks; ++ch) {
      const int t0 = ch * kChunk, count = M - t0 < kChunk ? M - t0 : kChunk;
      const size_t at = tq::part_at(ch, N, s, topk);
      tq::list_from_chunk(part_c + at, part_i + at, topk, row + t0, t0, count);
      for (int j = 0; j < topk && part_i[at + j] >= 0; ++j)
        for (int q = 0; q < P; ++q) part_coef[(at + j) * P + q] = rcoef[(size_t)part_i[at + j] * P + q];
    }
    if (all)
      for (int t = 0; t < M; ++t) all[(size_t)s * (size_t)ld_a + t] = row[t];
  }
  int src[tq::kMaxTopk];
  for (int s = 0; s < N; ++s) {
    merge_chunks_from(chisq + (size_t)s * topk, idx + (size_t)s * topk, src, topk, part_c, part_i, chunks, N, s);
    for (int j = 0; j < topk; ++j)
      flags[(size_t)s * topk + j] = finish_entry(src[j], part_coef, N, s, topk, P, w + (size_t)s * (size_t)ld_f, x, n, coef + ((size_t)s * topk + j) * P);
  }
}

}  // namespace tmatch_poly
}  // namespace payne
