// tmatch_pair_core.hpp -- arithmetic of payne_tmatch_match_pairs (k_tmatch_pair.hip): the template search of tmatch_core.hpp against PAIRS
// of templates with both amplitudes free,
//     chi^2[s][a][b] = min over (alpha, beta) of sum_p w_sp (f_sp - alpha m_ap - beta m_bp)^2,
// the starting points of payne_lmfit_update_pair's two-component fit: alpha + beta is its scale, beta / (alpha + beta) its light ratio.
// Plain C++, host / device: the same source runs in the kernels and on the host (tests/emul/tmatch_pair_emul.cpp, also under ASan /
// UBSan).  Nothing here indexes a private array: every array is the caller's (LDS or global memory in the kernels), so the kernels have
// no scratch.  The pixel steps, the groups of four, the staging maps, the operands' selects, c0 and the lists are tmatch_core.hpp's.
//   moments  per (star, template), over the star's counting pixels:  B[s][t] = sum a1 m_t,  S[s][t] = sum a2 m_t^2  (a1 = w f, a2 = w:
//            star_operands; m widened first, so m and m^2 are exact), and c0[s] = sum a1 f.  The plain search's tile with its two
//            products in accumulators of their own, each from +0: group g of a step hands pixels 32 step + 4 g + k, k = 0..3, to one
//            matrix instruction a moment, a chain of four fused multiply-adds.  A template value that is not finite at a counting
//            pixel of the star (pair_poisoned) makes both moments of that (star, template) NaN.
//   cross    X[s][a][b] = sum (a2 m_a) m_b.  The weight is the star's, so X belongs to a (star, primary): row r = s kA + j of the
//            call is star s with its primary a = cand[s][j], and carries the gathered operand g = a2[s] m_a (gathered_operand: one
//            rounding; zero where the pixel does not count, m_a is not finite, or cand lies outside 0 .. M - 1).  The columns are
//            the bank: one (N kA) x M matrix product over n, one matrix instruction per group where the plain search has two.
//   solve    D = fma(-X, X, Sa Sb);  alpha = (Ba Sb - Bb X) / D;  beta = (Bb Sa - Ba X) / D;
//            chi^2 = c0 + alpha (Sa alpha + X beta - 2 Ba) + beta (X alpha + Sb beta - 2 Bb)  (pair_solve states the order): the
//            quadratic form, second order in the error of (alpha, beta), so no condition number enters the error bound.
//   NaN      a pair is NaN (chi^2 and both amplitudes) and never listed when a == b; when cand[s][j] lies outside 0 .. M - 1; when
//            either template is not finite at a counting pixel of the star (through the moments); when Sa or Sb is not > 0; when
//            the pair is collinear, not (D > 2^-20 Sa Sb); when alpha or beta is not > 0 (one template with a scale fits as well:
//            payne_tmatch_match_poly with P = 1 covers that); when b is one of the star's primaries in an earlier slot j' < j
//            (that pair is (j', a): an unordered pair is listed once); when chi^2 itself is NaN (c0).
//   lists    ascending in (chi^2, slot j, b); an empty slot is idx = -1, chi^2 = +inf, amplitudes NaN.  A workgroup leaves the
//            list of each of its rows for its chunk of kChunk templates in the workspace, with the listed pairs' amplitudes;
//            merge_rows walks a star's rows in j order and each row's chunks in chunk order, so list_insert's candidates arrive in
//            ascending (j, b).  No atomics, one fixed order: the same inputs give the same bytes, and nothing in a star's arithmetic
//            depends on its place in the call or on the other stars.
#pragma once
#include <math.h>
#include <stddef.h>

#include "tmatch_core.hpp"
#include "tmatch_poly_core.hpp"

namespace payne {
namespace tmatch_pair {

namespace tq = payne::tmatch;
namespace tp = payne::tmatch_poly;

constexpr int kMaxPrimaries = PAYNE_TMATCH_MAX_PRIMARIES;
constexpr int kRows = tq::kStars;                   // rows (star, primary) of a workgroup's tile of the cross launch
constexpr int kChunk = tq::kChunk;                  // templates of a workgroup's tile = of one partial list
constexpr double kCollinear = 1.0 / 1048576.0;      // 2^-20: D / (Sa Sb) = 1 - cos^2 of the angle between the two templates

PAYNE_TMATCH_HD int row_tiles_of(int N, int kA) { return (N * kA + kRows - 1) / kRows; }
// row <-> (star, slot)
PAYNE_TMATCH_HD int row_of(int s, int j, int kA) { return s * kA + j; }
PAYNE_TMATCH_HD int row_star(int row, int kA) { return row / kA; }
PAYNE_TMATCH_HD int row_slot(int row, int kA) { return row % kA; }
// the moments' workspace: B then S, each [N][M] at the call's own M
PAYNE_TMATCH_HD size_t moment_at(int s, int M, int t) { return (size_t)s * (size_t)M + (size_t)t; }

PAYNE_TMATCH_HD bool cand_valid(int a, int M) { return a >= 0 && a < M; }
PAYNE_TMATCH_HD double template_value(float m) { return tq::finite32(m) ? (double)m : 0.0; }
// The row's operand at one pixel from star_operands' a2 and the primary's staged value (0 where cand is not valid).
PAYNE_TMATCH_HD double gathered_operand(double a2, float m) { return a2 * template_value(m); }
// b is one of the star's primaries in a slot before j
PAYNE_TMATCH_HD bool in_earlier_slot(const int* cand_star, int j, int b) {
  bool hit = false;
  for (int e = 0; e < j; ++e) hit = hit || cand_star[e] == b;
  return hit;
}

// One pair behind its sums.  `barred`: a == b, or b in an earlier slot.  An invalid primary arrives as Sa = NaN.  Writes both
// amplitudes and returns chi^2; all three NaN by the rules above.
PAYNE_TMATCH_HD double pair_solve(double Sa, double Ba, double Sb, double Bb, double X, double c0, bool barred, double* alpha, double* beta) {
  const double SS = Sa * Sb;
  const double D = fma(-X, X, SS);
  bool ok = !barred && Sa > 0.0 && Sb > 0.0 && D > kCollinear * SS;
  double al = (double)NAN, be = (double)NAN, chi = (double)NAN;
  if (ok) {
    al = fma(Ba, Sb, -(Bb * X)) / D;
    be = fma(Bb, Sa, -(Ba * X)) / D;
    ok = al > 0.0 && be > 0.0;
  }
  if (ok) {
    const double ra = fma(X, be, Sa * al), rb = fma(Sb, be, X * al);
    chi = c0 + fma(be, fma(-2.0, Bb, rb), al * fma(-2.0, Ba, ra));
    ok = chi == chi;
  }
  *alpha = ok ? al : (double)NAN;
  *beta = ok ? be : (double)NAN;
  return ok ? chi : (double)NAN;
}

// ---- the merge: a star's rows in j order, each row's chunks in chunk order ---------------------------------------------------------
// The workspace holds chunk ch's list of row r at tq::part_at(ch, R, r, k), R = N kA.  src[e] = (j * chunks + ch) * k + i names entry i
// of that list (-1: an empty slot).
PAYNE_TMATCH_HD void merge_rows(double* c, int* idx, int* src, int k, const double* part_c, const int* part_i, int chunks, int N, int kA, int s) {
  tq::list_clear(c, idx, k);
  for (int e = 0; e < k; ++e) src[e] = -1;
  for (int j = 0; j < kA; ++j)
    for (int ch = 0; ch < chunks; ++ch) {
      const size_t at = tq::part_at(ch, N * kA, row_of(s, j, kA), k);
      for (int e = 0; e < k && part_i[at + e] >= 0; ++e) tp::list_insert_from(c, idx, src, k, part_c[at + e], part_i[at + e], (j * chunks + ch) * k + e);
    }
}
// One entry of the merged list: the primary's template index (-1 for an empty slot) and the amplitudes from the chunk lists' (NaN).
PAYNE_TMATCH_HD int finish_entry(int src, const int* cand, const double* part_amp, int chunks, int N, int kA, int s, int k, double* amp) {
  if (src < 0) {
    amp[0] = amp[1] = (double)NAN;
    return -1;
  }
  const int j = src / (chunks * k), ch = (src / k) % chunks, e = src % k;
  const size_t at = tq::part_at(ch, N * kA, row_of(s, j, kA), k) + (size_t)e;
  amp[0] = part_amp[2 * at];
  amp[1] = part_amp[2 * at + 1];
  return cand[row_of(s, j, kA)];
}

// ---- one star on the host in the kernels' own order --------------------------------------------------------------------------------
// The star's operands a1, a2, fz [steps_of(n) * kStep] (zero beyond n) and c0, as tmatch_core.hpp's row_host forms them.
inline double star_host(const float* flux, const double* w, int n, double* a1, double* a2, double* fz) {
  const int steps = tq::steps_of(n), np = steps * tq::kStep;
  for (int p = 0; p < np; ++p) tq::star_operands(p < n ? flux[p] : 0.0f, p < n ? w[p] : 0.0, p < n, &a1[p], &a2[p], &fz[p]);
  double c0 = 0.0;
  for (int j = 0; j < tq::kStep; ++j) {
    double part = 0.0;
    for (int st = 0; st < steps; ++st) part = tq::c0_add(a1[st * tq::kStep + j], fz[st * tq::kStep + j], part);
    c0 += part;
  }
  return c0;
}
// B [M], S [M] of one star
inline void moments_host(const float* templates, long long ld_t, int M, const double* a1, const double* a2, int n, double* B, double* S) {
  const int steps = tq::steps_of(n);
  for (int t = 0; t < M; ++t) {
    const float* m = templates + (size_t)t * (size_t)ld_t;
    double accB = 0.0, accS = 0.0;
    bool poisoned = false;
    for (int st = 0; st < steps; ++st)
      for (int g = 0; g < tq::groups_in_step(n, st); ++g) {
        for (int k = 0; k < tq::kGroup; ++k) {
          const int p = tq::pixel_of(st, g, k);
          const float mv = p < n ? m[p] : 0.0f;
          const double md = template_value(mv);
          poisoned = poisoned || tq::pair_poisoned(a2[p], mv);
          accB = fma(a1[p], md, accB);
          accS = fma(a2[p], md * md, accS);
        }
      }
    B[t] = poisoned ? (double)NAN : accB;
    S[t] = poisoned ? (double)NAN : accS;
  }
}
// One row (star, slot j): chi [M], al [M], be [M].  g holds steps_of(n) * kStep doubles.
inline void row_host(const float* templates, long long ld_t, int M, const double* a2, int n, const int* cand_star, int j, const double* B,
                     const double* S, double c0, double* g, double* chi, double* al, double* be) {
  const int steps = tq::steps_of(n), np = steps * tq::kStep;
  const int a = cand_star[j];
  const bool valid = cand_valid(a, M);
  const float* ma = templates + (size_t)(valid ? a : 0) * (size_t)ld_t;
  for (int p = 0; p < np; ++p) g[p] = gathered_operand(a2[p], (valid && p < n) ? ma[p] : 0.0f);
  const double Sa = valid ? S[a] : (double)NAN, Ba = valid ? B[a] : (double)NAN;
  for (int b = 0; b < M; ++b) {
    const float* m = templates + (size_t)b * (size_t)ld_t;
    double X = 0.0;
    for (int st = 0; st < steps; ++st)
      for (int gr = 0; gr < tq::groups_in_step(n, st); ++gr)
        for (int k = 0; k < tq::kGroup; ++k) {
          const int p = tq::pixel_of(st, gr, k);
          X = fma(g[p], template_value(p < n ? m[p] : 0.0f), X);
        }
    chi[b] = pair_solve(Sa, Ba, S[b], B[b], X, c0, a == b || in_earlier_slot(cand_star, j, b), &al[b], &be[b]);
  }
}

// The call on the host, as the three launches do.  all may be NULL.  part_c / part_i hold chunks_of(M) * N * kA * topk entries,
// part_amp twice as many; work holds 4 * steps_of(n) * kStep + 5 * M doubles; src holds topk ints.
inline void match_pairs_host(const float* templates, long long ld_t, int M, const float* flux, const double* w, long long ld_f, int N, int n,
                             const int* cand, int kA, int topk, int* idx_a, int* idx_b, double* chisq, double* amp, double* all, long long ld_a,
                             double* part_c, int* part_i, double* part_amp, double* work, int* src) {
  const int chunks = tq::chunks_of(M), R = N * kA;
  const size_t np = (size_t)tq::steps_of(n) * tq::kStep;
  double *a1 = work, *a2 = work + np, *fz = work + 2 * np, *g = work + 3 * np;
  double *B = work + 4 * np, *S = B + M, *chi = S + M, *al = chi + M, *be = al + M;
  for (int s = 0; s < N; ++s) {
    const double c0 = star_host(flux + (size_t)s * (size_t)ld_f, w + (size_t)s * (size_t)ld_f, n, a1, a2, fz);
    moments_host(templates, ld_t, M, a1, a2, n, B, S);
    for (int j = 0; j < kA; ++j) {
      const int r = row_of(s, j, kA);
      row_host(templates, ld_t, M, a2, n, cand + (size_t)s * kA, j, B, S, c0, g, chi, al, be);
      for (int ch = 0; ch < chunks; ++ch) {
        const int t0 = ch * kChunk, count = M - t0 < kChunk ? M - t0 : kChunk;
        const size_t at = tq::part_at(ch, R, r, topk);
        tq::list_from_chunk(part_c + at, part_i + at, topk, chi + t0, t0, count);
        for (int e = 0; e < topk && part_i[at + e] >= 0; ++e) {
          part_amp[2 * (at + e)] = al[part_i[at + e]];
          part_amp[2 * (at + e) + 1] = be[part_i[at + e]];
        }
      }
      if (all)
        for (int b = 0; b < M; ++b) all[(size_t)r * (size_t)ld_a + b] = chi[b];
    }
  }
  for (int s = 0; s < N; ++s) {
    merge_rows(chisq + (size_t)s * topk, idx_b + (size_t)s * topk, src, topk, part_c, part_i, chunks, N, kA, s);
    for (int e = 0; e < topk; ++e)
      idx_a[(size_t)s * topk + e] = finish_entry(src[e], cand, part_amp, chunks, N, kA, s, topk, amp + 2 * ((size_t)s * topk + e));
  }
}

}  // namespace tmatch_pair
}  // namespace payne
