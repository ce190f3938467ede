// tmatch_core.hpp -- arithmetic of payne_tmatch_* (k_tmatch.hip): brute-force chi^2 of N spectra against a bank of M templates as one
// N x M matrix product on the fp64 matrix instruction, and the top-k selection behind it.  Plain C++, host / device: the same source
// runs in the kernels and on the host (tests/emul/tmatch_emul.cpp, also under ASan / UBSan).  Nothing here indexes a private array:
// every array is the caller's (LDS or global memory in the kernel), so the kernels have no scratch.
//   value    chi^2[s][t] = c0[s] + sum_p (a1[s][p] * (-2 m[t][p]) + a2[s][p] * m[t][p]^2), a1 = w f, a2 = w, c0 = sum_p a1 f, all fp64;
//            m is widened before it is doubled and squared, so both template operands are exact.
//   operands star side: a pixel with w == 0 or beyond n gives a1 = a2 = 0 (and adds nothing to c0) by a select, whatever the flux holds.
//            Template side: a value beyond n, or one that is not finite, gives zero operands by a select; a template value that is not
//            finite at a pixel where the star's w != 0 makes that pair's chi^2 NaN (pair_poisoned: the kernel looks only in the steps
//            in which a template value was not finite).  A NaN in the flux or in w at a weighted pixel reaches chi^2 through a1, a2, c0.
//   pixels   in steps of kStep = 32 (one LDS stage), inside a step in groups of four.  For group g the lane (i = lane & 15, k = lane >> 4)
//            hands pixel p = 32 step + 4 g + k to two matrix instructions: first A = a1 (stars as rows), B = -2 m (templates as columns),
//            then A = a2, B = m^2.  One instruction adds its four products k = 0 .. 3 to the accumulator as a chain of fused
//            multiply-adds; the accumulator starts at +0 and chi^2 = c0 + accumulator (one addition).
//   c0       pixel p adds fma(a1, f, .) to partial sum p % 32 of its star (the staging thread's own sum, steps in order); c0 is the 32
//            partial sums added j = 0 .. 31.
//   tile     a workgroup owns kStars = 64 stars x kChunk = 128 templates: wave v the templates 32 v .. 32 v + 31, as 4 x 2 accumulator
//            tiles of 16 x 16 (acc_star / acc_template below).  Grid = star tiles x template chunks.
//   top-k    ascending in (chi^2, template index); NaN never enters; an empty slot is idx = -1, chi^2 = +inf.  list_insert needs its
//            candidates in ascending template order; a workgroup leaves its chunk's list in the workspace and merge_chunks walks a
//            star's chunks in chunk order.  No atomics, one fixed order: the same inputs give the same bytes, and nothing in a star's
//            arithmetic depends on its place in the tile or on the other stars.
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/payne_hip.h"

#if defined(__HIPCC__)
#define PAYNE_TMATCH_HD __host__ __device__ inline
#else
#define PAYNE_TMATCH_HD inline
#endif

namespace payne {
namespace tmatch {

constexpr int kMaxTopk = PAYNE_TMATCH_MAX_TOPK;
constexpr int kStars = 64;                         // stars of a workgroup's tile
constexpr int kChunk = 128;                        // templates of a workgroup's tile = of one partial top-k list
constexpr int kStep = 32;                          // pixels of one LDS stage
constexpr int kGroup = 4;                          // pixels of one matrix instruction
constexpr int kWave = 64, kWaves = 4, kThreads = kWave * kWaves;
constexpr int kStarRegs = kStars * kStep / kThreads;      // 8: star values a thread stages per step
constexpr int kTemplRegs = kChunk * kStep / kThreads;     // 16: template values a thread stages per step
constexpr int kPitchA = kStep + 2;                 // doubles: lanes i = 0..15, k = 0..1 of one 8-byte read fall on distinct bank pairs
constexpr int kPitchT = kStep + 4;                 // floats: lanes i = 0..15, k = 0..3 of one 4-byte read fall on distinct banks
constexpr int kPitchChi = kChunk + 1;              // doubles: a thread a star walks its row without conflicts

PAYNE_TMATCH_HD int steps_of(int n) { return (n + kStep - 1) / kStep; }
PAYNE_TMATCH_HD int groups_in_step(int n, int step) {
  const int left = n - step * kStep;
  return left >= kStep ? kStep / kGroup : (left + kGroup - 1) / kGroup;
}
PAYNE_TMATCH_HD int tiles_of(int N) { return (N + kStars - 1) / kStars; }
PAYNE_TMATCH_HD int chunks_of(int M) { return (M + kChunk - 1) / kChunk; }
PAYNE_TMATCH_HD int pixel_of(int step, int g, int k) { return kStep * step + kGroup * g + k; }

// staging: value r of thread tid is row (of the tile's stars or templates) stage_row and pixel stage_pixel of the step
PAYNE_TMATCH_HD int stage_row(int tid, int r) { return (tid >> 5) + (kThreads / kStep) * r; }
PAYNE_TMATCH_HD int stage_pixel(int tid) { return tid & (kStep - 1); }
// accumulators: register reg of tile (rb, cb) of wave v, lane `lane`
PAYNE_TMATCH_HD int acc_star(int rb, int reg, int lane) { return 16 * rb + 4 * reg + (lane >> 4); }
PAYNE_TMATCH_HD int acc_template(int wave, int cb, int lane) { return 32 * wave + 16 * cb + (lane & 15); }
PAYNE_TMATCH_HD int acc_bit(int rb, int cb, int reg) { return 8 * rb + 4 * cb + reg; }

PAYNE_TMATCH_HD bool finite32(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// The star's operands at one pixel; `inside`: the star is one of the call's and the pixel is below n.  *fz is the flux as c0 sees it.
PAYNE_TMATCH_HD void star_operands(float f, double w, bool inside, double* a1, double* a2, double* fz) {
  const bool counts = inside && w != 0.0;
  const double fd = (double)f;
  *a1 = counts ? w * fd : 0.0;
  *a2 = counts ? w : 0.0;
  *fz = counts ? fd : 0.0;
}
PAYNE_TMATCH_HD double c0_add(double a1, double fz, double c0) { return fma(a1, fz, c0); }

// The template's operands from the staged value (zero where the template is not one of the call's or the pixel is beyond n).
PAYNE_TMATCH_HD void template_operands(float m, double* b1, double* b2) {
  const double md = finite32(m) ? (double)m : 0.0;
  *b1 = -2.0 * md;
  *b2 = md * md;
}
// a2 is the star's staged weight operand, m the template's staged value, at one pixel
PAYNE_TMATCH_HD bool pair_poisoned(double a2, float m) { return a2 != 0.0 && !finite32(m); }

// ---- the top-k list: c [k], idx [k], ascending in (c, idx) -------------------------------------------------------------------------
PAYNE_TMATCH_HD void list_clear(double* c, int* idx, int k) {
  for (int j = 0; j < k; ++j) {
    c[j] = INFINITY;
    idx[j] = -1;
  }
}
// Candidates arrive in ascending t, so an equal chi^2 goes behind the ones already there.
PAYNE_TMATCH_HD void list_insert(double* c, int* idx, int k, double v, int t) {
  if (v != v) return;
  if (idx[k - 1] >= 0 && !(v < c[k - 1])) return;
  int pos = k - 1;
  while (pos > 0 && (idx[pos - 1] < 0 || v < c[pos - 1])) {
    c[pos] = c[pos - 1];
    idx[pos] = idx[pos - 1];
    --pos;
  }
  c[pos] = v;
  idx[pos] = t;
}
// One chunk's part of a star's row: chi [count] holds templates t0 .. t0 + count - 1 (pitch 1).
PAYNE_TMATCH_HD void list_from_chunk(double* c, int* idx, int k, const double* chi, int t0, int count) {
  list_clear(c, idx, k);
  for (int j = 0; j < count; ++j) list_insert(c, idx, k, chi[j], t0 + j);
}
// The workspace holds chunk ch's list of star s at ((ch * N + s) * k).
PAYNE_TMATCH_HD size_t part_at(int ch, int N, int s, int k) { return ((size_t)ch * (size_t)N + (size_t)s) * (size_t)k; }
PAYNE_TMATCH_HD void merge_chunks(double* c, int* idx, int k, const double* part_c, const int* part_i, int chunks, int N, int s) {
  list_clear(c, idx, k);
  for (int ch = 0; ch < chunks; ++ch) {
    const size_t at = part_at(ch, N, s, k);
    for (int j = 0; j < k && part_i[at + j] >= 0; ++j) list_insert(c, idx, k, part_c[at + j], part_i[at + j]);
  }
}

// ---- one star's row on the host in the kernel's own order ---------------------------------------------------------------------------
// row [M]; work holds 3 * steps_of(n) * kStep doubles (a1, a2 and the flux as c0 sees it, zero beyond n).  Returns c0.
inline double row_host(const float* templates, long long ld_t, int M, const float* flux, const double* w, int n, double* row, double* work) {
  const int steps = steps_of(n), np = steps * kStep;
  double *a1 = work, *a2 = work + np, *fz = work + 2 * np;
  for (int p = 0; p < np; ++p) star_operands(p < n ? flux[p] : 0.0f, p < n ? w[p] : 0.0, p < n, &a1[p], &a2[p], &fz[p]);
  double c0 = 0.0;
  for (int j = 0; j < kStep; ++j) {
    double part = 0.0;
    for (int st = 0; st < steps; ++st) part = c0_add(a1[st * kStep + j], fz[st * kStep + j], part);
    c0 += part;
  }
  for (int t = 0; t < M; ++t) {
    const float* m = templates + (size_t)t * (size_t)ld_t;
    double acc = 0.0;
    bool poisoned = false;
    for (int st = 0; st < steps; ++st)
      for (int g = 0; g < groups_in_step(n, st); ++g) {
        double b1[kGroup], b2[kGroup];
        for (int k = 0; k < kGroup; ++k) {
          const int p = pixel_of(st, g, k);
          const float mv = p < n ? m[p] : 0.0f;
          template_operands(mv, &b1[k], &b2[k]);
          poisoned = poisoned || pair_poisoned(a2[p], mv);
        }
        for (int k = 0; k < kGroup; ++k) acc = fma(a1[pixel_of(st, g, k)], b1[k], acc);
        for (int k = 0; k < kGroup; ++k) acc = fma(a2[pixel_of(st, g, k)], b2[k], acc);
      }
    row[t] = poisoned ? (double)NAN : c0 + acc;
  }
  return c0;
}

// The call on the host: rows through row_host, every chunk's list, then the merge, as the two launches do.  all may be NULL.
// part_c / part_i hold chunks_of(M) * N * topk entries; work as row_host's plus M doubles (the row).
inline void match_host(const float* templates, long long ld_t, int M, const float* flux, const double* w, long long ld_f, int N, int n,
                       int topk, int* idx, double* chisq, double* all, long long ld_a, double* part_c, int* part_i, double* work) {
  const int chunks = chunks_of(M);
  double* row = work + 3 * (size_t)steps_of(n) * kStep;
  for (int s = 0; s < N; ++s) {
    row_host(templates, ld_t, M, flux + (size_t)s * (size_t)ld_f, w + (size_t)s * (size_t)ld_f, n, row, work);
    for (int ch = 0; ch < chunks; ++ch) {
      const int t0 = ch * kChunk, count = M - t0 < kChunk ? M - t0 : kChunk;
      const size_t at = part_at(ch, N, s, topk);
      list_from_chunk(part_c + at, part_i + at, topk, row + t0, t0, count);
    }
    if (all)
      for (int t = 0; t < M; ++t) all[(size_t)s * (size_t)ld_a + t] = row[t];
  }
  for (int s = 0; s < N; ++s) merge_chunks(chisq + (size_t)s * topk, idx + (size_t)s * topk, topk, part_c, part_i, chunks, N, s);
}

}  // namespace tmatch
}  // namespace payne
