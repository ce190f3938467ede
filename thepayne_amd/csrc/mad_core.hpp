// mad_core.hpp -- arithmetic of payne_mad_stats (k_mad.hip): medians of the absolute residual |truth - pred| of two fp32
// matrices, down the columns (per pixel, over a set of rows) and along the rows (per spectrum), what
// Payne/testing/testspec.py:94-108 asks of np.median.  Written host/device so that the same source runs
//   * on gfx950 inside payne_mad_cols_kernel / payne_mad_rows_kernel, and
//   * on the host (tests/emul/mad_emul.cpp: every wave of a workgroup in turn, phases separated where the kernels have
//     barriers) as the CPU-side check, also under ASan / UBSan.
// The residual is formed in fp64 from the two fp32 values and never stored.  Selection is most-significant-digit radix
// selection on the order-preserving integer image of the residual (the map of select.hpp): kPasses passes of kBits bits, each
// pass one counting sweep over the data and one walk over the counters.  Only integers are counted and compared: there is no
// sort and no floating-point accumulation, so the result is exact and the same on every call.
//
// One descent finds the element of rank (m-1)>>1 ("lo").  Its last pass leaves the rank r of lo among the c elements equal
// to it; for an even m the element of rank m>>1 ("hi") is lo again when r + 1 < c, and the smallest key above lo otherwise --
// one more sweep (a minimum, not a descent).  A NaN among the members makes the result NaN (np.median, not nanmedian): it is
// flagged in the first sweep; its key sorts above +inf, so the descent itself needs no special case.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define PAYNE_MAD_HD __host__ __device__ __forceinline__
#else
#define PAYNE_MAD_HD inline
#endif

namespace payne {
namespace mad {

constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;         // one workgroup
constexpr int kBits = 8;                         // digit width
constexpr int kBins = 1 << kBits;
constexpr int kPasses = 64 / kBits;
constexpr int kCols = kWave;                     // columns a workgroup of the column kernel owns: one per lane
constexpr int kQuarter = kBins / kWaves;         // bins whose counts one wave adds up before the walk (column kernel)
constexpr int kPerLane = kBins / kWave;          // bins whose counts one lane adds up before the walk (row kernel)
constexpr int kRowUnroll = 4;                    // member rows a wave of the column kernel has in flight
constexpr unsigned long long kNoKey = ~0ull;     // "no key above lo": above every key of a real number (the largest NaN's image)

// np.abs(t.astype(f8) - p.astype(f8)): the difference of two fp32 values rounded once to fp64.
PAYNE_MAD_HD double residual(float truth, float pred) { return fabs((double)truth - (double)pred); }

// order-preserving map double -> uint64 (select.hpp's key_of / value_of, here also for the host); NaN included: |NaN| maps
// above +inf
PAYNE_MAD_HD unsigned long long key_of(double x) {
  unsigned long long b;
  memcpy(&b, &x, sizeof b);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
PAYNE_MAD_HD double value_of(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
}
PAYNE_MAD_HD unsigned long long residual_key(float truth, float pred) { return key_of(residual(truth, pred)); }
PAYNE_MAD_HD bool key_is_nan(unsigned long long k) { return k > 0xFFF0000000000000ull; }     // above key_of(+inf)

PAYNE_MAD_HD int shift_of(int pass) { return 64 - kBits * (pass + 1); }
// Does k carry the digits chosen in the passes before `pass`?  (prefix holds them in their place, zeros below)
PAYNE_MAD_HD bool in_prefix(unsigned long long k, unsigned long long prefix, int pass) {
  return pass == 0 || ((k ^ prefix) >> (shift_of(pass) + kBits)) == 0ull;
}
PAYNE_MAD_HD int digit_of(unsigned long long k, int pass) { return (int)((k >> shift_of(pass)) & (unsigned long long)(kBins - 1)); }

// Walk n counters (stride apart) for the one that holds rank *rank: returns its index and leaves in *rank the rank inside
// it, in *count its count.  The caller guarantees *rank < the counters' sum; the last counter takes what is left.
PAYNE_MAD_HD int find_bin(const unsigned* counts, int stride, int n, unsigned* rank, unsigned* count) {
  unsigned r = *rank;
  int b = 0;
  for (; b < n - 1; ++b) {
    const unsigned c = counts[(size_t)b * (size_t)stride];
    if (r < c) break;
    r -= c;
  }
  *rank = r;
  *count = counts[(size_t)b * (size_t)stride];
  return b;
}

PAYNE_MAD_HD unsigned sum_bins(const unsigned* counts, int stride, int n) {
  unsigned s = 0;
  for (int b = 0; b < n; ++b) s += counts[(size_t)b * (size_t)stride];
  return s;
}

// The state of one selection (one column of a row set, or one row) between the passes.
struct Sel {
  unsigned long long prefix;                     // the digits chosen so far
  unsigned rank;                                 // rank of lo among the elements that carry the prefix
  unsigned count;                                // how many carry it (after the last pass: how many equal lo)
  unsigned m;                                    // members
};

// After the counting sweep of `pass`: choose the digit.  `part` holds n_part sums of consecutive groups of per_part counters
// (stride_part apart); `hist` the counters themselves (stride_hist apart).  Pass 0 also learns m (the sum of everything) and
// from it the rank of lo.
PAYNE_MAD_HD void choose_digit(Sel* s, int pass, const unsigned* part, int stride_part, int n_part, const unsigned* hist,
                               int stride_hist, int per_part) {
  if (pass == 0) {
    s->m = sum_bins(part, stride_part, n_part);
    s->rank = s->m ? (s->m - 1u) >> 1 : 0u;
    s->prefix = 0ull;
  }
  if (s->m == 0u) return;
  unsigned r = s->rank, c = 0u;
  const int q = find_bin(part, stride_part, n_part, &r, &c);
  const int b = find_bin(hist + (size_t)q * (size_t)per_part * (size_t)stride_hist, stride_hist, per_part, &r, &c);
  s->prefix |= (unsigned long long)(q * per_part + b) << shift_of(pass);
  s->rank = r;
  s->count = c;
}

// Does the median need the smallest key above lo?  (even m, and lo is the last of its equals)
PAYNE_MAD_HD bool needs_next(const Sel& s) { return s.m != 0u && (s.m & 1u) == 0u && s.rank + 1u >= s.count; }

// np.median from the two middle keys: 0.5 * (lo + hi) in fp64, as numpy's mean of the two; the odd case returns lo itself.
// `next` is the smallest key above lo (used when needs_next).
PAYNE_MAD_HD double median_of(const Sel& s, unsigned long long next, bool any_nan) {
  if (s.m == 0u || any_nan) return value_of(0xFFF8000000000000ull);          // quiet NaN
  const double lo = value_of(s.prefix);
  if (s.m & 1u) return lo;
  const double hi = needs_next(s) ? value_of(next) : lo;
  return 0.5 * (lo + hi);
}

}  // namespace mad
}  // namespace payne
