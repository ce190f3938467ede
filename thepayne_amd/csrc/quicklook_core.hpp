// quicklook_core.hpp -- arithmetic of the two quick-look scans (Payne/fitting/fitutils.py: RVcalc.chisq_rv :79-94,
// BROADcalc.chisq_broad :131-155), written host/device so that the same source runs
//   * on gfx950 inside payne_rv_scan_kernel / payne_chisq_below_kernel (k_quicklook.hip), and
//   * on the host (tests/emul/quicklook_emul.cpp: every thread of a workgroup in turn) as the CPU-side check, also under
//     ASan/UBSan.
// Everything is fp64.  Sums are formed in ONE fixed order -- a thread's pixels in ascending order, the 64 lanes of a wave by
// the halving tree of ql_tree64 (what the shuffles of the kernel do), the waves in ascending order -- so the same call gives the
// same bits every time; there are no floating-point atomics.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PAYNE_QL_HD __host__ __device__ __forceinline__
#else
#define PAYNE_QL_HD inline
#endif

namespace payne {
namespace ql {

constexpr double kCkmsDoppler = 299792.458;      // scipy.constants.c / 1000 (fitutils.py:5-6)
constexpr int kThreads = 256;                    // one workgroup: four waves
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;

// The shifted model abscissa j: modwave * (1 + rv / c), a PRODUCT as fitutils.py:87 forms it (its rounding decides which
// bracket a pixel on a knot falls in, and whether an end pixel is inside).
PAYNE_QL_HD double doppler_factor(double rv) { return 1.0 + (rv / kCkmsDoppler); }
PAYNE_QL_HD double shifted(const double* modwave, int j, double s) { return modwave[j] * s; }

// interp1d(kind='linear', bounds_error=False, fill_value=1.0)(x) on the shifted grid, by interp1d's own linear rule
// (scipy/interpolate/_interpolate.py, _call_linear + _check_bounds): hi = searchsorted(xs, x, side='left') clipped to
// [1, nm - 1], lo = hi - 1, y_lo + (y_hi - y_lo) / (x_hi - x_lo) * (x - x_lo); x < xs[0] or x > xs[nm-1] gives the fill
// value, both end points are inside.  A NaN in modflux reaches every pixel whose bracket touches it.
// (For fp64 1-d input recent scipy hands the same call to np.interp, whose bracket on a pixel that sits exactly on a knot is
// the one to the RIGHT: the two agree to rounding wherever both neighbours are finite.)
PAYNE_QL_HD double interp_fill(const double* modwave, const double* modflux, int nm, double s, double x) {
  if (x < shifted(modwave, 0, s) || x > shifted(modwave, nm - 1, s)) return 1.0;
  int lo = 0, hi = nm;                           // smallest hi with xs[hi] >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (shifted(modwave, mid, s) < x) lo = mid + 1; else hi = mid;
  }
  hi = hi < 1 ? 1 : (hi > nm - 1 ? nm - 1 : hi);
  const double x_lo = shifted(modwave, hi - 1, s), x_hi = shifted(modwave, hi, s);
  const double y_lo = modflux[hi - 1], y_hi = modflux[hi];
  const double slope = (y_hi - y_lo) / (x_hi - x_lo);
  return slope * (x - x_lo) + y_lo;
}

// ((m - o)**2.0) / (s**2.0), fitutils.py:92, :153
PAYNE_QL_HD double chisq_term(double m, double o, double e) {
  const double d = m - o;
  return (d * d) / (e * e);
}

// What thread `tid` of `nthreads` adds up in the velocity scan: its pixels tid, tid + nthreads, ... in ascending order.
PAYNE_QL_HD double rv_partial(const double* modwave, const double* modflux, int nm, const double* wave, const double* flux,
                              const double* eflux, int nobs, double rv, int tid, int nthreads) {
  const double s = doppler_factor(rv);
  double acc = 0.0;
  for (int i = tid; i < nobs; i += nthreads)
    acc += chisq_term(interp_fill(modwave, modflux, nm, s, wave[i]), flux[i], eflux[i]);
  return acc;
}

// `cond = modflux_i < 0.95` (fitutils.py:148) on an fp32 row: NaN compares false and is dropped.
PAYNE_QL_HD bool keep_below(float v, double threshold) { return (double)v < threshold; }

// Exclusive prefix count inside a wave from its ballot, and of a wave inside the workgroup from the per-wave totals.
PAYNE_QL_HD int lane_prefix(unsigned long long ballot, int lane) {
  return __builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}
PAYNE_QL_HD int wave_prefix(const int* wave_total, int wave) {
  int off = 0;
  for (int w = 0; w < wave; ++w) off += wave_total[w];
  return off;
}

// The term of kept pixel i, the j-th kept one of its row.  BROADcalc.chisq_broad (fitutils.py:148-154) masks the model and
// the flux (`flux = flux[cond]`) but its line `eflux[cond]` discards the result, and zip() stops at the shortest list: the
// j-th kept model value meets the j-th kept flux -- flux[i] -- and eflux[j], the first n_kept entries of the UNMASKED error
// vector.  This build reproduces the reference's arithmetic, not its intent.
PAYNE_QL_HD double below_term(const float* row, const double* flux, const double* eflux, int i, int j) {
  return chisq_term((double)row[i], flux[i], eflux[j]);
}

#ifndef __HIP_DEVICE_COMPILE__
// The order in which the kernels combine the kThreads per-thread sums (host restatement of block_sum in k_quicklook.hip):
// lanes by halving (offset 32, 16, ... 1: what __shfl_down does), then the waves' lane-0 values in ascending order.
inline double tree64(double* v) {
  for (int off = kWave / 2; off > 0; off >>= 1)
    for (int l = 0; l < off; ++l) v[l] += v[l + off];
  return v[0];
}
inline double block_sum_host(double* partial) {
  double total = 0.0;
  for (int w = 0; w < kWaves; ++w) total += tree64(partial + w * kWave);
  return total;
}
#endif

}  // namespace ql
}  // namespace payne
