// queue_block.hpp -- the staging block of the sampler's random-walk queue: its format, written once (host code, no GPU include).
//
// A queue is ONE block of doubles, on the device (payne_sampler::q_dev) and in mapped host memory (q_host, dq_host[2]):
//
//   region     doubles                     holds                                              travels
//   u          K nd                        the chains' unit-cube points                       up (start points) and down (results)
//   v          K nd                        the chains' transformed points                     up and down
//   lnprob     K                           the chains' lnprob                                 up and down
//   counters   (3 K + 1) / 2               int nacc[K] | ncall[K] | nredraw[K]                down (their slots go up unused)
//   axes       n_ell nd nd                 the ellipsoids' unit axes                          up
//   ctr        n_ell nd      (n_ell > 1)   the ellipsoids' centres                            up
//   ainv       n_ell nd nd   (n_ell > 1)   the ellipsoids' inverse axes                       up
//   ell        (K + 1) / 2   (n_ell > 1)   int ell[K]: each chain's ellipsoid                 never (the walk's first step writes it)
//
// One transfer each way: [0, n_down()) comes back, [0, n_up()) goes up.  Every region starts where the one before it ends, so
// the offsets depend on K and n_ell; the allocation is sized for (k_max, nd, PAYNE_MAX_ELL): capacity(k_max, nd).
// Behind the block, on the host copies only:
//   q_host    capacity + kQHostTail doubles:   the completion word at capacity                  (HostBlock q_host_block)
//   dq_host   capacity + kDqHostTail doubles:  the completion word at capacity + 8              (HostBlock dq_host_block)
//             and the {scale, loglstar} pair the queue ran under at n_down() of the queue's OWN K (Layout::dyn_pair): nothing
//             goes up through a dq_host block -- a new bound has a mapped block of its own, bound_capacity(nd) doubles --, so
//             the slots behind what came down are free.
#pragma once
#include <math.h>

#include <cstddef>
#include <cstring>

#include "../../include/payne_hip.h"

namespace payne_queue {

// one block seen through its regions (ctr / ainv / ell: null with a single ellipsoid)
struct View {
  double *u, *v, *lnprob;
  int *nacc, *ncall, *nredraw;
  double *axes, *ctr, *ainv;
  int* ell;
};

inline size_t bound_capacity(size_t nd) { return (size_t)PAYNE_MAX_ELL * (2 * nd * nd + nd); }
// doubles of a block that holds any queue of up to k_max chains
inline size_t capacity(size_t k_max, size_t nd) { return k_max * (2 * nd + 1) + (3 * k_max + 1) / 2 + bound_capacity(nd) + (k_max + 1) / 2; }

struct Layout {
  size_t K, nd, n_ell;
  Layout(int K_, int nd_, int n_ell_) : K((size_t)K_), nd((size_t)nd_), n_ell((size_t)n_ell_) {}
  // offsets (doubles)
  size_t u() const { return 0; }
  size_t v() const { return K * nd; }
  size_t lnprob() const { return 2 * K * nd; }
  size_t counters() const { return K * (2 * nd + 1); }
  size_t axes() const { return counters() + n_counters(); }
  size_t ctr() const { return axes() + n_axes(); }
  size_t ainv() const { return ctr() + n_ell * nd; }
  size_t ell() const { return axes() + n_bound(); }
  // lengths (doubles)
  size_t n_counters() const { return (3 * K + 1) / 2; }
  size_t n_axes() const { return n_ell * nd * nd; }
  size_t n_bound() const { return n_ell > 1 ? 2 * n_axes() + n_ell * nd : n_axes(); }     // axes | ctr | ainv
  size_t n_ell_ints() const { return n_ell > 1 ? (K + 1) / 2 : 0; }
  size_t n_down() const { return counters() + n_counters(); }                              // chains, then the three counters
  size_t n_up() const { return n_down() + n_bound(); }                                     // ... and the bound behind them
  size_t end() const { return ell() + n_ell_ints(); }
  size_t dyn_pair() const { return n_down(); }                                             // (dq_host blocks only)
  View view(double* b) const {
    int* c = reinterpret_cast<int*>(b + counters());
    const bool multi = n_ell > 1;
    return View{b + u(), b + v(), b + lnprob(), c, c + K, c + 2 * K, b + axes(), multi ? b + ctr() : nullptr,
                multi ? b + ainv() : nullptr, multi ? reinterpret_cast<int*>(b + ell()) : nullptr};
  }
};

// a mapped host copy of the block: its allocation and where its completion word sits (both in doubles)
struct HostBlock { size_t doubles, flag; };
constexpr size_t kQHostTail = 8, kDqHostTail = 16;
inline HostBlock q_host_block(size_t k_max, size_t nd) { return {capacity(k_max, nd) + kQHostTail, capacity(k_max, nd)}; }
inline HostBlock dq_host_block(size_t k_max, size_t nd) { return {capacity(k_max, nd) + kDqHostTail, capacity(k_max, nd) + 8}; }

// axes | ctr | ainv as they travel up (dst: a block's axes region, or the device turn's mapped block for the bound)
inline void pack_bound(const Layout& L, double* dst, const double* axes_unit, const double* ctr, const double* ainv) {
  std::memcpy(dst, axes_unit, L.n_axes() * 8);
  if (L.n_ell > 1) {
    std::memcpy(dst + (L.ctr() - L.axes()), ctr, L.n_ell * L.nd * 8);
    std::memcpy(dst + (L.ainv() - L.axes()), ainv, L.n_axes() * 8);
  }
}

// the ellipsoid list of a call: null when it is fine, else the message (`per_ell`: the call has what several ellipsoids need --
// the chains' indices, or centres and inverse axes; `ell`: per-chain indices to range-check, or null)
inline const char* check_ell_list(int n_ell, bool per_ell, const int* ell = nullptr, int K = 0) {
  if (n_ell < 1 || n_ell > PAYNE_MAX_ELL || (n_ell > 1 && !per_ell)) return "bad ellipsoid list";
  if (ell)
    for (int i = 0; i < K; ++i)
      if (ell[i] < 0 || ell[i] >= n_ell) return "ellipsoid index out of range";
  return nullptr;
}

inline unsigned long long mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// ---- start points: uniform among the live points (splitmix of the seed).  With several ellipsoids the walk's first step finds
//      the one each chain steps in on the device (walk_assign_ell: on the host that loop was 8 us per ellipsoid, before the GPU
//      could start)
// `src` (payne_ns_rwalk_queue_turn): live slot i holds row src[i] of (qu, qv) with lnprob lg[i] when src[i] >= 0 -- the live set a
// queue's consumption will leave, by index (payne_ns::peek_index), never copied
inline void fill_starts(const Layout& L, double* blk, unsigned long long seed, int nlive, const double* live_u, const double* live_v,
                        const double* live_logl, const int* src, const double* qu, const double* qv, const double* lg) {
  const int K = (int)L.K, nd = (int)L.nd;
  double *hu = blk + L.u(), *hv = blk + L.v(), *hl = blk + L.lnprob();
  for (int k = 0; k < K; ++k) {
    const unsigned long long r0 = mix(seed ^ (0xA5A5A5A5ull + (unsigned long long)k * 0x100000001B3ull));
    const int i = (int)(r0 % (unsigned long long)nlive);
    const bool q = src && src[i] >= 0;
    // (rows of a dozen doubles, 2 K of them between two queues: copied in place -- a memcpy call each was 20 us of the turn)
    const double* su = q ? qu + (size_t)src[i] * nd : live_u + (size_t)i * nd;
    const double* sv = q ? qv + (size_t)src[i] * nd : live_v + (size_t)i * nd;
    double* du_ = hu + (size_t)k * nd;
    double* dv_ = hv + (size_t)k * nd;
    for (int d = 0; d < nd; ++d) { du_[d] = su[d]; dv_[d] = sv[d]; }
    hl[k] = src ? lg[i] : live_logl[i];
  }
}

// ---- the chains that moved are the queue; a chain that never moved is a copy of a live point
inline void queue_extract(const double* hu, int K, int nd, double* qu, double* qv, double* ql, int* qnc, int* nq, long long* stats) {
  const Layout L(K, nd, 1);                                      // (what comes down lies in front of the bound)
  const double *hv = hu + L.v(), *hl = hu + L.lnprob();
  long long acc = 0, calls = 0, redraw = 0, idle_calls = 0;
  int m = 0;
  const int *na = reinterpret_cast<const int*>(hu + L.counters()), *nc = na + K, *nr = nc + K;
  for (int k = 0; k < K; ++k) {
    acc += na[k]; calls += nc[k]; redraw += nr[k];
    if (na[k] > 0) {
      const double* su = hu + (size_t)k * nd;
      const double* sv = hv + (size_t)k * nd;
      double* du_ = qu + (size_t)m * nd;
      double* dv_ = qv + (size_t)m * nd;
      for (int d = 0; d < nd; ++d) { du_[d] = su[d]; dv_[d] = sv[d]; }
      const double l = hl[k];
      ql[m] = (l != l) ? -INFINITY : l;
      qnc[m] = nc[k] > 1 ? nc[k] : 1;
      ++m;
    } else {
      idle_calls += nc[k];
    }
  }
  *nq = m;
  stats[0] = acc; stats[1] = calls; stats[2] = redraw; stats[3] = idle_calls;
}

// the step scale after a queue with these counters (dynesty's rule, as thepayne_amd/sampler/nested.py applies it)
inline double adapt_scale(double scale, const long long* stats, int nd) {
  const long long denom = stats[1] + stats[2] > 1 ? stats[1] + stats[2] : 1;
  const double frac = (double)stats[0] / (double)denom;          // a redrawn (out-of-cube) proposal counts as a rejection
  double sc = scale * exp((frac - 0.5) / nd / 0.5);
  sc = sc > 1e-4 ? sc : 1e-4;
  return sc < 4.0 ? sc : 4.0;
}

}  // namespace payne_queue
