// k_sedfit.hip -- payne_sedfit_*: the photometric magnitudes' derivatives and the SED fit of many stars (include/payne_hip.h).  The
// arithmetic is sedfit_core.hpp, which runs on the host too (tests/emul/sedfit_emul.cpp); the step is lmfit_core.hpp's update_star.
//
//   sedfit_filter             one filter's net for the stars of a workgroup on the photometric nets' tile (sed_tile.hpp) with tangent
//     rows: the rows of the 48-row tile X are (star, tangent), star s at rows s (1 + Kn) ..  Layer 1 runs on the stars' encoded
//     labels (Xin [48][8], K = 6 padded to 8) and lands in the stars' value rows; the tangent rows behind it are a1 (1 - a1) times
//     the table W1[:, d] / (xmax_d - xmin_d), a product per element.  Layer 2 runs on all 48 rows, the bias on the value rows only.
//     Both are the tile's sed_mfma; the raw sums go back to LDS, where one thread per (star, unit) applies s(z) to the value row
//     (sed_sigmoid_n, four side by side) and a (1 - a) to the Kn tangent rows above it.  Layer 3 is the tile's, the four partial
//     sums added in wave order by whoever reads them.
//   payne_sedfit_jac_kernel   a workgroup per (filter, 8 stars), all five tangents; eight threads apply the chain rule and store.
//   payne_sedfit_run_kernel   a workgroup per 48 / (1 + Kn) stars for the whole fit: for eval < maxiter { for filter { sedfit_filter;
//     one thread a star forms R; one thread per (star, i, j) adds R_i w R_j to G in LDS }; one thread a star adds the priors and
//     takes update_star's step }, leaving early once no star of the workgroup is RUNNING.  The state of update_star lives in LDS.
//   No atomics; every sum has a fixed order, and a row of the tile depends on that row alone.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/payne_hip.h"
#include "host_prologue.hpp"
#include "sed_core.hpp"
#include "sedfit_core.hpp"

namespace sf = payne::sedfit;
namespace lm = payne::lmfit;

namespace {

using payne::host::DeviceBag;
using payne::host::OnDevice;
using payne::host::fail;

constexpr int kThreads = kSedThreads;

// The handle's device copies: the width padded to Hp with zero weights.
struct Tables {
  int F, Hp;
  const float *w1;     // [F][8][Hp]: [d][h], rows 6, 7 zero
  const float *b1, *b2, *w3;   // [F][Hp]
  const float *w2t;    // [F][Hp][Hp]: [k][h]
  const float *b3;     // [F]
  const double *w1t;   // [F][5][Hp]: sedfit_core.hpp's tangent_weight
  const double *hiav;  // [F][5] or null
  double xmin[sf::kNetIn], xden[sf::kNetIn];
};

// LDS of a workgroup with S stars and K fitted parameters (K = 0: payne_sedfit_jac), in bytes from the start: the tile (SedTileLds),
// then what is the fit's own.
struct Layout {
  size_t tile, Xin, W1T, pars, terms, dm, dbc, G, R, wt, xb, xt, A, g, chisq, lambda, hi, status, niter, at_bound, nfilt, total;
};
__host__ __device__ inline Layout layout_of(int S, int K) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
  L.tile = take(SedTileLds::bytes);
  L.Xin = take((size_t)kSedCandsMax * 8 * 8);
  L.W1T = take((size_t)sf::kMaxTan * kSedMaxH * 8);
  L.pars = take((size_t)S * sf::kMaxK * 8);
  L.terms = take((size_t)S * sizeof(sf::RowTerms));
  L.dm = take((size_t)S * sf::kMaxK * 8);
  L.dbc = take((size_t)S * sf::kMaxTan * 8);
  L.G = take((size_t)S * sf::tile_doubles(K) * 8);
  L.R = take((size_t)S * (K + 1) * 8);
  L.wt = take((size_t)S * 8);
  L.xb = take((size_t)S * K * 8);
  L.xt = take((size_t)S * K * 8);
  L.A = take((size_t)S * K * K * 8);
  L.g = take((size_t)S * K * 8);
  L.chisq = take((size_t)S * 8);
  L.lambda = take((size_t)S * 8);
  L.hi = take((size_t)S * 4);
  L.status = take((size_t)S * 4);
  L.niter = take((size_t)S * 4);
  L.at_bound = take((size_t)S * 4);
  L.nfilt = take((size_t)S * 4);
  L.total = o;
  return L;
}
// update_star's workspace lies on the tile's X, which nobody needs between the last filter of an evaluation and the first of the next
constexpr bool work_fits_on_x() {
  for (int Kn = 0; Kn <= sf::kMaxTan; ++Kn) {
    const int K = Kn + 2 < sf::kMaxK ? Kn + 2 : sf::kMaxK;                  // the most parameters with Kn of them network inputs
    if ((kSedCandsMax / (1 + Kn)) * (2 * K * K + 3 * K) > kSedCandsMax * kSedPitchA) return false;
  }
  return true;
}
static_assert(work_fits_on_x(), "X holds the stars' workspaces");

template <class T>
__device__ __forceinline__ T* at(unsigned char* smem, size_t off) { return reinterpret_cast<T*>(smem + off); }

// Filter f for S stars with Kn tangents each (net inputs tan_in[t]).  In: Xin [s][8], the stars' encoded labels (columns 6, 7 and
// the rows from S on zero).  Out: Pt [4][48], the waves' partial sums of w3 . X[row]; a barrier follows them.  The first barrier
// in here is also the one behind which the caller's writes to Xin are seen and the previous filter's Pt is free.
__device__ inline void sedfit_filter(const Tables& T, int f, int S, int Kn, const int* tan_in, unsigned char* smem, const Layout& L) {
  const int Hp = T.Hp, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SedTileView t = sed_tile_view(smem + L.tile);
  double* X = t.X;
  const double* Xin = at<double>(smem, L.Xin);
  double* W1T = at<double>(smem, L.W1T);
  const int rps = 1 + Kn;                                                   // rows a star
  // ---- requests: the W2 tile and the three vectors, W1, the tangent table
  const SedWeights wr = sed_weights_request(T.w2t + (size_t)f * Hp * Hp, Hp, T.b1 + (size_t)f * Hp, T.b2 + (size_t)f * Hp, T.w3 + (size_t)f * Hp);
  float w1reg[2];
  double w1treg[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = tid + kThreads * q;
    w1reg[q] = T.w1[(size_t)f * 8 * Hp + (i < 8 * Hp ? i : 0)];
    w1treg[q] = T.w1t[(size_t)f * sf::kMaxTan * Hp + (i < sf::kMaxTan * Hp ? i : 0)];
  }
  __syncthreads();
  // ---- commit to LDS
  sed_weights_commit(wr, Hp, t);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = tid + kThreads * q;
    if (i < 8 * Hp) { const int d = i / Hp, h = i - d * Hp; t.W1[d * kSedPitchW + h] = w1reg[q]; }
    if (i < sf::kMaxTan * Hp) { const int d = i / Hp, h = i - d * Hp; W1T[d * kSedMaxH + h] = w1treg[q]; }
  }
  __syncthreads();
  const int nt_n = Hp >> 4, li = lane & 15, lk = lane >> 4;
  const bool on = wave < nt_n;                                              // wave w owns the 16-column tile w (or none)
  const int nt = on ? wave : 0;
  constexpr int MT = kSedCandsMax / 16;
  // s(z) on the value rows, s'(z) on the tangent rows above them: one thread per (star, unit), four units a thread at a time
  auto activate = [&](bool first) {
    const int n = S * Hp;
    for (int base = 0; base < n; base += 4 * kThreads) {
      double z[4];
      int r0[4], hh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = base + tid + kThreads * q, ec = e < n ? e : 0;
        const int s = ec / Hp;
        hh[q] = ec - s * Hp;
        r0[q] = s * rps;
        z[q] = X[r0[q] * kSedPitchA + hh[q]];
      }
      sed_sigmoid_n<4>(z);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (base + tid + kThreads * q < n) {
          const double a = z[q], sp = a * (1.0 - a);
          X[r0[q] * kSedPitchA + hh[q]] = a;
          for (int t = 0; t < Kn; ++t) {
            double* x = X + (r0[q] + 1 + t) * kSedPitchA + hh[q];
            *x = sp * (first ? W1T[tan_in[t] * kSedMaxH + hh[q]] : *x);
          }
        }
      }
    }
  };
  // ---- layer 1 (photANN.py:127): rows are stars
  {
    sed_d4 acc[MT];
    const double bz = (double)t.Bv[16 * nt + li];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (sed_d4){bz, bz, bz, bz};
    if (on) {
      sed_mfma<MT, 2>(Xin, 8, t.W1, 2, nt, li, lk, acc);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int s = 16 * mt + lk + 4 * v;
          if (s < S) X[s * rps * kSedPitchA + 16 * nt + li] = acc[mt][v];
        }
    }
  }
  __syncthreads();
  activate(true);
  __syncthreads();
  // ---- layer 2 (:128): all rows, the bias on the value rows
  {
    sed_d4 acc[MT];
    const double bz = (double)t.Bv[kSedMaxH + 16 * nt + li];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[mt][v] = (16 * mt + lk + 4 * v) % rps == 0 ? bz : 0.0;
    if (on) sed_mfma<MT, kSedMaxH / 4>(X, kSedPitchA, t.W2, Hp >> 2, nt, li, lk, acc);
    __syncthreads();                                                        // every wave has read X
    if (on) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) X[(16 * mt + lk + 4 * v) * kSedPitchA + 16 * nt + li] = acc[mt][v];
    }
  }
  __syncthreads();
  activate(false);
  __syncthreads();
  // ---- layer 3 (:129-131)
  sed_layer3_partials(t, lane, wave, on);
  __syncthreads();
}

// Star s of the workgroup: its row's encoded labels into Xin, whether its Av is on the high branch, what its magnitudes share.
__device__ __forceinline__ void stage_star(const Tables& T, int photscale, const double* row, int s, unsigned char* smem, const Layout& L) {
  sf::Row r;
  sf::encode(row, photscale, T.xmin, T.xden, &r);
  double* xin = at<double>(smem, L.Xin) + s * 8;
#pragma unroll
  for (int d = 0; d < sf::kNetIn; ++d) xin[d] = r.xs[d];
  xin[6] = 0.0;
  xin[7] = 0.0;
  at<int>(smem, L.hi)[s] = r.hi ? 1 : 0;
  sf::row_terms(photscale, row, at<sf::RowTerms>(smem, L.terms) + s);
}

// Star s behind sedfit_filter: the magnitude of filter f and its derivatives (dm [P] in LDS) from the tile's row sums.
__device__ __forceinline__ double chain_star(const Tables& T, const sf::Plan& pl, int f, int s, unsigned char* smem, const Layout& L) {
  const double* Pt = sed_tile_view(smem + L.tile).Pt;
  double* dbc = at<double>(smem, L.dbc) + s * sf::kMaxTan;
  const int r0 = s * (1 + pl.Kn);
  const double bc = (double)T.b3[f] + sed_row_sum(Pt, r0);
  for (int d = 0; d < sf::kMaxTan; ++d) {
    const int t = pl.tan_of[d < 4 ? d : pl.P - 1];
    dbc[d] = t >= 0 ? sed_row_sum(Pt, r0 + 1 + t) : 0.0;
  }
  double m;
  sf::mag_grad(pl.photscale, at<sf::RowTerms>(smem, L.terms)[s], at<double>(smem, L.pars)[s * sf::kMaxK + pl.P - 1], bc, dbc, at<int>(smem, L.hi)[s] != 0,
               T.hiav ? T.hiav + (size_t)5 * f : nullptr, &m, at<double>(smem, L.dm) + s * sf::kMaxK);
  return m;
}

__global__ void __launch_bounds__(kThreads) payne_sedfit_jac_kernel(const Tables T, const sf::Plan pl, const double* __restrict__ pars, int B,
                                                                    double* __restrict__ mags, double* __restrict__ dmags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int S = sf::stars_per_tile(pl.Kn), P = pl.P, tid = threadIdx.x;
  const Layout L = layout_of(S, 0);
  const int f = (int)(blockIdx.x % (unsigned)T.F);
  const long long b0 = (long long)(blockIdx.x / (unsigned)T.F) * S;
  const long long b = b0 + tid;
  const bool live = tid < S && b < B;
  if (tid < S) {
    double* row = at<double>(smem, L.pars) + tid * sf::kMaxK;
    for (int p = 0; p < P; ++p) row[p] = pars[(size_t)(live ? b : b0) * P + p];
    stage_star(T, pl.photscale, row, tid, smem, L);
  } else if (tid < kSedCandsMax) {
    double* xin = at<double>(smem, L.Xin) + tid * 8;
#pragma unroll
    for (int d = 0; d < 8; ++d) xin[d] = 0.0;
  }
  sedfit_filter(T, f, S, pl.Kn, pl.tan_in, smem, L);
  if (live) {
    const double m = chain_star(T, pl, f, tid, smem, L);
    const double* dm = at<double>(smem, L.dm) + tid * sf::kMaxK;
    const size_t o = (size_t)b * T.F + f;
    mags[o] = m;
    for (int p = 0; p < P; ++p) dmags[o * P + p] = dm[p];
  }
}

struct RunArgs {
  int B;
  const double *start, *obs, *w, *mu, *sigma;
  double* pars;
  double* chisq;
  double* A;
  int* status;
  int* niter;
  unsigned* at_bound;
  int* nfilt;
};

__global__ void __launch_bounds__(kThreads) payne_sedfit_run_kernel(const Tables T, const sf::Plan pl, const RunArgs a, const lm::Box box,
                                                                    const payne_lmfit_opts opts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = pl.K, P = pl.P, F = T.F, S = sf::stars_per_tile(pl.Kn), tid = threadIdx.x;
  const Layout L = layout_of(S, K);
  const int tileK = sf::tile_doubles(K), K1 = K + 1;
  const long long b = (long long)blockIdx.x * S + tid;
  const bool mine = tid < S, live = mine && b < a.B;
  const lm::State st{at<double>(smem, L.xb), at<double>(smem, L.xt), at<double>(smem, L.A), at<double>(smem, L.g), at<double>(smem, L.chisq),
                     at<double>(smem, L.lambda), at<int>(smem, L.status), at<int>(smem, L.niter), at<unsigned>(smem, L.at_bound)};
  double* G = at<double>(smem, L.G);
  double* R = at<double>(smem, L.R);
  double* wt = at<double>(smem, L.wt);
  double* rowp = at<double>(smem, L.pars) + tid * sf::kMaxK;                // (threads below S only)
  const double* sig = live && a.sigma ? a.sigma + (size_t)b * K : nullptr;
  const double* mu = live && a.mu ? a.mu + (size_t)b * K : nullptr;
  if (mine) {
    for (int p = 0; p < P; ++p) rowp[p] = live ? a.start[(size_t)b * P + p] : 0.0;
    double* x0 = st.x_best + (size_t)tid * K;                               // (begin_star reads x0[k] before it writes x_best[k])
    for (int k = 0; k < K; ++k) x0[k] = rowp[pl.par[k]];
    lm::begin_star(st, (size_t)tid, K, x0, box, opts.lambda0);
    const int nf = live ? sf::count_filters(a.w + (size_t)b * F, F) : 0;
    at<int>(smem, L.nfilt)[tid] = nf;
    if (!live) {
      st.status[tid] = PAYNE_LMFIT_CONVERGED;                               // (no star: never RUNNING, never stored)
    } else if (sf::too_few(nf, K, sig)) {
      st.status[tid] = PAYNE_SEDFIT_TOO_FEW;
      st.chisq[tid] = __builtin_nan("");
    }
  } else if (tid < kSedCandsMax) {
    double* xin = at<double>(smem, L.Xin) + tid * 8;
#pragma unroll
    for (int d = 0; d < 8; ++d) xin[d] = 0.0;
  }
  __syncthreads();
  for (int eval = 0; eval < opts.maxiter; ++eval) {
    if (!__syncthreads_or(mine && st.status[tid] == PAYNE_LMFIT_RUNNING)) break;
    for (int e = tid; e < S * tileK; e += kThreads) G[e] = 0.0;
    if (mine) {
      for (int k = 0; k < K; ++k) rowp[pl.par[k]] = st.x_trial[(size_t)tid * K + k];
      stage_star(T, pl.photscale, rowp, tid, smem, L);
    }
    for (int f = 0; f < F; ++f) {
      sedfit_filter(T, f, S, pl.Kn, pl.tan_in, smem, L);
      if (mine) {
        const double m = chain_star(T, pl, f, tid, smem, L);
        const double w = live ? a.w[(size_t)b * F + f] : 0.0;
        sf::residual_row(pl, m, at<double>(smem, L.dm) + tid * sf::kMaxK, w != 0.0 ? a.obs[(size_t)b * F + f] : 0.0, R + tid * K1);
        wt[tid] = w;
      }
      __syncthreads();
      for (int e = tid; e < S * K1 * K1; e += kThreads) {
        const int s = e / (K1 * K1), ij = e - s * K1 * K1, i = ij / K1, j = ij - i * K1;
        const double w = wt[s];
        double* g = G + s * tileK + i * lm::kTile + j;
        if (w != 0.0) *g = sf::tile_add(*g, R[s * K1 + i], R[s * K1 + j], w);
      }
    }
    __syncthreads();
    if (live && st.status[tid] == PAYNE_LMFIT_RUNNING) {
      sf::add_priors(G + tid * tileK, K, st.x_trial + (size_t)tid * K, mu, sig);
      lm::update_star(st, (size_t)tid, K, G + tid * tileK, opts, box, sed_tile_view(smem + L.tile).X + tid * sf::work_doubles(K));
    }
  }
  __syncthreads();
  if (live) {
    for (int k = 0; k < K; ++k) rowp[pl.par[k]] = st.x_best[(size_t)tid * K + k];
    for (int p = 0; p < P; ++p) a.pars[(size_t)b * P + p] = rowp[p];
    a.status[b] = st.status[tid];
    if (a.chisq) a.chisq[b] = st.chisq[tid];
    if (a.niter) a.niter[b] = st.niter[tid];
    if (a.at_bound) a.at_bound[b] = st.at_bound[tid];
    if (a.nfilt) a.nfilt[b] = at<int>(smem, L.nfilt)[tid];
  }
  if (a.A) {
    const long long b0 = (long long)blockIdx.x * S;
    for (int e = tid; e < S * K * K; e += kThreads)
      if (b0 + e / (K * K) < a.B) a.A[(size_t)b0 * K * K + e] = st.A[e];
  }
}

}  // namespace

struct payne_sedfit {
  int device = 0, F = 0, H = 0;
  Tables T;
  DeviceBag bag;
};

namespace {

size_t max_lds_bytes() {
  size_t m = 0;
  for (int Kn = 0; Kn <= sf::kMaxTan; ++Kn) {
    const size_t n = layout_of(sf::stars_per_tile(Kn), Kn + 2 < sf::kMaxK ? Kn + 2 : sf::kMaxK).total;
    m = n > m ? n : m;
  }
  return m;
}

}  // namespace

extern "C" int payne_sedfit_create(int device, int F, int H, const float* w1, const float* b1, const float* w2, const float* b2,
                                   const float* w3, const float* b3, const double* xmin, const double* xmax, const double* hiav,
                                   payne_sedfit** out) {
  if (!out) return fail(PAYNE_E_INVALID, "payne_sedfit_create: null handle pointer");
  *out = nullptr;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !xmin || !xmax) return fail(PAYNE_E_INVALID, "payne_sedfit_create: a null array");
  if (F < 1 || H < 1) return fail(PAYNE_E_INVALID, "payne_sedfit_create: F < 1 or H < 1");
  if (H > sf::kMaxH) return fail(PAYNE_E_UNSUPPORTED, "payne_sedfit_create: H > 64 (the tile holds 64 units)");
  for (int d = 0; d < sf::kNetIn; ++d)
    if (!sf::finite(xmin[d]) || !sf::finite(xmax[d]) || !(xmin[d] < xmax[d])) return fail(PAYNE_E_INVALID, "payne_sedfit_create: xmin / xmax");
  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_sedfit_create: hipSetDevice");
  const int Hp = sed_padded_width(H);
  const size_t f_n = (size_t)F, hp = (size_t)Hp;
  std::vector<float> W1(f_n * 8 * hp, 0.f), B1(f_n * hp, 0.f), W2(f_n * hp * hp, 0.f), B2(f_n * hp, 0.f), W3(f_n * hp, 0.f), B3(b3, b3 + F);
  std::vector<double> W1T(f_n * sf::kMaxTan * hp, 0.0);
  payne_sedfit* h = new payne_sedfit;
  h->device = device;
  h->F = F;
  h->H = H;
  Tables& T = h->T;
  T.F = F;
  T.Hp = Hp;
  T.hiav = nullptr;
  for (int d = 0; d < sf::kNetIn; ++d) {
    T.xmin[d] = xmin[d];
    T.xden[d] = xmax[d] - xmin[d];
  }
  for (size_t f = 0; f < f_n; ++f)
    for (int hh = 0; hh < H; ++hh) {
      const size_t u = f * H + hh;
      for (int d = 0; d < sf::kNetIn; ++d) W1[(f * 8 + d) * hp + hh] = w1[u * sf::kNetIn + d];
      for (int d = 0; d < sf::kMaxTan; ++d) W1T[(f * sf::kMaxTan + d) * hp + hh] = sf::tangent_weight(w1[u * sf::kNetIn + d], T.xden[d]);
      B1[f * hp + hh] = b1[u];
      B2[f * hp + hh] = b2[u];
      W3[f * hp + hh] = w3[u];
    }
  sed_transpose_w2(F, H, Hp, w2, W2.data());
  DeviceBag& bag = h->bag;
  T.w1 = bag.upload(W1); T.b1 = bag.upload(B1); T.w2t = bag.upload(W2); T.b2 = bag.upload(B2); T.w3 = bag.upload(W3);
  T.b3 = bag.upload(B3); T.w1t = bag.upload(W1T);
  if (hiav) T.hiav = bag.upload(std::vector<double>(hiav, hiav + 5 * f_n));
  const int lds = (int)max_lds_bytes();
  const bool ok = bag.ok && hipFuncSetAttribute(reinterpret_cast<const void*>(payne_sedfit_jac_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess &&
                  hipFuncSetAttribute(reinterpret_cast<const void*>(payne_sedfit_run_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
  if (!ok) {
    payne_sedfit_destroy(h);
    return fail(PAYNE_E_HIP, "payne_sedfit_create: uploading the nets failed");
  }
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_sedfit_jac(payne_sedfit* h, const double* pars_dev, int B, int photscale, double* mags_dev, double* dmags_dev,
                                void* stream) {
  if (!h || B < 0 || (photscale != 0 && photscale != 1)) return PAYNE_E_INVALID;
  if (B == 0) return PAYNE_OK;
  if (!pars_dev || !mags_dev || !dmags_dev) return PAYNE_E_INVALID;
  sf::Plan pl;
  if (!sf::make_plan(photscale, (1u << sf::n_pars(photscale)) - 1u, &pl)) return PAYNE_E_INVALID;
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  const int S = sf::stars_per_tile(pl.Kn);
  const unsigned long long blocks = (unsigned long long)((B + S - 1) / S) * (unsigned long long)h->F;
  if (blocks > 0x7fffffffull) return PAYNE_E_UNSUPPORTED;
  hipLaunchKernelGGL(payne_sedfit_jac_kernel, dim3((unsigned)blocks), dim3(kThreads), layout_of(S, 0).total, reinterpret_cast<hipStream_t>(stream),
                     h->T, pl, pars_dev, B, mags_dev, dmags_dev);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" int payne_sedfit_run(payne_sedfit* h, int photscale, unsigned free_mask, const double* start_dev, const double* obs_dev,
                                const double* w_dev, int B, const double* lo, const double* hi, const double* prior_mu_dev,
                                const double* prior_sigma_dev, const payne_lmfit_opts* opts, double* pars_dev, double* chisq_dev,
                                double* A_dev, int* status_dev, int* niter_dev, unsigned* at_bound_dev, int* nfilt_dev, void* stream) {
  if (!h || B < 0 || (prior_mu_dev == nullptr) != (prior_sigma_dev == nullptr)) return PAYNE_E_INVALID;
  const int rc = sf::check_run(photscale, free_mask, lo, hi, opts);
  if (rc != PAYNE_OK) return rc;
  if (B == 0) return PAYNE_OK;
  if (!start_dev || !obs_dev || !w_dev || !pars_dev || !status_dev) return PAYNE_E_INVALID;
  sf::Plan pl;
  sf::make_plan(photscale, free_mask, &pl);
  lm::Box box;
  for (int k = 0; k < lm::kMaxK; ++k) {
    box.lo[k] = k < pl.K ? lo[k] : 0.0;
    box.hi[k] = k < pl.K ? hi[k] : 1.0;
  }
  OnDevice on(h->device);
  if (!on.ok()) return PAYNE_E_HIP;
  const int S = sf::stars_per_tile(pl.Kn);
  const RunArgs a{B, start_dev, obs_dev, w_dev, prior_mu_dev, prior_sigma_dev, pars_dev, chisq_dev, A_dev, status_dev, niter_dev, at_bound_dev, nfilt_dev};
  hipLaunchKernelGGL(payne_sedfit_run_kernel, dim3((unsigned)((B + S - 1) / S)), dim3(kThreads), layout_of(S, pl.K).total,
                     reinterpret_cast<hipStream_t>(stream), h->T, pl, a, box, opts ? *opts : lm::default_opts());
  return hipGetLastError() == hipSuccess ? PAYNE_OK : PAYNE_E_HIP;
}

extern "C" void payne_sedfit_destroy(payne_sedfit* h) { payne::host::destroy(h, true); }
