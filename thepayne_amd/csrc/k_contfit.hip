// k_contfit.hip -- payne_contfit_batch: continuum polynomials for many stars (include/payne_hip.h).  The arithmetic is
// contfit_core.hpp, which runs on the host too (tests/emul/contfit_emul.cpp); fit_star_host there is this kernel's sequence.
//
//   payne_contfit_kernel  one 256-thread workgroup a star.  Passes over the star's flux (4 B), w (8 B) and model (4 B) per pixel;
//     x is shared by every star and stays in cache.
//       sums      normal_tile.hpp's loop (wave_sums, sum_waves): lane (i = lane & 15, q = lane >> 4) of every wave takes four
//                 consecutive pixels and forms row i of R = [m T_0(x) .. m T_P-1(x) ; f] there.  The sixteen lanes of one q read
//                 the same four pixels; lane i = 0 counts and checks them.
//       solve     thread 0, solve_star on LDS.
//       residual  (nclip > 0) a thread takes four consecutive pixels, eight neighbouring lanes OR their keep bits into one word
//                 of the mask in LDS (dynamic, ceil(n / 32) words) and one of them stores it: no atomics.
//       output    the same four pixels a thread: the status NONPOSITIVE, and flux / p and w p^2 where asked for.
//     <VEC>: 16-byte loads and stores (every leading dimension a multiple of four, every pointer aligned; a store only where its
//     four pixels are inside n); otherwise element by element, the same values in the same places.
//     The sums pass issues n / 4 matrix instructions a star on a (P + 1)^2 corner of the tile, and its sixteen lanes a q prepare the
//     same operands: measured at 13 - 19 % of the matrix instructions' floor, not waiting for memory (NOTES.md, 2026-10-20).
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "contfit_core.hpp"
#include "host_prologue.hpp"

namespace cf = payne::contfit;
namespace nt = payne::ntile;

namespace {

using nt::load4;
using payne::host::OnDevice;
using payne::host::aligned16;
using payne::host::fail;

struct Args {
  const float* flux;
  const double* w;
  long long ld_f;
  const float* model;
  long long ld_m;
  int n_models;
  const int* model_index;
  const double* x;
  int n;
  payne_contfit_opts o;
  double* coef;
  double* chisq;
  int* npix;
  int* status;
  int* rounds;
  float* flux_out;
  double* w_out;
  long long ld_o;
};

// The sum of v over the workgroup (integers: any order gives the same value).
__device__ inline long long block_sum(long long v, long long* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                                                  // (the readers of the call before are done with red)
  if ((threadIdx.x & (nt::kWave - 1)) == 0) red[threadIdx.x / nt::kWave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool VEC>
__global__ void __launch_bounds__(nt::kThreads) payne_contfit_kernel(const Args a) {
  extern __shared__ unsigned mask[];                                // cf::mask_words(n) words where nclip > 0
  __shared__ double part[nt::kWaves][nt::kTileSize];
  __shared__ double tile[nt::kTileSize];
  __shared__ double work[cf::kWorkDoubles];
  __shared__ double coef[cf::kMaxP + 1];
  __shared__ double chisq_s;
  __shared__ long long red[nt::kWaves];
  __shared__ int status_s;
  const size_t s = blockIdx.x;
  const int tid = threadIdx.x, i = tid & 15;
  const int n = a.n, P = a.o.P;
  const int mi = a.model_index ? a.model_index[s] : (int)s;
  const bool bad_model = mi < 0 || mi >= a.n_models;
  const float* fb = a.flux + s * (size_t)a.ld_f;
  const double* wb = a.w + s * (size_t)a.ld_f;
  const float* mb = a.model + (size_t)(bad_model ? 0 : mi) * (size_t)a.ld_m;   // (not read when bad_model)
  const int chunks = (n + cf::kChunk - 1) / cf::kChunk, sweeps = (chunks + nt::kThreads - 1) / nt::kThreads;
  int st = bad_model ? PAYNE_CONTFIT_BAD_MODEL : PAYNE_CONTFIT_OK, solves = 0, kept = 0;
  double chi = 0.0;
  bool masked = false;
  if (!bad_model) {
    const bool live = i <= P;
    for (int round = 0;; ++round) {
      // ---- sums
      long long seen = 0;                                           // counting pixels; bit 32 up: those that are not finite
      const nt::d4 acc = nt::wave_sums(n, [&](int p) PAYNE_TILE_CALLABLE {
        float f[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        double wv[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0};
        unsigned bits = 0u;
        if (p < n) {
          load4<VEC>(wb, p, n, true, wv);
          load4<VEC>(a.x, p, n, p + 3 < n, xv);
          if (live) {
            load4<VEC>(fb, p, n, true, f);
            load4<VEC>(mb, p, n, true, m);
          }
          bits = round > 0 ? (mask[p >> 5] >> (p & 31)) & 15u : 15u;
        }
        double T[4];
        cf::cheb4(live ? i : 0, P, xv, T);
        return [=, &seen](int t, double* r, double* wt) PAYNE_TILE_CALLABLE {
          const bool counts = p + t < n && wv[t] != 0.0;
          if (round == 0 && i == 0 && counts) seen += 1ll + (cf::pixel_finite(f[t], m[t], wv[t]) ? 0ll : 1ll << 32);
          *r = cf::row_from(live ? i : 0, P, m[t], f[t], T[t]);
          *wt = wv[t];
          return live && counts && ((bits >> t) & 1u);
        };
      });
      bool bad = false;
      nt::sum_waves(acc, part, tile, [&]() PAYNE_TILE_CALLABLE {
        if (round == 0) {
          const long long total = block_sum(seen, red);             // (its barriers publish part too)
          kept = (int)(total & 0xffffffffll);
          bad = (total >> 32) != 0;
        } else {
          __syncthreads();
        }
      });
      // ---- solve
      if (tid == 0) status_s = cf::solve_star(tile, P, kept, bad, work, coef, &chisq_s);
      __syncthreads();
      st = status_s;
      if (st != PAYNE_CONTFIT_OK) break;
      ++solves;
      chi = chisq_s;
      if (round == a.o.nclip) break;
      // ---- residuals: the new mask
      const double sc = cf::clip_scale(chi, kept, P, a.o.rescale), lo = a.o.kappa_lo * sc, hi = a.o.kappa_hi * sc;
      long long tally = 0;                                          // kept pixels; bit 32 up: threads whose four bits changed
      for (int k = 0; k < sweeps; ++k) {
        const int c = k * nt::kThreads + tid, p = cf::kChunk * c;
        unsigned nib = 0u, old = 0u;
        if (p < n) {
          float f[4], m[4];
          double wv[4], xv[4];
          load4<VEC>(wb, p, n, true, wv);
          load4<VEC>(a.x, p, n, p + 3 < n, xv);
          load4<VEC>(fb, p, n, true, f);
          load4<VEC>(mb, p, n, true, m);
          double pv[4];
          cf::poly4(coef, P, xv, pv);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const bool counts = p + t < n && wv[t] != 0.0;
            const bool keep = counts && cf::keeps(f[t], m[t], wv[t], pv[t], lo, hi);
            nib |= (keep ? 1u : 0u) << t;
            old |= (counts ? 1u : 0u) << t;
          }
          if (masked) old = (mask[c >> 3] >> (4 * (c & 7))) & 15u;
        }
        unsigned word = nib << (4 * (c & 7));                       // (c & 7 == lane & 7: eight neighbouring lanes, one word)
        word |= __shfl_xor(word, 1);
        word |= __shfl_xor(word, 2);
        word |= __shfl_xor(word, 4);
        if ((c & 7) == 0 && p < n) mask[c >> 3] = word;
        tally += (long long)__popc(nib) + (old != nib ? 1ll << 32 : 0ll);
      }
      const long long total = block_sum(tally, red);                // (its barriers publish the mask)
      masked = true;
      if ((total >> 32) == 0) break;
      kept = (int)(total & 0xffffffffll);
    }
  }
  // ---- output
  const bool fail = cf::failed(st);
  float* fo_row = a.flux_out ? a.flux_out + s * (size_t)a.ld_o : nullptr;
  double* wo_row = a.w_out ? a.w_out + s * (size_t)a.ld_o : nullptr;
  const bool rows = fo_row || wo_row;
  long long nonpos = 0;
  if (!fail || rows) {
    for (int k = 0; k < sweeps; ++k) {
      const int c = k * nt::kThreads + tid, p = cf::kChunk * c;
      if (p >= n) continue;
      float f[4] = {0.0f, 0.0f, 0.0f, 0.0f}, fo[4];
      double wv[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0}, wo[4];
      if (rows) load4<VEC>(fb, p, n, true, f);
      if (!fail) {
        load4<VEC>(wb, p, n, true, wv);
        load4<VEC>(a.x, p, n, p + 3 < n, xv);
      }
      const unsigned bits = masked && a.o.drop_clipped ? (mask[c >> 3] >> (4 * (c & 7))) & 15u : 15u;
      double pv[4] = {0.0, 0.0, 0.0, 0.0};
      if (!fail) cf::poly4(coef, P, xv, pv);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fo[t] = f[t];
        wo[t] = 0.0;
        if (!fail && p + t < n && cf::out_pixel(f[t], wv[t], pv[t], wv[t] != 0.0, !((bits >> t) & 1u), &fo[t], &wo[t]))
          nonpos = 1;
      }
      if (VEC && p + 3 < n) {
        if (fo_row) *reinterpret_cast<float4*>(fo_row + p) = make_float4(fo[0], fo[1], fo[2], fo[3]);
        if (wo_row) {
          *reinterpret_cast<double2*>(wo_row + p) = make_double2(wo[0], wo[1]);
          *reinterpret_cast<double2*>(wo_row + p + 2) = make_double2(wo[2], wo[3]);
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (p + t < n) {
            if (fo_row) fo_row[p + t] = fo[t];
            if (wo_row) wo_row[p + t] = wo[t];
          }
      }
    }
  }
  if (!fail && block_sum(nonpos, red) != 0) st = PAYNE_CONTFIT_NONPOSITIVE;   // (fail is the whole workgroup's)
  if (tid < P) a.coef[s * (size_t)P + (size_t)tid] = fail ? (double)NAN : coef[tid];
  if (tid == 0) {
    a.chisq[s] = fail ? (double)NAN : chi;
    a.npix[s] = kept;
    a.status[s] = st;
    a.rounds[s] = solves;
  }
}

}  // namespace

extern "C" int payne_contfit_batch(int device, const float* flux_dev, const double* w_dev, long long ld_f, const float* model_dev,
                                   long long ld_m, int n_models, const int* model_index_dev, const double* x_dev, int N, int n,
                                   const payne_contfit_opts* opts, double* coef_dev, double* chisq_dev, int* npix_dev, int* status_dev,
                                   int* rounds_dev, float* flux_out_dev, double* w_out_dev, long long ld_o, void* stream) {
  if (!opts || !cf::opts_ok(*opts)) return fail(PAYNE_E_INVALID, "payne_contfit_batch: null opts, P outside 1..15, nclip outside 0..16 or a kappa that is not positive");
  if (N < 0 || n < 1 || ld_f < n || ld_m < n || n_models < 1) return fail(PAYNE_E_INVALID, "payne_contfit_batch: N < 0, n < 1, ld_f < n, ld_m < n or n_models < 1");
  if (!model_index_dev && n_models < N) return fail(PAYNE_E_INVALID, "payne_contfit_batch: n_models < N without model_index_dev");
  if ((flux_out_dev || w_out_dev) && ld_o < n) return fail(PAYNE_E_INVALID, "payne_contfit_batch: ld_o < n");
  if (N > 0 && (!flux_dev || !w_dev || !model_dev || !x_dev || !coef_dev || !chisq_dev || !npix_dev || !status_dev || !rounds_dev))
    return fail(PAYNE_E_INVALID, "payne_contfit_batch: a null device pointer");
  if (n > cf::kMaxN) return fail(PAYNE_E_UNSUPPORTED, "payne_contfit_batch: n > 262144 (the clipping mask is a bit set in LDS)");
  if (N == 0) return PAYNE_OK;
  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_contfit_batch: hipSetDevice");
  const Args a{flux_dev, w_dev, ld_f, model_dev, ld_m, n_models, model_index_dev, x_dev, n, *opts, coef_dev, chisq_dev, npix_dev, status_dev,
               rounds_dev, flux_out_dev, w_out_dev, ld_o};
  const bool rows = flux_out_dev || w_out_dev;
  const bool vec = ld_f % 4 == 0 && ld_m % 4 == 0 && aligned16(flux_dev) && aligned16(w_dev) && aligned16(model_dev) && aligned16(x_dev) &&
                   (!rows || (ld_o % 4 == 0 && aligned16(flux_out_dev) && aligned16(w_out_dev)));
  const size_t lds = opts->nclip > 0 ? (size_t)cf::mask_words(n) * sizeof(unsigned) : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(payne_contfit_kernel<true>, dim3((unsigned)N), dim3(nt::kThreads), lds, st, a);
  else
    hipLaunchKernelGGL(payne_contfit_kernel<false>, dim3((unsigned)N), dim3(nt::kThreads), lds, st, a);
  return hipGetLastError() == hipSuccess ? PAYNE_OK : fail(PAYNE_E_HIP, "payne_contfit_batch: the launch failed");
}
