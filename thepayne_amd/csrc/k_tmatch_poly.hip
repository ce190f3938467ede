// k_tmatch_poly.hip -- payne_tmatch_create_poly, payne_tmatch_match_poly: the template search with a free Chebyshev series of P <= 8
// coefficients per (star, template) pair (include/payne_hip.h).  The arithmetic, its order and the rules are tmatch_poly_core.hpp, which
// runs on the host too (tests/emul/tmatch_poly_emul.cpp); the steps, the staging maps and the lists are tmatch_core.hpp's.
//
//   payne_tmatch_poly_tile_kernel<P>   grid (star tiles, template chunks), 256 threads; one instantiation per P.  A workgroup owns
//     16 stars x 64 templates and walks the pixels in steps of 32.  Every thread stages 2 star pixels -- (flux, w, x) of the NEXT
//     step wait in registers -- as the star's 3 P - 1 operands a1 T_j, a2 T_q (fp64 [3 P - 1][16][34] in LDS) and 8 template values
//     (fp32 [64][36]); the staging thread carries its stars' c0 partial sums and counts of counting pixels.  Wave v owns templates
//     16 v .. 16 v + 15 against the 16 stars: 3 P - 1 accumulator tiles of v_mfma_f64_16x16x4_f64 (4 (3 P - 1) <= 92 fp64 registers a
//     lane); per group of four pixels it reads one template value and 3 P - 1 star operands a lane and issues 3 P - 1 matrix
//     instructions.  A step in which some template value is not finite takes tmatch's side path that marks the pairs it poisons.
//     Behind the pixels the stage is dead and the LDS holds: a solve area per solver (the pair's sums, then scaled_solve's work, at an
//     odd pitch), the coefficient tile [16][64][P] and chi^2 [16][65].  solvers_of(P) of the 256 threads solve at a time -- register
//     reg = 0 .. 3 of the accumulators by 256 / solvers_of(P) parts of each wave's lanes; the lanes that share an area take turns,
//     a barrier between the parts.  Then the optional N x M output in rows, and a thread a star
//     inserts the chunk's 64 values into its list, which goes to the workspace with the listed pairs' coefficients.
//   payne_tmatch_poly_merge_kernel     32 stars a workgroup: a thread a star walks its chunks' lists in chunk order and writes idx,
//     chisq; then a thread an entry copies the coefficients and walks the star's pixels for the flags.
//   No atomics; every sum and every list has one fixed order.  Nothing is contracted into a fused multiply-add that the source does
//   not write as one, so the host's bytes are the device's.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "host_prologue.hpp"
#include "normal_tile.hpp"
#include "tmatch_core.hpp"
#include "tmatch_handle.hpp"
#include "tmatch_poly_core.hpp"

namespace tq = payne::tmatch;
namespace tp = payne::tmatch_poly;

namespace {

using payne::ntile::d4;
using payne::host::OnDevice;
using payne::host::fail;

constexpr int stage_bytes(int P) { return tp::ops_of(P) * tp::kStars * tq::kPitchA * 8 + tp::kChunk * tq::kPitchT * 4; }
constexpr int solve_bytes(int P) { return tp::solvers_of(P) * tp::area_doubles(P) * 8; }
constexpr int coef_bytes(int P) { return tp::kStars * tp::kChunk * P * 8; }
constexpr int kChiBytes = tp::kStars * tp::kPitchChi * 8;
constexpr int behind_bytes(int P) { return solve_bytes(P) + coef_bytes(P) + kChiBytes; }
constexpr int union_bytes(int P) { return behind_bytes(P) > stage_bytes(P) ? behind_bytes(P) : stage_bytes(P); }
static_assert(union_bytes(tp::kMaxPoly) + 4096 <= 160 * 1024, "the stage and what follows it share 160 KB of LDS");
static_assert(tp::kStars * tq::kStep * 12 <= stage_bytes(1), "the c0 partial sums and the counts share the stage");

template <int P>
__global__ void __launch_bounds__(tq::kThreads) payne_tmatch_poly_tile_kernel(const float* __restrict__ templ, long long ld_t, int M,
                                                                              const float* __restrict__ flux, const double* __restrict__ w,
                                                                              long long ld_f, int N, int n, const double* __restrict__ x, int topk,
                                                                              double* __restrict__ part_c, int* __restrict__ part_i,
                                                                              double* __restrict__ part_coef, double* __restrict__ all, long long ld_a) {
  constexpr int kOps = tp::ops_of(P), kArea = tp::area_doubles(P);
  __shared__ __attribute__((aligned(16))) unsigned char raw[union_bytes(P)];
  __shared__ double c0s[tp::kStars];
  __shared__ int cnts[tp::kStars];
  __shared__ double lc[tp::kStars * tq::kMaxTopk];
  __shared__ int li[tp::kStars * tq::kMaxTopk];
  __shared__ int nf_step;                                           // 1 + the last step that staged a template value that is not finite
  double* As = reinterpret_cast<double*>(raw);                      // [kOps][16][kPitchA]
  float* Ts = reinterpret_cast<float*>(raw + kOps * tp::kStars * tq::kPitchA * 8);
  double* c0p = reinterpret_cast<double*>(raw);                     // behind the pixel loop: [16][32], and the counts [16][32]
  int* cntp = reinterpret_cast<int*>(raw + tp::kStars * tq::kStep * 8);
  double* areas = reinterpret_cast<double*>(raw);                   // behind c0: [solvers][kArea]
  double* coefs = reinterpret_cast<double*>(raw + solve_bytes(P));  // [16][64][P]
  double* chi = reinterpret_cast<double*>(raw + solve_bytes(P) + coef_bytes(P));   // [16][65]

  const int tid = threadIdx.x, lane = tid & (tq::kWave - 1), wave = tid / tq::kWave;
  const int i = lane & 15, k = lane >> 4;
  const int s0 = blockIdx.x * tp::kStars, t0 = blockIdx.y * tp::kChunk;
  const int pp = tq::stage_pixel(tid);
  if (tid == 0) nf_step = 0;

  float fr[tp::kStarRegs], mr[tp::kTemplRegs];
  double wr[tp::kStarRegs], c0acc[tp::kStarRegs], xr = 0.0;
  int cntacc[tp::kStarRegs];
  d4 acc[kOps];
#pragma unroll
  for (int op = 0; op < kOps; ++op) acc[op] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < tp::kStarRegs; ++r) {
    c0acc[r] = 0.0;
    cntacc[r] = 0;
  }
  unsigned poison = 0u;

  auto load_step = [&](int step) {
    const int p = tq::kStep * step + pp;
    xr = p < n ? x[p] : 0.0;
#pragma unroll
    for (int r = 0; r < tp::kStarRegs; ++r) {
      const int s = s0 + tq::stage_row(tid, r);
      const bool inside = s < N && p < n;
      fr[r] = inside ? flux[(size_t)s * (size_t)ld_f + p] : 0.0f;
      wr[r] = inside ? w[(size_t)s * (size_t)ld_f + p] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < tp::kTemplRegs; ++r) {
      const int t = t0 + tq::stage_row(tid, r);
      mr[r] = (t < M && p < n) ? templ[(size_t)t * (size_t)ld_t + p] : 0.0f;
    }
  };

  const int steps = tq::steps_of(n);
  load_step(0);
  __syncthreads();                                                  // nf_step = 0 is seen
  for (int step = 0; step < steps; ++step) {
    bool bad = false;
#pragma unroll
    for (int r = 0; r < tp::kStarRegs; ++r) {
      double a1, a2, fz;
      tq::star_operands(fr[r], wr[r], true, &a1, &a2, &fz);        // (outside the call: f = 0, w = 0 from load_step)
      const bool counts = tp::pixel_counts(wr[r], true);
      tp::star_basis(a1, a2, counts, counts ? xr : 0.0, P, As + tq::stage_row(tid, r) * tq::kPitchA + pp, tp::kStars * tq::kPitchA);
      c0acc[r] = tq::c0_add(a1, fz, c0acc[r]);
      cntacc[r] += counts ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < tp::kTemplRegs; ++r) {
      Ts[tq::stage_row(tid, r) * tq::kPitchT + pp] = mr[r];
      bad = bad || !tq::finite32(mr[r]);
    }
    if (bad) nf_step = step + 1;                                    // (every writer of a step writes the same value)
    __syncthreads();
    if (step + 1 < steps) load_step(step + 1);                      // in flight under the matrix instructions
    if (nf_step == step + 1) {
      for (int p = 0; p < tq::kStep; ++p)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)                           // (operand P is a2 T_0 = a2: the staged weight)
          if (tq::pair_poisoned(As[(P * tp::kStars + tp::acc_star(reg, lane)) * tq::kPitchA + p], Ts[tp::acc_template(wave, lane) * tq::kPitchT + p]))
            poison |= 1u << reg;
    }
    const int groups = tq::groups_in_step(n, step);
    for (int g = 0; g < groups; ++g) {
      const int px = tq::kGroup * g + k;
      double b1, b2;
      tp::template_operands(Ts[(16 * wave + i) * tq::kPitchT + px], &b1, &b2);
#pragma unroll
      for (int op = 0; op < kOps; ++op)
        acc[op] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(op * tp::kStars + i) * tq::kPitchA + px], op < P ? b1 : b2, acc[op], 0, 0, 0);
    }
    __syncthreads();
  }

  // c0 and the count: the staging threads' partial sums, then j = 0 .. 31 in order
#pragma unroll
  for (int r = 0; r < tp::kStarRegs; ++r) {
    c0p[tq::stage_row(tid, r) * tq::kStep + pp] = c0acc[r];
    cntp[tq::stage_row(tid, r) * tq::kStep + pp] = cntacc[r];
  }
  __syncthreads();
  if (tid < tp::kStars) {
    double c0 = 0.0;
    int cnt = 0;
    for (int j = 0; j < tq::kStep; ++j) {
      c0 += c0p[tid * tq::kStep + j];
      cnt += cntp[tid * tq::kStep + j];
    }
    c0s[tid] = c0;
    cnts[tid] = cnt;
  }
  __syncthreads();

  // the pairs: solvers_of(P) at a time
  constexpr int kParts = tq::kThreads / tp::solvers_of(P), kLanesOn = tq::kWave / kParts;
  double* area = areas + (wave * kLanesOn + lane % kLanesOn) * kArea;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
    for (int part = 0; part < kParts; ++part) {
      if (kParts > 1) __syncthreads();                              // (the parts stay apart: the lanes that share an area take turns)
      if (lane / kLanesOn == part) {
#pragma unroll
        for (int op = 0; op < kOps; ++op) area[op] = acc[op][reg];
        const int sr = tp::acc_star(reg, lane), tc = tp::acc_template(wave, lane);
        chi[sr * tp::kPitchChi + tc] =
            tp::pair_solve(area, 1, P, c0s[sr], cnts[sr], ((poison >> reg) & 1u) != 0u, area + kOps, coefs + (sr * tp::kChunk + tc) * P, 1);
      }
    }
  __syncthreads();
  const int count = M - t0 < tp::kChunk ? M - t0 : tp::kChunk;
  if (all) {
    for (int e = tid; e < tp::kStars * tp::kChunk; e += tq::kThreads) {
      const int sr = e / tp::kChunk, tr = e % tp::kChunk;
      if (s0 + sr < N && tr < count) all[(size_t)(s0 + sr) * (size_t)ld_a + (size_t)(t0 + tr)] = chi[sr * tp::kPitchChi + tr];
    }
  }
  if (tid < tp::kStars && s0 + tid < N) {
    double* c = lc + tid * tq::kMaxTopk;
    int* ix = li + tid * tq::kMaxTopk;
    tq::list_from_chunk(c, ix, topk, chi + tid * tp::kPitchChi, t0, count);
    const size_t at = tq::part_at((int)blockIdx.y, N, s0 + tid, topk);
    for (int j = 0; j < topk; ++j) {
      part_c[at + j] = c[j];
      part_i[at + j] = ix[j];
      if (ix[j] >= 0)
        for (int q = 0; q < P; ++q) part_coef[(at + j) * P + q] = coefs[(tid * tp::kChunk + (ix[j] - t0)) * P + q];
    }
  }
}

__global__ void __launch_bounds__(tq::kThreads) payne_tmatch_poly_merge_kernel(const double* __restrict__ part_c, const int* __restrict__ part_i,
                                                                               const double* __restrict__ part_coef, int chunks, int N, int topk,
                                                                               int P, const double* __restrict__ w, long long ld_f,
                                                                               const double* __restrict__ x, int n, int* __restrict__ idx,
                                                                               double* __restrict__ chisq, double* __restrict__ coef,
                                                                               int* __restrict__ flags) {
  __shared__ double lc[tp::kMergeStars * tq::kMaxTopk];
  __shared__ int li[tp::kMergeStars * tq::kMaxTopk];
  __shared__ int ls[tp::kMergeStars * tq::kMaxTopk];
  const int tid = threadIdx.x;
  if (tid < tp::kMergeStars) {
    const int s = blockIdx.x * tp::kMergeStars + tid;
    if (s < N) {
      double* c = lc + tid * tq::kMaxTopk;
      int* ix = li + tid * tq::kMaxTopk;
      tp::merge_chunks_from(c, ix, ls + tid * tq::kMaxTopk, topk, part_c, part_i, chunks, N, s);
      for (int j = 0; j < topk; ++j) {
        chisq[(size_t)s * topk + j] = c[j];
        idx[(size_t)s * topk + j] = ix[j];
      }
    }
  }
  __syncthreads();
  const int sl = tid / tq::kMaxTopk, j = tid % tq::kMaxTopk;
  const int s = blockIdx.x * tp::kMergeStars + sl;
  if (s < N && j < topk)
    flags[(size_t)s * topk + j] = tp::finish_entry(ls[sl * tq::kMaxTopk + j], part_coef, N, s, topk, P, w + (size_t)s * (size_t)ld_f, x, n,
                                                   coef + ((size_t)s * topk + j) * P);
}
static_assert(tp::kMergeStars * tq::kMaxTopk == tq::kThreads, "a thread an entry");

struct Launch {
  const float *templ, *flux;
  const double *w, *x;
  long long ld_t, ld_f, ld_a;
  int M, N, n, topk;
  double *part_c, *part_coef, *all;
  int* part_i;
};

template <int P>
void launch_tile(const Launch& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(payne_tmatch_poly_tile_kernel<P>, grid, dim3(tq::kThreads), 0, st, a.templ, a.ld_t, a.M, a.flux, a.w, a.ld_f, a.N, a.n, a.x, a.topk,
                     a.part_c, a.part_i, a.part_coef, a.all, a.ld_a);
}

}  // namespace

extern "C" int payne_tmatch_poly_stars(void) { return tp::kStars; }
extern "C" int payne_tmatch_poly_chunk(void) { return tp::kChunk; }

extern "C" int payne_tmatch_create_poly(int device, int max_stars, int max_templates, int max_poly, payne_tmatch** out) {
  if (!out) return fail(PAYNE_E_INVALID, "payne_tmatch_create_poly: null handle pointer");
  *out = nullptr;
  if (max_poly < 1 || max_poly > tp::kMaxPoly) return fail(PAYNE_E_INVALID, "payne_tmatch_create_poly: max_poly outside 1 .. 8");
  payne_tmatch* h = nullptr;
  const int rc = payne_tmatch_create(device, max_stars, max_templates, &h);
  if (rc != PAYNE_OK) return rc;
  OnDevice on(device);
  const size_t entries = (size_t)tp::chunks_of(max_templates) * (size_t)max_stars * (size_t)tq::kMaxTopk;
  void *pc = nullptr, *pi = nullptr, *pk = nullptr;
  if (!on.ok() || hipMalloc(&pc, entries * sizeof(double)) != hipSuccess || hipMalloc(&pi, entries * sizeof(int)) != hipSuccess ||
      hipMalloc(&pk, entries * (size_t)max_poly * sizeof(double)) != hipSuccess) {
    if (pc) (void)hipFree(pc);
    if (pi) (void)hipFree(pi);
    payne_tmatch_destroy(h);
    return fail(PAYNE_E_HIP, "payne_tmatch_create_poly: allocating the workspace failed");
  }
  h->max_poly = max_poly;
  h->poly_c = static_cast<double*>(pc);
  h->poly_i = static_cast<int*>(pi);
  h->poly_coef = static_cast<double*>(pk);
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_tmatch_match_poly(payne_tmatch* h, const float* templates_dev, int ld_t, int M, const float* flux_dev, const double* w_dev,
                                       int ld_f, int N, int n, const double* x_dev, int P, int topk, int* idx_dev, double* chisq_dev,
                                       double* coef_dev, int* flags_dev, double* all_dev, long long ld_a, void* stream) {
  if (!h) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: null handle");
  if (P < 1 || P > h->max_poly) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: P outside 1 .. the handle's max_poly");
  if (topk < 1 || topk > tq::kMaxTopk) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: topk outside 1 .. 8");
  if (N < 0 || N > h->max_stars) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: N outside 0 .. max_stars");
  if (M < 0 || M > h->max_templates) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: M outside 0 .. max_templates");
  if (n < 1 || ld_t < n || ld_f < n) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: n < 1, ld_t < n or ld_f < n");
  if (N == 0 || M == 0) return PAYNE_OK;
  if (!templates_dev || !flux_dev || !w_dev || !x_dev || !idx_dev || !chisq_dev || !coef_dev || !flags_dev)
    return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: null pointer");
  if (all_dev && ld_a < (long long)M) return fail(PAYNE_E_INVALID, "payne_tmatch_match_poly: ld_a < M");
  OnDevice on(h->device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_tmatch_match_poly: hipSetDevice");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int chunks = tp::chunks_of(M), tiles = tp::tiles_of(N);
  if (chunks > 65535) return fail(PAYNE_E_UNSUPPORTED, "payne_tmatch_match_poly: more than 65535 chunks of templates");
  const Launch a = {templates_dev, flux_dev, w_dev, x_dev, (long long)ld_t, (long long)ld_f, ld_a, M, N, n, topk, h->poly_c, h->poly_coef, all_dev, h->poly_i};
  const dim3 grid((unsigned)tiles, (unsigned)chunks);
  switch (P) {
    case 1: launch_tile<1>(a, grid, st); break;
    case 2: launch_tile<2>(a, grid, st); break;
    case 3: launch_tile<3>(a, grid, st); break;
    case 4: launch_tile<4>(a, grid, st); break;
    case 5: launch_tile<5>(a, grid, st); break;
    case 6: launch_tile<6>(a, grid, st); break;
    case 7: launch_tile<7>(a, grid, st); break;
    default: launch_tile<8>(a, grid, st); break;
  }
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match_poly: launching the tile kernel failed");
  hipLaunchKernelGGL(payne_tmatch_poly_merge_kernel, dim3((unsigned)((N + tp::kMergeStars - 1) / tp::kMergeStars)), dim3(tq::kThreads), 0, st, h->poly_c,
                     h->poly_i, h->poly_coef, chunks, N, topk, P, w_dev, (long long)ld_f, x_dev, n, idx_dev, chisq_dev, coef_dev, flags_dev);
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match_poly: launching the merge kernel failed");
  return PAYNE_OK;
}
