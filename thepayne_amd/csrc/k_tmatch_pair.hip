// k_tmatch_pair.hip -- payne_tmatch_create_pairs, payne_tmatch_match_pairs: the template search against pairs of templates with both
// amplitudes free (include/payne_hip.h).  The arithmetic, its order and the rules are tmatch_pair_core.hpp, which runs on the host too
// (tests/emul/tmatch_pair_emul.cpp); the steps, the staging maps, the LDS pitches and the lists are tmatch_core.hpp's.
//
//   payne_tmatch_pair_moments_kernel  grid (star tiles, template chunks), 256 threads: k_tmatch.hip's tile loop (64 stars x 128
//     templates, steps of 32 pixels, the next step's values in registers under the current step's matrix instructions) with the
//     template operands m and m^2 and an accumulator tile each for B = sum a1 m and S = sum a2 m^2 (128 accumulator registers a
//     lane).  The moments leave the registers for the workspace directly, 16 consecutive templates a store; a poisoned (star,
//     template) leaves NaN in both.  The workgroups of chunk 0 write c0.
//   payne_tmatch_pair_cross_kernel    grid (row tiles, template chunks), 256 threads: the same loop over 64 rows (star, primary) x 128
//     templates.  The A side is gathered: a thread stages w of its rows' stars and the rows' primaries and writes their product, one
//     fp64 tile [64][34]; one matrix instruction per 16 x 16 tile and group, 32 fp64 accumulators a lane.  Sa, Ba, c0, the primary and
//     the star's earlier primaries wait per row in LDS from the start.  Behind the pixels every lane solves its 32 pairs (Sb, Bb from
//     the workspace, 16 consecutive templates a load) into the chi^2 tile [64][129]; the optional output leaves from there in rows;
//     a thread a row inserts the chunk's 128 values into its list, which goes to the workspace; then the lane that holds a listed
//     pair's X solves it once more and writes its amplitudes beside the entry (pair_solve is a function of its arguments, so these
//     are the bytes of the first solve).
//   payne_tmatch_pair_merge_kernel    a thread a star walks its rows in j order and their chunks in chunk order (lists in LDS), then a
//     thread an entry copies the primary's index and the amplitudes.
//   No atomics; every sum and every list has one fixed order.  Nothing is contracted into a fused multiply-add that the source does
//   not write as one, so the host's bytes are the device's.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "host_prologue.hpp"
#include "normal_tile.hpp"
#include "tmatch_core.hpp"
#include "tmatch_handle.hpp"
#include "tmatch_pair_core.hpp"

namespace tq = payne::tmatch;
namespace tr = payne::tmatch_pair;

namespace {

using payne::ntile::d4;
using payne::host::OnDevice;
using payne::host::fail;

constexpr int kMomentStageBytes = 2 * tq::kStars * tq::kPitchA * 8 + tq::kChunk * tq::kPitchT * 4;   // a1, a2, the templates
static_assert(tq::kStars * tq::kStep * 8 <= kMomentStageBytes, "the c0 partial sums share the stage");
constexpr int kCrossStageBytes = tr::kRows * tq::kPitchA * 8 + tq::kChunk * tq::kPitchT * 4;         // g, the templates
constexpr int kChiBytes = tr::kRows * tq::kPitchChi * 8;
constexpr int kCrossUnionBytes = kChiBytes > kCrossStageBytes ? kChiBytes : kCrossStageBytes;
constexpr int kMergeStars = 32;                     // stars of one workgroup of the merge launch: a thread an entry afterwards
static_assert(kMergeStars * tq::kMaxTopk == tq::kThreads, "a thread an entry");

__global__ void __launch_bounds__(tq::kThreads) payne_tmatch_pair_moments_kernel(const float* __restrict__ templ, long long ld_t, int M,
                                                                                 const float* __restrict__ flux, const double* __restrict__ w,
                                                                                 long long ld_f, int N, int n, double* __restrict__ Bw,
                                                                                 double* __restrict__ Sw, double* __restrict__ c0w) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[kMomentStageBytes];
  __shared__ int nf_step;                                           // 1 + the last step that staged a template value that is not finite
  double* As1 = reinterpret_cast<double*>(raw);
  double* As2 = As1 + tq::kStars * tq::kPitchA;
  float* Ts = reinterpret_cast<float*>(raw + 2 * tq::kStars * tq::kPitchA * 8);
  double* c0p = reinterpret_cast<double*>(raw);                     // behind the pixel loop: [64][32]

  const int tid = threadIdx.x, lane = tid & (tq::kWave - 1), wave = tid / tq::kWave;
  const int i = lane & 15, k = lane >> 4;
  const int s0 = blockIdx.x * tq::kStars, t0 = blockIdx.y * tq::kChunk;
  const int pp = tq::stage_pixel(tid);
  if (tid == 0) nf_step = 0;

  float fr[tq::kStarRegs], mr[tq::kTemplRegs];
  double wr[tq::kStarRegs], c0acc[tq::kStarRegs];
  d4 accB[4][2], accS[4][2];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      accB[rb][cb] = d4{0.0, 0.0, 0.0, 0.0};
      accS[rb][cb] = d4{0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll
  for (int r = 0; r < tq::kStarRegs; ++r) c0acc[r] = 0.0;
  unsigned poison = 0u;

  auto load_step = [&](int step) {
    const int p = tq::kStep * step + pp;
#pragma unroll
    for (int r = 0; r < tq::kStarRegs; ++r) {
      const int s = s0 + tq::stage_row(tid, r);
      const bool inside = s < N && p < n;
      fr[r] = inside ? flux[(size_t)s * (size_t)ld_f + p] : 0.0f;
      wr[r] = inside ? w[(size_t)s * (size_t)ld_f + p] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < tq::kTemplRegs; ++r) {
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
    for (int r = 0; r < tq::kStarRegs; ++r) {
      double a1, a2, fz;
      tq::star_operands(fr[r], wr[r], true, &a1, &a2, &fz);        // (outside the call: f = 0, w = 0 from load_step)
      const int at = tq::stage_row(tid, r) * tq::kPitchA + pp;
      As1[at] = a1;
      As2[at] = a2;
      c0acc[r] = tq::c0_add(a1, fz, c0acc[r]);
    }
#pragma unroll
    for (int r = 0; r < tq::kTemplRegs; ++r) {
      Ts[tq::stage_row(tid, r) * tq::kPitchT + pp] = mr[r];
      bad = bad || !tq::finite32(mr[r]);
    }
    if (bad) nf_step = step + 1;                                    // (every writer of a step writes the same value)
    __syncthreads();
    if (step + 1 < steps) load_step(step + 1);                      // in flight under the matrix instructions
    if (nf_step == step + 1) {
      for (int p = 0; p < tq::kStep; ++p)
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
              if (tq::pair_poisoned(As2[tq::acc_star(rb, reg, lane) * tq::kPitchA + p], Ts[tq::acc_template(wave, cb, lane) * tq::kPitchT + p]))
                poison |= 1u << tq::acc_bit(rb, cb, reg);
    }
    const int groups = tq::groups_in_step(n, step);
    for (int g = 0; g < groups; ++g) {
      const int px = tq::kGroup * g + k;
      double b1[2], b2[2], A1[4], A2[4];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        b1[cb] = tr::template_value(Ts[(32 * wave + 16 * cb + i) * tq::kPitchT + px]);
        b2[cb] = b1[cb] * b1[cb];
      }
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        A1[rb] = As1[(16 * rb + i) * tq::kPitchA + px];
        A2[rb] = As2[(16 * rb + i) * tq::kPitchA + px];
      }
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) accB[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1[rb], b1[cb], accB[rb][cb], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) accS[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(A2[rb], b2[cb], accS[rb][cb], 0, 0, 0);
    }
    __syncthreads();
  }

  // the moments, from the registers: lanes i = 0 .. 15 of one store are consecutive templates of one star
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int s = s0 + tq::acc_star(rb, reg, lane), t = t0 + tq::acc_template(wave, cb, lane);
        if (s < N && t < M) {
          const bool poisoned = ((poison >> tq::acc_bit(rb, cb, reg)) & 1u) != 0u;
          Bw[tr::moment_at(s, M, t)] = poisoned ? __builtin_nan("") : accB[rb][cb][reg];
          Sw[tr::moment_at(s, M, t)] = poisoned ? __builtin_nan("") : accS[rb][cb][reg];
        }
      }
  // c0: the staging threads' partial sums, then j = 0 .. 31 in order; chunk 0's workgroups write it
  if (blockIdx.y != 0) return;
#pragma unroll
  for (int r = 0; r < tq::kStarRegs; ++r) c0p[tq::stage_row(tid, r) * tq::kStep + pp] = c0acc[r];
  __syncthreads();
  if (tid < tq::kStars && s0 + tid < N) {
    double c0 = 0.0;
    for (int j = 0; j < tq::kStep; ++j) c0 += c0p[tid * tq::kStep + j];
    c0w[s0 + tid] = c0;
  }
}

__global__ void __launch_bounds__(tq::kThreads) payne_tmatch_pair_cross_kernel(const float* __restrict__ templ, long long ld_t, int M,
                                                                               const double* __restrict__ w, long long ld_f, int N, int n,
                                                                               const int* __restrict__ cand, int kA, int topk,
                                                                               const double* __restrict__ Bw, const double* __restrict__ Sw,
                                                                               const double* __restrict__ c0w, double* __restrict__ part_c,
                                                                               int* __restrict__ part_i, double* __restrict__ part_amp,
                                                                               double* __restrict__ all, long long ld_a) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[kCrossUnionBytes];
  __shared__ double rSa[tr::kRows], rBa[tr::kRows], rc0[tr::kRows];
  __shared__ int rstar[tr::kRows], rslot[tr::kRows], rcand[tr::kRows];        // the row's star (-1: beyond the call), slot and primary
  __shared__ int rprev[tr::kRows * tr::kMaxPrimaries];                          // the star's primaries of the slots before the row's
  __shared__ double lc[tr::kRows * tq::kMaxTopk];
  __shared__ int li[tr::kRows * tq::kMaxTopk];
  double* Gs = reinterpret_cast<double*>(raw);                      // [64][34]
  float* Ts = reinterpret_cast<float*>(raw + tr::kRows * tq::kPitchA * 8);
  double* chi = reinterpret_cast<double*>(raw);                     // behind the pixel loop: [64][129]

  const int tid = threadIdx.x, lane = tid & (tq::kWave - 1), wave = tid / tq::kWave;
  const int i = lane & 15, k = lane >> 4;
  const int R = N * kA, r0 = blockIdx.x * tr::kRows, t0 = blockIdx.y * tq::kChunk;
  const int pp = tq::stage_pixel(tid);

  if (tid < tr::kRows) {
    const int row = r0 + tid;
    int s = -1, j = 0, a = -1;
    double Sa = __builtin_nan(""), Ba = __builtin_nan(""), c0 = __builtin_nan("");
    if (row < R) {
      s = tr::row_star(row, kA);
      j = tr::row_slot(row, kA);
      a = cand[row];
      c0 = c0w[s];
      if (tr::cand_valid(a, M)) {
        Sa = Sw[tr::moment_at(s, M, a)];
        Ba = Bw[tr::moment_at(s, M, a)];
      }
      for (int e = 0; e < j; ++e) rprev[tid * tr::kMaxPrimaries + e] = cand[tr::row_of(s, e, kA)];
    }
    rstar[tid] = s;
    rslot[tid] = j;
    rcand[tid] = a;
    rSa[tid] = Sa;
    rBa[tid] = Ba;
    rc0[tid] = c0;
  }
  __syncthreads();

  int srow[tq::kStarRegs], arow[tq::kStarRegs];                     // of the rows this thread stages: the star and the primary, or -1
#pragma unroll
  for (int r = 0; r < tq::kStarRegs; ++r) {
    const int rr = tq::stage_row(tid, r);
    srow[r] = rstar[rr];
    arow[r] = (rstar[rr] >= 0 && tr::cand_valid(rcand[rr], M)) ? rcand[rr] : -1;
  }
  float gr[tq::kStarRegs], mr[tq::kTemplRegs];
  double wr[tq::kStarRegs];
  d4 acc[4][2];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = d4{0.0, 0.0, 0.0, 0.0};

  auto load_step = [&](int step) {
    const int p = tq::kStep * step + pp;
#pragma unroll
    for (int r = 0; r < tq::kStarRegs; ++r) {
      const bool inside = arow[r] >= 0 && p < n;
      wr[r] = inside ? w[(size_t)srow[r] * (size_t)ld_f + p] : 0.0;
      gr[r] = inside ? templ[(size_t)arow[r] * (size_t)ld_t + p] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < tq::kTemplRegs; ++r) {
      const int t = t0 + tq::stage_row(tid, r);
      mr[r] = (t < M && p < n) ? templ[(size_t)t * (size_t)ld_t + p] : 0.0f;
    }
  };

  const int steps = tq::steps_of(n);
  load_step(0);
  for (int step = 0; step < steps; ++step) {
#pragma unroll
    for (int r = 0; r < tq::kStarRegs; ++r) {
      double a1, a2, fz;
      tq::star_operands(0.0f, wr[r], true, &a1, &a2, &fz);         // (a2 alone is used; outside the call w = 0 from load_step)
      Gs[tq::stage_row(tid, r) * tq::kPitchA + pp] = tr::gathered_operand(a2, gr[r]);
    }
#pragma unroll
    for (int r = 0; r < tq::kTemplRegs; ++r) Ts[tq::stage_row(tid, r) * tq::kPitchT + pp] = mr[r];
    __syncthreads();
    if (step + 1 < steps) load_step(step + 1);                      // in flight under the matrix instructions
    const int groups = tq::groups_in_step(n, step);
    for (int g = 0; g < groups; ++g) {
      const int px = tq::kGroup * g + k;
      double b[2], A[4];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) b[cb] = tr::template_value(Ts[(32 * wave + 16 * cb + i) * tq::kPitchT + px]);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) A[rb] = Gs[(16 * rb + i) * tq::kPitchA + px];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[rb], b[cb], acc[rb][cb], 0, 0, 0);
    }
    __syncthreads();
  }

  // the pairs: the lane that holds X solves
  auto solve = [&](int rr, int tb, double X, double* al, double* be) {
    const int s = rstar[rr];
    const double Sb = Sw[tr::moment_at(s, M, tb)], Bb = Bw[tr::moment_at(s, M, tb)];
    const bool barred = rcand[rr] == tb || tr::in_earlier_slot(rprev + rr * tr::kMaxPrimaries, rslot[rr], tb);
    return tr::pair_solve(rSa[rr], rBa[rr], Sb, Bb, X, rc0[rr], barred, al, be);
  };
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rr = tq::acc_star(rb, reg, lane), tc = tq::acc_template(wave, cb, lane);
        double v = __builtin_nan(""), al, be;
        if (r0 + rr < R && t0 + tc < M) v = solve(rr, t0 + tc, acc[rb][cb][reg], &al, &be);
        chi[rr * tq::kPitchChi + tc] = v;
      }
  __syncthreads();
  const int count = M - t0 < tq::kChunk ? M - t0 : tq::kChunk;
  if (all) {
    for (int e = tid; e < tr::kRows * tq::kChunk; e += tq::kThreads) {
      const int rr = e / tq::kChunk, tc = e % tq::kChunk;
      if (r0 + rr < R && tc < count) all[(size_t)(r0 + rr) * (size_t)ld_a + (size_t)(t0 + tc)] = chi[rr * tq::kPitchChi + tc];
    }
  }
  if (tid < tr::kRows) {
    double* c = lc + tid * tq::kMaxTopk;
    int* ix = li + tid * tq::kMaxTopk;
    if (r0 + tid < R) {
      tq::list_from_chunk(c, ix, topk, chi + tid * tq::kPitchChi, t0, count);
      const size_t at = tq::part_at((int)blockIdx.y, R, r0 + tid, topk);
      for (int j = 0; j < topk; ++j) {
        part_c[at + j] = c[j];
        part_i[at + j] = ix[j];
      }
    } else {
      tq::list_clear(c, ix, topk);
    }
  }
  __syncthreads();
  // the listed pairs' amplitudes: every entry has one lane that holds its X
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rr = tq::acc_star(rb, reg, lane), tb = t0 + tq::acc_template(wave, cb, lane);
        for (int e = 0; e < topk; ++e)
          if (li[rr * tq::kMaxTopk + e] == tb) {
            double al, be;
            (void)solve(rr, tb, acc[rb][cb][reg], &al, &be);
            const size_t at = tq::part_at((int)blockIdx.y, R, r0 + rr, topk) + (size_t)e;
            part_amp[2 * at] = al;
            part_amp[2 * at + 1] = be;
          }
      }
}

__global__ void __launch_bounds__(tq::kThreads) payne_tmatch_pair_merge_kernel(const double* __restrict__ part_c, const int* __restrict__ part_i,
                                                                               const double* __restrict__ part_amp, const int* __restrict__ cand,
                                                                               int chunks, int N, int kA, int topk, int* __restrict__ idx_a,
                                                                               int* __restrict__ idx_b, double* __restrict__ chisq,
                                                                               double* __restrict__ amp) {
  __shared__ double lc[kMergeStars * tq::kMaxTopk];
  __shared__ int li[kMergeStars * tq::kMaxTopk];
  __shared__ int ls[kMergeStars * tq::kMaxTopk];
  const int tid = threadIdx.x;
  if (tid < kMergeStars) {
    const int s = blockIdx.x * kMergeStars + tid;
    if (s < N) {
      double* c = lc + tid * tq::kMaxTopk;
      int* ix = li + tid * tq::kMaxTopk;
      tr::merge_rows(c, ix, ls + tid * tq::kMaxTopk, topk, part_c, part_i, chunks, N, kA, s);
      for (int j = 0; j < topk; ++j) {
        chisq[(size_t)s * topk + j] = c[j];
        idx_b[(size_t)s * topk + j] = ix[j];
      }
    }
  }
  __syncthreads();
  const int sl = tid / tq::kMaxTopk, j = tid % tq::kMaxTopk;
  const int s = blockIdx.x * kMergeStars + sl;
  if (s < N && j < topk)
    idx_a[(size_t)s * topk + j] = tr::finish_entry(ls[sl * tq::kMaxTopk + j], cand, part_amp, chunks, N, kA, s, topk, amp + 2 * ((size_t)s * topk + j));
}

}  // namespace

extern "C" int payne_tmatch_pair_rows(void) { return tr::kRows; }
extern "C" int payne_tmatch_pair_chunk(void) { return tr::kChunk; }

extern "C" int payne_tmatch_create_pairs(int device, int max_stars, int max_templates, int max_primaries, payne_tmatch** out) {
  if (!out) return fail(PAYNE_E_INVALID, "payne_tmatch_create_pairs: null handle pointer");
  *out = nullptr;
  if (max_primaries < 1 || max_primaries > tr::kMaxPrimaries) return fail(PAYNE_E_INVALID, "payne_tmatch_create_pairs: max_primaries outside 1 .. 16");
  if (max_stars > 0 && (long long)max_stars * (long long)max_primaries > 0x7fffffffLL)
    return fail(PAYNE_E_INVALID, "payne_tmatch_create_pairs: max_stars * max_primaries does not fit an int");
  payne_tmatch* h = nullptr;
  const int rc = payne_tmatch_create(device, max_stars, max_templates, &h);
  if (rc != PAYNE_OK) return rc;
  OnDevice on(device);
  const size_t cells = (size_t)max_stars * (size_t)max_templates;
  const size_t entries = (size_t)tq::chunks_of(max_templates) * (size_t)max_stars * (size_t)max_primaries * (size_t)tq::kMaxTopk;
  void *pm = nullptr, *p0 = nullptr, *pc = nullptr, *pi = nullptr, *pa = nullptr;
  if (!on.ok() || hipMalloc(&pm, 2 * cells * sizeof(double)) != hipSuccess || hipMalloc(&p0, (size_t)max_stars * sizeof(double)) != hipSuccess ||
      hipMalloc(&pc, entries * sizeof(double)) != hipSuccess || hipMalloc(&pi, entries * sizeof(int)) != hipSuccess ||
      hipMalloc(&pa, 2 * entries * sizeof(double)) != hipSuccess) {
    if (pm) (void)hipFree(pm);
    if (p0) (void)hipFree(p0);
    if (pc) (void)hipFree(pc);
    if (pi) (void)hipFree(pi);
    payne_tmatch_destroy(h);
    return fail(PAYNE_E_HIP, "payne_tmatch_create_pairs: allocating the workspace failed");
  }
  h->max_primaries = max_primaries;
  h->pair_mom = static_cast<double*>(pm);
  h->pair_c0 = static_cast<double*>(p0);
  h->pair_c = static_cast<double*>(pc);
  h->pair_i = static_cast<int*>(pi);
  h->pair_amp = static_cast<double*>(pa);
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_tmatch_match_pairs(payne_tmatch* h, const float* templates_dev, int ld_t, int M, const float* flux_dev, const double* w_dev,
                                        int ld_f, int N, int n, const int* cand_dev, int kA, int topk, int* idx_a_dev, int* idx_b_dev,
                                        double* chisq_dev, double* amp_dev, double* all_dev, long long ld_a, void* stream) {
  if (!h) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: null handle");
  if (kA < 1 || kA > h->max_primaries) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: kA outside 1 .. the handle's max_primaries");
  if (topk < 1 || topk > tq::kMaxTopk) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: topk outside 1 .. 8");
  if (N < 0 || N > h->max_stars) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: N outside 0 .. max_stars");
  if (M < 0 || M > h->max_templates) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: M outside 0 .. max_templates");
  if (n < 1 || ld_t < n || ld_f < n) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: n < 1, ld_t < n or ld_f < n");
  if (N == 0 || M == 0) return PAYNE_OK;
  if (!templates_dev || !flux_dev || !w_dev || !cand_dev || !idx_a_dev || !idx_b_dev || !chisq_dev || !amp_dev)
    return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: null pointer");
  if (all_dev && ld_a < (long long)M) return fail(PAYNE_E_INVALID, "payne_tmatch_match_pairs: ld_a < M");
  OnDevice on(h->device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_tmatch_match_pairs: hipSetDevice");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int chunks = tq::chunks_of(M), tiles = tq::tiles_of(N), row_tiles = tr::row_tiles_of(N, kA);
  if (chunks > 65535) return fail(PAYNE_E_UNSUPPORTED, "payne_tmatch_match_pairs: more than 65535 chunks of templates");
  double *Bw = h->pair_mom, *Sw = h->pair_mom + (size_t)h->max_stars * (size_t)h->max_templates;
  hipLaunchKernelGGL(payne_tmatch_pair_moments_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(tq::kThreads), 0, st, templates_dev, (long long)ld_t, M,
                     flux_dev, w_dev, (long long)ld_f, N, n, Bw, Sw, h->pair_c0);
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match_pairs: launching the moments kernel failed");
  hipLaunchKernelGGL(payne_tmatch_pair_cross_kernel, dim3((unsigned)row_tiles, (unsigned)chunks), dim3(tq::kThreads), 0, st, templates_dev, (long long)ld_t,
                     M, w_dev, (long long)ld_f, N, n, cand_dev, kA, topk, Bw, Sw, h->pair_c0, h->pair_c, h->pair_i, h->pair_amp, all_dev, ld_a);
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match_pairs: launching the cross kernel failed");
  hipLaunchKernelGGL(payne_tmatch_pair_merge_kernel, dim3((unsigned)((N + kMergeStars - 1) / kMergeStars)), dim3(tq::kThreads), 0, st, h->pair_c, h->pair_i,
                     h->pair_amp, cand_dev, chunks, N, kA, topk, idx_a_dev, idx_b_dev, chisq_dev, amp_dev);
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match_pairs: launching the merge kernel failed");
  return PAYNE_OK;
}
