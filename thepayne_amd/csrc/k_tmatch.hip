// k_tmatch.hip -- payne_tmatch_*: chi^2 of N spectra against a bank of M templates and each star's top-k (include/payne_hip.h).  The
// arithmetic, the index maps and the lists are tmatch_core.hpp, which runs on the host too (tests/emul/tmatch_emul.cpp).
//
//   payne_tmatch_tile_kernel   grid (star tiles, template chunks), 256 threads.  A workgroup owns 64 stars x 128 templates and walks
//     the pixels in steps of 32: every thread loads 8 (flux, w) pairs and 16 template values of the NEXT step into registers, then
//     the current step's matrix instructions run from LDS (a1, a2 as fp64 [64][34], the templates as fp32 [128][36]; pitches chosen
//     so that one wave's read touches every bank once).  Wave v owns templates 32 v .. 32 v + 31 as 4 x 2 accumulator tiles of
//     v_mfma_f64_16x16x4_f64 (64 accumulator registers a lane); per group of four pixels it reads 8 fp64 star operands and 2 fp32
//     template values a lane and issues 16 matrix instructions.  The staging thread also carries its stars' c0 partial sums.  A
//     step in which some template value is not finite takes a side path that marks the (star, template) pairs it poisons.
//     Behind the pixels: c0 from the partial sums, chi^2 = c0 + accumulator into an LDS tile [64][129], the optional N x M output
//     written from there in rows, and a thread a star inserts the chunk's 128 values into its list, which goes to the workspace.
//   payne_tmatch_merge_kernel  a thread a star walks its chunks' lists in chunk order (lists in LDS) and writes idx, chisq.
//   No atomics; every sum and every list has one fixed order.
#include <hip/hip_runtime.h>

#include "../../include/payne_hip.h"
#include "host_prologue.hpp"
#include "normal_tile.hpp"
#include "tmatch_core.hpp"

namespace tq = payne::tmatch;

#include "tmatch_handle.hpp"

namespace {

using payne::ntile::d4;
using payne::host::OnDevice;
using payne::host::fail;

constexpr int kStageDoubles = 2 * tq::kStars * tq::kPitchA;                              // a1, a2
constexpr int kStageBytes = kStageDoubles * 8 + tq::kChunk * tq::kPitchT * 4;            // + the templates
constexpr int kChiBytes = tq::kStars * tq::kPitchChi * 8;
constexpr int kUnionBytes = kChiBytes > kStageBytes ? kChiBytes : kStageBytes;
static_assert(tq::kStars * tq::kStep * 8 <= kUnionBytes, "the c0 partial sums share the stage");

__global__ void __launch_bounds__(tq::kThreads) payne_tmatch_tile_kernel(const float* __restrict__ templ, long long ld_t, int M,
                                                                         const float* __restrict__ flux, const double* __restrict__ w,
                                                                         long long ld_f, int N, int n, int topk, double* __restrict__ part_c,
                                                                         int* __restrict__ part_i, double* __restrict__ all, long long ld_a) {
  __shared__ __attribute__((aligned(16))) unsigned char raw[kUnionBytes];
  __shared__ double c0s[tq::kStars];
  __shared__ double lc[tq::kStars * tq::kMaxTopk];
  __shared__ int li[tq::kStars * tq::kMaxTopk];
  __shared__ int nf_step;                                           // 1 + the last step that staged a template value that is not finite
  double* As1 = reinterpret_cast<double*>(raw);
  double* As2 = As1 + tq::kStars * tq::kPitchA;
  float* Ts = reinterpret_cast<float*>(raw + kStageDoubles * 8);
  double* c0p = reinterpret_cast<double*>(raw);                     // behind the pixel loop: [64][32]
  double* chi = reinterpret_cast<double*>(raw);                     // behind c0: [64][129]

  const int tid = threadIdx.x, lane = tid & (tq::kWave - 1), wave = tid / tq::kWave;
  const int i = lane & 15, k = lane >> 4;
  const int s0 = blockIdx.x * tq::kStars, t0 = blockIdx.y * tq::kChunk;
  const int pp = tq::stage_pixel(tid);
  if (tid == 0) nf_step = 0;

  float fr[tq::kStarRegs], mr[tq::kTemplRegs];
  double wr[tq::kStarRegs], c0acc[tq::kStarRegs];
  d4 acc[4][2];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = d4{0.0, 0.0, 0.0, 0.0};
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
      for (int cb = 0; cb < 2; ++cb) tq::template_operands(Ts[(32 * wave + 16 * cb + i) * tq::kPitchT + px], &b1[cb], &b2[cb]);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        A1[rb] = As1[(16 * rb + i) * tq::kPitchA + px];
        A2[rb] = As2[(16 * rb + i) * tq::kPitchA + px];
      }
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1[rb], b1[cb], acc[rb][cb], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(A2[rb], b2[cb], acc[rb][cb], 0, 0, 0);
    }
    __syncthreads();
  }

  // c0: the staging threads' partial sums, then j = 0 .. 31 in order
#pragma unroll
  for (int r = 0; r < tq::kStarRegs; ++r) c0p[tq::stage_row(tid, r) * tq::kStep + pp] = c0acc[r];
  __syncthreads();
  if (tid < tq::kStars) {
    double c0 = 0.0;
    for (int j = 0; j < tq::kStep; ++j) c0 += c0p[tid * tq::kStep + j];
    c0s[tid] = c0;
  }
  __syncthreads();
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int sr = tq::acc_star(rb, reg, lane);
        const double v = c0s[sr] + acc[rb][cb][reg];
        chi[sr * tq::kPitchChi + tq::acc_template(wave, cb, lane)] = ((poison >> tq::acc_bit(rb, cb, reg)) & 1u) ? __builtin_nan("") : v;
      }
  __syncthreads();
  const int count = M - t0 < tq::kChunk ? M - t0 : tq::kChunk;
  if (all) {
    for (int e = tid; e < tq::kStars * tq::kChunk; e += tq::kThreads) {
      const int sr = e / tq::kChunk, tr = e % tq::kChunk;
      if (s0 + sr < N && tr < count) all[(size_t)(s0 + sr) * (size_t)ld_a + (size_t)(t0 + tr)] = chi[sr * tq::kPitchChi + tr];
    }
  }
  if (tid < tq::kStars && s0 + tid < N) {
    double* c = lc + tid * tq::kMaxTopk;
    int* ix = li + tid * tq::kMaxTopk;
    tq::list_from_chunk(c, ix, topk, chi + tid * tq::kPitchChi, t0, count);
    const size_t at = tq::part_at((int)blockIdx.y, N, s0 + tid, topk);
    for (int j = 0; j < topk; ++j) {
      part_c[at + j] = c[j];
      part_i[at + j] = ix[j];
    }
  }
}

__global__ void __launch_bounds__(tq::kStars) payne_tmatch_merge_kernel(const double* __restrict__ part_c, const int* __restrict__ part_i, int chunks,
                                                                        int N, int topk, int* __restrict__ idx, double* __restrict__ chisq) {
  __shared__ double lc[tq::kStars * tq::kMaxTopk];
  __shared__ int li[tq::kStars * tq::kMaxTopk];
  const int s = blockIdx.x * tq::kStars + threadIdx.x;
  if (s >= N) return;
  double* c = lc + threadIdx.x * tq::kMaxTopk;
  int* ix = li + threadIdx.x * tq::kMaxTopk;
  tq::merge_chunks(c, ix, topk, part_c, part_i, chunks, N, s);
  for (int j = 0; j < topk; ++j) {
    chisq[(size_t)s * topk + j] = c[j];
    idx[(size_t)s * topk + j] = ix[j];
  }
}

}  // namespace

extern "C" int payne_tmatch_chunk(void) { return tq::kChunk; }

extern "C" int payne_tmatch_create(int device, int max_stars, int max_templates, payne_tmatch** out) {
  if (!out) return fail(PAYNE_E_INVALID, "payne_tmatch_create: null handle pointer");
  *out = nullptr;
  if (max_stars < 1 || max_templates < 1) return fail(PAYNE_E_INVALID, "payne_tmatch_create: max_stars < 1 or max_templates < 1");
  OnDevice on(device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_tmatch_create: hipSetDevice");
  payne_tmatch* h = new payne_tmatch;
  h->device = device;
  h->max_stars = max_stars;
  h->max_templates = max_templates;
  const size_t entries = (size_t)tq::chunks_of(max_templates) * (size_t)max_stars * (size_t)tq::kMaxTopk;
  void *pc = nullptr, *pi = nullptr;
  if (hipMalloc(&pc, entries * sizeof(double)) != hipSuccess || hipMalloc(&pi, entries * sizeof(int)) != hipSuccess) {
    if (pc) (void)hipFree(pc);
    delete h;
    return fail(PAYNE_E_HIP, "payne_tmatch_create: allocating the workspace failed");
  }
  h->part_c = static_cast<double*>(pc);
  h->part_i = static_cast<int*>(pi);
  *out = h;
  return PAYNE_OK;
}

extern "C" int payne_tmatch_match(payne_tmatch* h, const float* templates_dev, int ld_t, int M, const float* flux_dev, const double* w_dev,
                                  int ld_f, int N, int n, int topk, int* idx_dev, double* chisq_dev, double* all_dev, long long ld_a,
                                  void* stream) {
  if (!h) return fail(PAYNE_E_INVALID, "payne_tmatch_match: null handle");
  if (topk < 1 || topk > tq::kMaxTopk) return fail(PAYNE_E_INVALID, "payne_tmatch_match: topk outside 1 .. 8");
  if (N < 0 || N > h->max_stars) return fail(PAYNE_E_INVALID, "payne_tmatch_match: N outside 0 .. max_stars");
  if (M < 0 || M > h->max_templates) return fail(PAYNE_E_INVALID, "payne_tmatch_match: M outside 0 .. max_templates");
  if (n < 1 || ld_t < n || ld_f < n) return fail(PAYNE_E_INVALID, "payne_tmatch_match: n < 1, ld_t < n or ld_f < n");
  if (N == 0 || M == 0) return PAYNE_OK;
  if (!templates_dev || !flux_dev || !w_dev || !idx_dev || !chisq_dev) return fail(PAYNE_E_INVALID, "payne_tmatch_match: null pointer");
  if (all_dev && ld_a < (long long)M) return fail(PAYNE_E_INVALID, "payne_tmatch_match: ld_a < M");
  OnDevice on(h->device);
  if (!on.ok()) return fail(PAYNE_E_HIP, "payne_tmatch_match: hipSetDevice");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int chunks = tq::chunks_of(M), tiles = tq::tiles_of(N);
  if (chunks > 65535) return fail(PAYNE_E_UNSUPPORTED, "payne_tmatch_match: more than 65535 chunks of templates");
  hipLaunchKernelGGL(payne_tmatch_tile_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(tq::kThreads), 0, st, templates_dev, (long long)ld_t, M,
                     flux_dev, w_dev, (long long)ld_f, N, n, topk, h->part_c, h->part_i, all_dev, ld_a);
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match: launching the tile kernel failed");
  hipLaunchKernelGGL(payne_tmatch_merge_kernel, dim3((unsigned)tiles), dim3(tq::kStars), 0, st, h->part_c, h->part_i, chunks, N, topk, idx_dev,
                     chisq_dev);
  if (hipGetLastError() != hipSuccess) return fail(PAYNE_E_HIP, "payne_tmatch_match: launching the merge kernel failed");
  return PAYNE_OK;
}

extern "C" void payne_tmatch_destroy(payne_tmatch* h) {
  if (!h) return;
  {
    OnDevice on(h->device);
    if (on.ok()) {
      (void)hipDeviceSynchronize();
      (void)hipFree(h->part_c);
      (void)hipFree(h->part_i);
      (void)hipFree(h->poly_c);                                     // (null unless payne_tmatch_create_poly made the handle)
      (void)hipFree(h->poly_i);
      (void)hipFree(h->poly_coef);
      (void)hipFree(h->pair_mom);                                   // (null unless payne_tmatch_create_pairs made the handle)
      (void)hipFree(h->pair_c0);
      (void)hipFree(h->pair_c);
      (void)hipFree(h->pair_i);
      (void)hipFree(h->pair_amp);
    }
  }
  delete h;
}
