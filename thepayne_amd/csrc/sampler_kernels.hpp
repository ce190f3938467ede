// sampler_kernels.hpp -- the sampler step's kernels (device functions: sampler_core.hpp), then the queue's: its staging block's two
// transfers and the turn between two queues (payne_ns_turn_kernel).  Included once, by sampler_api.hip.
#pragma once
#include "sampler_core.hpp"

// transform only (mode 0) or transform + ln-prior + theta row (mode 1).
// (No private arrays and no reference to the by-value argument handed to an out-of-line function: the first version kept the
//  transformed point in a `double vv[PAYNE_MAX_DIM]` indexed by the loop counter and passed `sd.dims[d]` / `sd.adv` by reference to
//  helpers the compiler did not inline -- the whole 4 KB argument struct was copied to scratch memory, 4 400 bytes and 319 spilled
//  registers per thread.  The point is read back from `v`, which this thread has just written; the helpers are inlined.)
__global__ void __launch_bounds__(128) __attribute__((flatten)) payne_prior_kernel(SamplerDev sd, const double* u, int K, double* v, double* lnprior, double* rows, int mode) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K) return;
  double* __restrict__ vc = v + (size_t)c * sd.ndim;
  double lp = 0.0;
  for (int d = 0; d < sd.ndim; ++d) {
    const payne_prior_dim dim = sd.dims[d];
    const double vd = prior_ppf(dim, sd.q0[d], sd.q1[d], u[(size_t)c * sd.ndim + d], sd.adv);
    vc[d] = vd;
    lp += prior_ln(dim, vd);
  }
  if (adv_any(sd.adv)) {
    const payne_adv_priors& a = sd.adv;
    const double add = adv_lnprior(a, a.dim_logg >= 0 ? vc[a.dim_logg] : a.val_logg, a.dim_logr >= 0 ? vc[a.dim_logr] : a.val_logr,
                                   a.dim_vrot >= 0 ? vc[a.dim_vrot] : a.val_vrot, a.plx_dim >= 0 ? vc[a.plx_dim] : 1.0);
    lp = (lp == -INFINITY || add == -INFINITY) ? -INFINITY : lp + add;
  }
  if (mode) {
    lnprior[c] = lp;
    double* row = rows + (size_t)c * sd.ncols;                    // the theta row by column (col_src / col_val: resolved at sampler creation)
    for (int q = 0; q < sd.ncols; ++q) { const int src = sd.col_src[q]; row[q] = src >= 0 ? vc[src] : sd.col_val[q]; }
  }
}
// the per-dimension constants of the transforms, by the device's own normcdf / expm1 / log (sampler creation)
__global__ void payne_prior_cache_kernel(SamplerDev sd, double* q) {
  const int d = threadIdx.x;
  if (d >= sd.ndim) return;
  prior_cache(sd.dims[d], q[d], q[PAYNE_MAX_DIM + d]);
}
// lnprob = lnprior + lnlike (-inf prior wins; NaN likelihood stays NaN)
__global__ void payne_lnprob_kernel(const double* lnprior, const double* lnl, int K, double* out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < K) out[c] = (lnprior[c] == -INFINITY) ? -INFINITY : lnprior[c] + lnl[c];
}

// One random-walk step for every chain, one wave per chain (rwalk_step_wave).  `propose` = 0 on the closing call.
__global__ void __launch_bounds__(256) payne_rwalk_kernel(SamplerDev sd, WalkState W, const double* lnl_prop, int step, int settle, int propose,
                                                             WalkTail* publish) {
  const int lane = threadIdx.x & 63;
  const int c = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  // the walk for the post kernel's tail (the steps that follow run there): written in stream order, by the launch that
  // opens the walk
  // (a queue launched without the host in between: the record carries the scale and threshold the turn kernel left)
  // (publish->sd: uploaded when the sampler was created)
  // (the two values read FIRST, together: behind the record's stores -- which may alias them -- each was a round trip of its own on the
  // wave that then walks chain 0, and the launch lasts as long as its slowest wave)
  if (publish && blockIdx.x == 0 && threadIdx.x == 0) {
    const double sc = walk_scale(W), ls = walk_lstar(W);
    publish->w = W; publish->w.scale = sc; publish->w.loglstar = ls; publish->w.dyn = nullptr;
  }
  if (c >= W.K) return;                                         // the whole wave leaves together
  rwalk_step_wave(sd, W, c, lane, lnl_prop[c], step, settle, propose);
}

// One slice-sampling round for every chain, one wave per chain (slice_round_wave).  `first`: the walk's first round; `propose` = 0 on
// the closing launch, which leaves the number of unfinished chains in S.n_active (zeroed by every proposing launch before it).
__global__ void __launch_bounds__(256) payne_slice_kernel(SamplerDev sd, SliceState S, const double* lnl_prop, int settle, int propose,
                                                             int first) {
  const int lane = threadIdx.x & 63;
  const int c = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (propose && blockIdx.x == 0 && threadIdx.x == 0) *S.n_active = 0;
  if (c >= S.K) return;                                         // the whole wave leaves together
  const SliceLoads L = slice_loads(sd, S, lnl_prop, c, lane);
  slice_round_wave(sd, S, L, c, lane, first, settle, propose);
}

// The queue's staging block up (from mapped host memory) and down (into it; ONE workgroup, which then publishes the queue's
// sequence number behind the block with system scope -- what payne_ns_rwalk_queue_end waits for).
__global__ void __launch_bounds__(256) payne_stage_in_kernel(double* __restrict__ dst, const double* __restrict__ src_host, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src_host[i];
}
__global__ void __launch_bounds__(1024) payne_stage_out_kernel(double* __restrict__ dst_host, const double* __restrict__ src, size_t n,
                                                               unsigned long long* flag, unsigned long long seq,
                                                               const double* __restrict__ src2 = nullptr, int n2 = 0,
                                                               unsigned* arrivals = nullptr) {
  // (several workgroups when `arrivals` is given: the last one to arrive publishes -- atomicInc wraps the count back to zero)
  for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += (size_t)gridDim.x * 1024) dst_host[i] = src[i];
  if (blockIdx.x == 0 && src2 && (int)threadIdx.x < n2) dst_host[n + threadIdx.x] = src2[threadIdx.x];   // (the device's scale and threshold behind the block)
  // (every wave's stores are acknowledged before it passes the barrier; ONE thread's release then covers the workgroup's -- release
  // fences are cumulative --: a fence in each of the sixteen waves, each a write-back of the L2, was 6 us in the turn kernel)
  __syncthreads();
  if (threadIdx.x == 0) {
    bool last = true;
    if (arrivals && gridDim.x > 1) { __threadfence_system(); last = atomicInc(arrivals, gridDim.x - 1) == gridDim.x - 1; }
    if (last) { __threadfence_system(); __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
  }
}

// ---- the queue's turn on the device ------------------------------------------------------------------------------------
// What payne_ns_rwalk_queue_turn does on the host between two queues, as ONE workgroup: the chains that moved are the proposals;
// consuming them in order (each replaces the worst live point if it beats it) leaves the nlive LARGEST of live points and proposals
// -- thresholds only rise, so a proposal in that set beat every threshold it met, and one outside it died or never got in --: a sort
// by (lnprob descending, live points before proposals on ties: the test is strict).  Then the scale adaptation dynesty-style from
// the queue's counters, the new threshold (the largest lnprob left outside the set: the last point to die), and every chain's start point, uniform among the new live
// points (the host's splitmix of the seed).  The host replays the same queue for the evidence in its own time; its live SET is the
// same, its slot order is not (nothing on the device depends on it).
// sum of an int over the wave, in lane 63 (an inclusive scan inside each row of 16 lanes, then the rows' totals handed on)
template <int CTRL> __device__ __forceinline__ int turn_dpp_add(int x) { return x + __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ int turn_wave_sum_to_last(int x) {
  x = turn_dpp_add<0x111>(x); x = turn_dpp_add<0x112>(x); x = turn_dpp_add<0x114>(x); x = turn_dpp_add<0x118>(x);   // row_shr 1, 2, 4, 8
  x = turn_dpp_add<0x142>(x); x = turn_dpp_add<0x143>(x);                                                            // row_bcast 15, 31
  return x;
}
// (the network's exchanges at distances below 64: lane_xor_i32, sampler_core.hpp)
// one stage of the bitonic network at distance J < 64 inside runs of KK, "before" = larger lnprob, then smaller id
template <int KK, int J>
__device__ __forceinline__ void turn_cmpx(double& kv, int& iv, int i) {
  union { double d; int w[2]; } me, pa;
  me.d = kv;
  const bool upper = (i & J) != 0;
  pa.w[0] = lane_xor_i32<J>(me.w[0], upper); pa.w[1] = lane_xor_i32<J>(me.w[1], upper);
  const int ip = lane_xor_i32<J>(iv, upper);
  const bool mine_first = (kv > pa.d) || (kv == pa.d && iv < ip);
  const bool want_first = (!upper) == ((i & KK) == 0);                       // the lower place of an ascending run, the upper of a descending one
  if (mine_first != want_first) { kv = pa.d; iv = ip; }
  if constexpr (J > 1) turn_cmpx<KK, J / 2>(kv, iv, i);
}
struct TurnArgs {
  const double *lu, *lv, *ll; double *ou, *ov, *ol;    // live set in / out (the same arrays when merge == 0)
  int nlive, nd, K, merge, n2;                         // n2: power of two >= nlive + K (<= 2048)
  double *cu, *cv, *cl; int *na, *nc, *nr;             // chains: the finished queue's results in, the next queue's start points out
  double* dyn;                                         // {scale, loglstar}
  double scale0, lstar0;                               // merge == 0: what to start from
  unsigned long long seed;
  // the finished queue's results on their way to the host from HERE (its own transfer kernel was 9 us between two queues): the
  // stores are issued first and drain under the sort; the completion word follows the kernel's last statement
  double* exp_dst; int exp_n; unsigned long long* exp_flag; unsigned long long exp_seq;
  const double* ax_src; double* ax_dst; int ax_n;      // a new bound (axes, centres, inverse axes) from its mapped host block: a launch of its own was 2.8 us in front of this one
  int live_sorted;                                     // the live set comes from a merging turn: best first (rows and lnprob)
  int rows_lds;                                        // the launch carries nlive * nd * 16 bytes of dynamic LDS: the new live set's rows stay there for the start points
};
constexpr size_t kTurnRowsLdsMax = 128 * 1024;
__global__ void __launch_bounds__(1024) payne_ns_turn_kernel(TurnArgs a) {
  __shared__ double key[2048];
  __shared__ int id[2048];
  __shared__ int wsum[3][16];
  __shared__ int got_in_flag;
  extern __shared__ __attribute__((aligned(16))) double turn_rows[];   // [2][nlive * nd] when a.rows_lds
  const int tid = threadIdx.x, nl = a.nlive, nd = a.nd, K = a.K;
  // With the new rows in LDS nothing below the sort reads what this kernel stored to global memory: the barriers there need not wait
  // for the stores to be acknowledged (1.5 us each time) -- the one in front of the completion word does.
  const bool lds_rows = a.merge && a.rows_lds;
  auto lds_barrier = []() {                                  // (__syncthreads also waits for the stores towards the host to be acknowledged)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  };
  auto turn_barrier = [&]() {
    if (lds_rows) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); }
    else __syncthreads();
  };
  double scale = a.scale0, lstar = a.lstar0;
  // Everything the kernel reads before the sort is REQUESTED first, in one go: the keys (a counter and the lnprob it admits), the
  // counters, the scale and threshold, the export's values (sixteen to a thread).  One value at a time -- a load, its store towards
  // the host, the next load: the two may alias -- the export alone was 13 memory latencies end to end (3.3 us), the keys (the counter,
  // THEN the lnprob) and the counters three more.  The export's stores go out right in front of the sort, whose exchanges and
  // comparisons leave the memory path to them.
  // (Every one of these loads is unconditional, its index clamped: a load under a branch leaves the compiler without a count of the
  // loads behind it, and it waits for ALL of them -- the bound's values included, 2 us away across the bus -- in front of the sort.)
  double l_in[2]; int na_in[2];
  int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {                               // (n2 <= 2048; read whether or not this turn merges: one basic block, loads in source order)
    const int e = tid + q * 1024;
    const bool is_live = e < nl;
    const int k = (!is_live && e < nl + K) ? e - nl : 0;
    const double* lp = is_live ? a.ll + e : a.cl + k;
    l_in[q] = *lp;
    na_in[q] = a.na[k];
  }
  const int kc = tid < K ? tid : K - 1;
  const int cnt0 = a.na[kc], cnt1 = a.nc[kc], cnt2 = a.nr[kc];
  const double dyn0 = a.dyn[0], dyn1 = a.dyn[1];
  constexpr int kExpBatch = 16;
  double ex[kExpBatch];
  if (a.exp_dst) {
#pragma unroll
    for (int q = 0; q < kExpBatch; ++q) { const int e = tid + q * 1024; ex[q] = e < a.exp_n ? a.cu[e] : 0.0; }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) if (tid + q * 1024 < nl) na_in[q] = 1;
  if (tid < K) { s0 = cnt0; s1 = cnt1; s2 = cnt2; }
  if (a.merge) for (int k = tid + 1024; k < K; k += 1024) { s0 += a.na[k]; s1 += a.nc[k]; s2 += a.nr[k]; }
  auto export_out = [&]() {                                  // chains | counters (contiguous from a.cu), then the scale and threshold they ran under
    if (!a.exp_dst) return;
#pragma unroll
    for (int q = 0; q < kExpBatch; ++q) { const int e = tid + q * 1024; if (e < a.exp_n) a.exp_dst[e] = ex[q]; }
    for (int e = tid + kExpBatch * 1024; e < a.exp_n; e += 1024) a.exp_dst[e] = a.cu[e];
    if (tid < 2) a.exp_dst[a.exp_n + tid] = tid ? dyn1 : dyn0;
  };
  if (a.merge) {
    // the queue's counters: a sum per wave (a thousand atomics on three LDS words were 25 us of this kernel), met by thread 0 below
    s0 = turn_wave_sum_to_last(s0); s1 = turn_wave_sum_to_last(s1); s2 = turn_wave_sum_to_last(s2);
    if ((tid & 63) == 63) { wsum[0][tid >> 6] = s0; wsum[1][tid >> 6] = s1; wsum[2][tid >> 6] = s2; }
    if (tid == 0) got_in_flag = 0;
    auto adapted_scale = [&]() {                               // dynesty-style, from the queue's counters
      long long c0 = 0, c1 = 0, c2 = 0;
      for (int w = 0; w < 16; ++w) { c0 += wsum[0][w]; c1 += wsum[1][w]; c2 += wsum[2][w]; }
      const long long denom = c1 + c2 > 1 ? c1 + c2 : 1;
      const double frac = (double)c0 / (double)denom;         // a redrawn (out-of-cube) proposal counts as a rejection
      double sc = dyn0 * exp((frac - 0.5) / nd / 0.5);
      sc = sc > 1e-4 ? sc : 1e-4;
      return sc < 4.0 ? sc : 4.0;
    };
    double kv0[2]; int iv0[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + q * 1024;
      kv0[q] = -INFINITY; iv0[q] = (1 << 30) + e;
      if (e < nl + K && na_in[q] > 0) { const double l = l_in[q]; kv0[q] = (l != l) ? -INFINITY : l; iv0[q] = e; }
    }
    // bitonic sort, "before" = larger lnprob, then smaller id
    if (a.n2 <= 1024) {
      // One element per thread, in registers.  The exchanges at distances below 64 stay inside the wave (45 of the 55 stages of 1024
      // elements), the others go through LDS, two buffers in turn: one barrier a stage (every stage as an LDS pass between two
      // barriers made this kernel 38 us).
      // A live set that comes from a merging turn arrives best first, which is the order the network's first stages (runs up to half
      // the array) would bring it to: when it IS one half of the array its threads sit those stages out.
      const int i = tid;
      const bool half_sorted = a.live_sorted && 2 * nl == a.n2 && (nl & 63) == 0;
      double kv = kv0[0];
      int iv = iv0[0];
      lds_barrier();                                          // (the flag's zero in front of its ones; the waves' counters)
      export_out();
      if (tid == 0) scale = adapted_scale();                  // (no part of the sort's result in it: here thread 0's wave has the time, with a sorted half)
      int buf = 0;
      auto lds_stages = [&](int kk, bool idle) {                // distances 64 and up
        for (int j = kk >> 1; j >= 64; j >>= 1) {
          double* kb = key + buf * 1024; int* ib = id + buf * 1024;
          buf ^= 1;
          if (i < a.n2) { kb[i] = kv; ib[i] = iv; }             // (the sorted half's threads too: their partners read them at the last level)
          lds_barrier();
          if (!idle) {
            const double kp = i < a.n2 ? kb[i ^ j] : kv; const int ip = i < a.n2 ? ib[i ^ j] : iv;
            const bool mine_first = (kv > kp) || (kv == kp && iv < ip);
            const bool want_first = (((i & j) == 0) == ((i & kk) == 0));
            if (mine_first != want_first) { kv = kp; iv = ip; }
          }
        }
      };
      if (a.n2 == 1024) {                                       // the usual size, unrolled: the distances are compile-time constants
#define PAYNE_TURN_LEVEL(KK) do { const bool idle = half_sorted && KK <= nl && i < nl; lds_stages(KK, idle); \
                                  if (!idle) turn_cmpx<KK, (KK / 2 < 32 ? KK / 2 : 32)>(kv, iv, i); } while (0)
        PAYNE_TURN_LEVEL(2); PAYNE_TURN_LEVEL(4); PAYNE_TURN_LEVEL(8); PAYNE_TURN_LEVEL(16); PAYNE_TURN_LEVEL(32);
        PAYNE_TURN_LEVEL(64); PAYNE_TURN_LEVEL(128); PAYNE_TURN_LEVEL(256); PAYNE_TURN_LEVEL(512); PAYNE_TURN_LEVEL(1024);
#undef PAYNE_TURN_LEVEL
      } else {
        for (int kk = 2; kk <= a.n2; kk <<= 1) {
          const bool idle = half_sorted && kk <= nl && i < nl;   // (the same for a whole wave: nl is a multiple of 64 here)
          lds_stages(kk, idle);
          if (idle) continue;
          for (int j = kk >> 1 < 32 ? kk >> 1 : 32; j > 0; j >>= 1) {
            const double kp = __shfl_xor(kv, j); const int ip = __shfl_xor(iv, j);
            const bool mine_first = (kv > kp) || (kv == kp && iv < ip);
            const bool want_first = (((i & j) == 0) == ((i & kk) == 0));      // the lower place of an ascending run, the upper of a descending one
            if (mine_first != want_first) { kv = kp; iv = ip; }
          }
        }
      }
      if (buf == 1) lds_barrier();                            // (the last exchange read the first buffer, which the result goes to)
      if (i < a.n2) { key[i] = kv; id[i] = iv; }
      if (i < nl && iv >= nl) got_in_flag = 1;
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q) { const int e = tid + q * 1024; if (e < a.n2) { key[e] = kv0[q]; id[e] = iv0[q]; } }
      export_out();
      lds_barrier();
      if (tid == 0) scale = adapted_scale();
      for (int kk = 2; kk <= a.n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
          lds_barrier();
          for (int i = tid; i < a.n2; i += 1024) {
            const int p = i ^ j;
            if (p > i) {
              const double ki = key[i], kp = key[p]; const int ii = id[i], ip = id[p];
              const bool i_first = (ki > kp) || (ki == kp && ii < ip);
              const bool up = (i & kk) == 0;                   // this run sorts "first things first"
              if (i_first != up) { key[i] = kp; key[p] = ki; id[i] = ip; id[p] = ii; }
            }
          }
        }
      lds_barrier();
      for (int r = tid; r < nl; r += 1024) if (id[r] >= nl) got_in_flag = 1;
    }
    lds_barrier();
    // the threshold the next queue walks under: the largest lnprob left outside the new set.  That is the lnprob D of the last point
    // to die (dynesty's loglstar; payne_ns::peek_index) OR a proposal that was turned away after the last replacement, which lies
    // between D and the new live minimum M -- any threshold in [D, M) is valid to walk under (a proposal is tested again, against the
    // worst live point of its iteration, when the host consumes it), and the host accepts exactly that window (nested.py
    // _fill_queue_dev).  If no proposal got in, nothing died and the old threshold stays.
    if (tid == 0) lstar = got_in_flag ? key[nl] : dyn1;       // (thread 0 alone writes it, and the scale)
    // the new live set, row r = the r-th best
    // (four elements' loads in flight per thread: one element at a time this loop was a dozen memory latencies end to end, 2.6 us)
    const float inv_nd = 1.0f / (float)nd;                   // (e < 2^15, nd <= 64: (e + 0.5) / nd is never within rounding of an integer)
    for (int e0 = tid; e0 < nl * nd; e0 += 4096) {
      double xu[4], xv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q * 1024;
        xu[q] = 0.0; xv[q] = 0.0;
        if (e < nl * nd) {
          const int r = (int)(((float)e + 0.5f) * inv_nd), d = e - r * nd, who = id[r];
          const bool live = who < nl;
          const size_t src = (size_t)(live ? who : who - nl) * nd + d;
          xu[q] = live ? a.lu[src] : a.cu[src];
          xv[q] = live ? a.lv[src] : a.cv[src];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q * 1024;
        if (e < nl * nd) {
          a.ou[e] = xu[q]; a.ov[e] = xv[q];
          if (lds_rows) { turn_rows[e] = xu[q]; turn_rows[nl * nd + e] = xv[q]; }
        }
      }
    }
    for (int r = tid; r < nl; r += 1024) a.ol[r] = key[r];
  }
  // a new bound: read across the bus (2 us), requested HERE -- loads return in order, whoever waits for a later one waits for these --
  // and stored at the end, behind the chains' rows
  double axv[2] = {0.0, 0.0};
  if (a.ax_n > 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) { const int e = tid + q * 1024; if (e < a.ax_n) axv[q] = a.ax_src[e]; }
  }
  if (!a.merge) export_out();
  turn_barrier();                                            // (the chains' rows are overwritten below -- the export above has read the old values --; the new set is read back by this workgroup only)
  if (tid == 0) { a.dyn[0] = scale; a.dyn[1] = lstar; }
  // start points: uniform among the live points (queue_begin_core's draw)
  auto mix = [](unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  };
  for (int k = tid; k < K; k += 1024) {                       // (K <= 1024; the slot of every chain once, through the sort's LDS -- id[] is free: the barrier above)
    const unsigned long long r0 = mix(a.seed ^ (0xA5A5A5A5ull + (unsigned long long)k * 0x100000001B3ull));
    const int i = (nl & (nl - 1)) == 0 ? (int)(r0 & (unsigned long long)(nl - 1)) : (int)(r0 % (unsigned long long)nl);   // (the 64-bit remainder is a routine of 200 instructions)
    id[k] = i;
    a.cl[k] = a.merge ? key[i] : a.ol[i];
    a.na[k] = 0; a.nc[k] = 0; a.nr[k] = 0;
  }
  turn_barrier();
  const float inv_nd_ = 1.0f / (float)nd;
  for (int e0 = tid; e0 < K * nd; e0 += 4096) {
    double xu[4], xv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = e0 + q * 1024;
      xu[q] = 0.0; xv[q] = 0.0;
      if (e < K * nd) {
        const int k = (int)(((float)e + 0.5f) * inv_nd_), d = e - k * nd, i = id[k];
        xu[q] = lds_rows ? turn_rows[i * nd + d] : a.ou[(size_t)i * nd + d];
        xv[q] = lds_rows ? turn_rows[nl * nd + i * nd + d] : a.ov[(size_t)i * nd + d];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = e0 + q * 1024;
      if (e < K * nd) { a.cu[e] = xu[q]; a.cv[e] = xv[q]; }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) { const int e = tid + q * 1024; if (e < a.ax_n) a.ax_dst[e] = axv[q]; }
  for (int e = tid + 2048; e < a.ax_n; e += 1024) a.ax_dst[e] = a.ax_src[e];
  if (a.exp_dst) {
    // every wave's stores are acknowledged before it passes the barrier (__syncthreads waits for them); ONE system-scope release then
    // covers them all (release fences are cumulative) -- a fence in each of the sixteen waves, each a write-back of the L2, was 6 us
    __syncthreads();
    if (tid == 0) __hip_atomic_store(a.exp_flag, a.exp_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
