// mad_emul.cpp -- thepayne_amd/csrc/mad_core.hpp on the host: the two kernels of k_mad.hip restated as loops over the waves
// and lanes of one workgroup (phases separated where the kernels have barriers), calling the same key, digit, walk and median
// functions on counters laid out as the kernels lay them out in LDS.  Built by tests/test_testspec.py with
// -fsanitize=address,undefined as a program of its own (a sanitizer runtime wants to be the first thing a process loads):
//   mad_emul DIR N P ld_pred ld_truth G rows   reads DIR/pred.bin (fp32 [N][ld_pred]), truth.bin (fp32 [N][ld_truth]),
//                                              groups.bin (uint8 [G][N]); writes pix_med.bin (fp64 [G][P]) and, with rows = 1,
//                                              row_med.bin (fp64 [N])
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/mad_core.hpp"

using namespace payne;

typedef unsigned long long u64;

namespace {

// for_member_rows of k_mad.hip for one wave: the chunks of 64 rows this wave takes, the members of each in ascending order.
template <class F> void for_member_rows(int N, const unsigned char* grp, int wave, F&& f) {
  for (long long row0 = (long long)wave * mad::kWave; row0 < N; row0 += (long long)mad::kWaves * mad::kWave) {
    u64 members = 0;
    for (int lane = 0; lane < mad::kWave; ++lane)
      if (row0 + lane < N && grp[row0 + lane] != 0) members |= 1ull << lane;
    for (; members; members &= members - 1ull) f(row0 + __builtin_ctzll(members));
  }
}

}  // namespace

extern "C" int mad_emul_cols(const float* pred, int ld_pred, const float* truth, int ld_truth, int N, int P,
                             const unsigned char* groups, int G, double* pix_med) {
  if (N < 1 || P < 1 || ld_pred < P || ld_truth < P || G < 0) return -1;
  std::vector<unsigned> hist((size_t)mad::kBins * mad::kCols), part((size_t)mad::kWaves * mad::kCols), any_nan(mad::kCols);
  std::vector<u64> mins((size_t)mad::kWaves * mad::kCols);
  std::vector<mad::Sel> sel(mad::kCols);
  for (int g = 0; g < G; ++g) {
    const unsigned char* grp = groups + (size_t)g * (size_t)N;
    for (int block = 0; block * mad::kCols < P; ++block) {
      auto key = [&](long long row, int lane) {
        const size_t col = (size_t)block * mad::kCols + lane;
        return mad::residual_key(truth[(size_t)row * ld_truth + col], pred[(size_t)row * ld_pred + col]);
      };
      auto live = [&](int lane) { return block * mad::kCols + lane < P; };
      std::fill(hist.begin(), hist.end(), 0u);
      std::fill(any_nan.begin(), any_nan.end(), 0u);
      for (int pass = 0; pass < mad::kPasses; ++pass) {
        for (int wave = 0; wave < mad::kWaves; ++wave)                        // the counting sweep
          for_member_rows(N, grp, wave, [&](long long row) {
            for (int lane = 0; lane < mad::kWave; ++lane) {
              if (!live(lane)) continue;
              const u64 k = key(row, lane);
              if (pass == 0 && mad::key_is_nan(k)) any_nan[lane] |= 1u;
              if (mad::in_prefix(k, pass ? sel[lane].prefix : 0ull, pass)) hist[(size_t)mad::digit_of(k, pass) * mad::kCols + lane] += 1u;
            }
          });
        for (int wave = 0; wave < mad::kWaves; ++wave)                        // every wave adds up a quarter of the bins
          for (int lane = 0; lane < mad::kWave; ++lane)
            part[wave * mad::kCols + lane] = mad::sum_bins(hist.data() + lane + (size_t)wave * mad::kQuarter * mad::kCols, mad::kCols, mad::kQuarter);
        for (int lane = 0; lane < mad::kWave; ++lane)                         // wave 0 walks
          mad::choose_digit(&sel[lane], pass, part.data() + lane, mad::kCols, mad::kWaves, hist.data() + lane, mad::kCols, mad::kQuarter);
        std::fill(hist.begin(), hist.end(), 0u);
      }
      bool any = false;
      for (int lane = 0; lane < mad::kWave; ++lane) any = any || (live(lane) && mad::needs_next(sel[lane]));
      if (any)
        for (int wave = 0; wave < mad::kWaves; ++wave) {
          for (int lane = 0; lane < mad::kWave; ++lane) mins[wave * mad::kCols + lane] = mad::kNoKey;
          for_member_rows(N, grp, wave, [&](long long row) {
            for (int lane = 0; lane < mad::kWave; ++lane) {
              if (!live(lane)) continue;
              const u64 k = key(row, lane);
              u64& mn = mins[wave * mad::kCols + lane];
              if (k > sel[lane].prefix && k < mn) mn = k;
            }
          });
        }
      for (int lane = 0; lane < mad::kWave; ++lane) {
        if (!live(lane)) continue;
        u64 next = mad::kNoKey;
        if (mad::needs_next(sel[lane]))
          for (int w = 0; w < mad::kWaves; ++w) next = mins[w * mad::kCols + lane] < next ? mins[w * mad::kCols + lane] : next;
        pix_med[(size_t)g * P + (size_t)block * mad::kCols + lane] = mad::median_of(sel[lane], next, any_nan[lane] != 0u);
      }
    }
  }
  return 0;
}

extern "C" int mad_emul_rows(const float* pred, int ld_pred, const float* truth, int ld_truth, int N, int P, double* row_med) {
  if (N < 1 || P < 1 || ld_pred < P || ld_truth < P) return -1;
  std::vector<unsigned> hist(mad::kBins), part(mad::kWave);
  std::vector<u64> mins(mad::kWave);
  for (int row = 0; row < N; ++row) {                                          // one wave each
    const float* t_row = truth + (size_t)row * ld_truth;
    const float* p_row = pred + (size_t)row * ld_pred;
    mad::Sel sel = mad::Sel();
    bool any_nan = false;
    std::fill(hist.begin(), hist.end(), 0u);
    for (int pass = 0; pass < mad::kPasses; ++pass) {
      for (int lane = 0; lane < mad::kWave; ++lane)
        for (int j = lane; j < P; j += mad::kWave) {
          const u64 k = mad::residual_key(t_row[j], p_row[j]);
          if (pass == 0 && mad::key_is_nan(k)) any_nan = true;
          if (mad::in_prefix(k, pass ? sel.prefix : 0ull, pass)) hist[mad::digit_of(k, pass)] += 1u;
        }
      for (int lane = 0; lane < mad::kWave; ++lane) part[lane] = mad::sum_bins(hist.data() + lane * mad::kPerLane, 1, mad::kPerLane);
      mad::choose_digit(&sel, pass, part.data(), 1, mad::kWave, hist.data(), 1, mad::kPerLane);
      std::fill(hist.begin(), hist.end(), 0u);
    }
    u64 next = mad::kNoKey;
    if ((P & 1) == 0) {
      for (int lane = 0; lane < mad::kWave; ++lane) {
        mins[lane] = mad::kNoKey;
        if (mad::needs_next(sel))
          for (int j = lane; j < P; j += mad::kWave) {
            const u64 k = mad::residual_key(t_row[j], p_row[j]);
            if (k > sel.prefix && k < mins[lane]) mins[lane] = k;
          }
      }
      if (mad::needs_next(sel))
        for (int lane = 0; lane < mad::kWave; ++lane) next = mins[lane] < next ? mins[lane] : next;
    }
    row_med[row] = mad::median_of(sel, next, any_nan);
  }
  return 0;
}

namespace {

template <class V> std::vector<V> read_bin(const std::string& dir, const char* name, size_t n) {
  std::vector<V> v(n);
  FILE* f = fopen((dir + "/" + name).c_str(), "rb");
  if (!f || (n && fread(v.data(), sizeof(V), n, f) != n)) { fprintf(stderr, "cannot read %zu values of %s\n", n, name); exit(2); }
  fclose(f);
  return v;
}

template <class V> void write_bin(const std::string& dir, const char* name, const std::vector<V>& v) {
  FILE* f = fopen((dir + "/" + name).c_str(), "wb");
  if (!f || (v.size() && fwrite(v.data(), sizeof(V), v.size(), f) != v.size())) { fprintf(stderr, "cannot write %s\n", name); exit(2); }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: mad_emul DIR N P ld_pred ld_truth G rows\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int N = atoi(argv[2]), P = atoi(argv[3]), ld_pred = atoi(argv[4]), ld_truth = atoi(argv[5]), G = atoi(argv[6]);
  const bool rows = atoi(argv[7]) != 0;
  if (N < 1 || P < 1 || ld_pred < P || ld_truth < P || G < 0) return 2;
  const auto pred = read_bin<float>(dir, "pred.bin", (size_t)N * ld_pred);
  const auto truth = read_bin<float>(dir, "truth.bin", (size_t)N * ld_truth);
  const auto groups = read_bin<unsigned char>(dir, "groups.bin", (size_t)G * N);
  std::vector<double> pix_med((size_t)G * P), row_med(rows ? N : 0);
  if (mad_emul_cols(pred.data(), ld_pred, truth.data(), ld_truth, N, P, groups.data(), G, pix_med.data())) return 3;
  write_bin(dir, "pix_med.bin", pix_med);
  if (rows) {
    if (mad_emul_rows(pred.data(), ld_pred, truth.data(), ld_truth, N, P, row_med.data())) return 3;
    write_bin(dir, "row_med.bin", row_med);
  }
  return 0;
}
