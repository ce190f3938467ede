// quicklook_emul.cpp -- thepayne_amd/csrc/quicklook_core.hpp on the host: the two kernels of k_quicklook.hip restated as
// loops over the threads of one workgroup (phases separated where the kernels have barriers), calling the same
// interpolate-and-sum and compaction functions.  Built by tests/test_quicklook.py with -fsanitize=address,undefined as a
// program of its own (a sanitizer runtime wants to be the first thing a process loads):
//   quicklook_emul rv DIR nm nobs G            reads DIR/{modwave,modflux,wave,flux,eflux,rv}.bin (fp64), writes chisq.bin
//   quicklook_emul below DIR ld n G threshold  reads DIR/rows.bin (fp32 [G][ld]), flux.bin, eflux.bin; writes chisq.bin, kept.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/quicklook_core.hpp"

using namespace payne;

extern "C" int ql_emul_rv_scan(const double* modwave, const double* modflux, int nm, const double* wave, const double* flux,
                               const double* eflux, int nobs, const double* rv, int G, double* chisq) {
  if (nm < 2 || nobs < 1 || G < 1) return -1;
  std::vector<double> partial(ql::kThreads);
  for (int g = 0; g < G; ++g) {
    for (int tid = 0; tid < ql::kThreads; ++tid)
      partial[tid] = ql::rv_partial(modwave, modflux, nm, wave, flux, eflux, nobs, rv[g], tid, ql::kThreads);
    chisq[g] = ql::block_sum_host(partial.data());
  }
  return 0;
}

extern "C" int ql_emul_chisq_below(const float* rows, int ld, int n, int G, const double* flux, const double* eflux,
                                   double threshold, double* chisq, int* n_kept) {
  if (n < 1 || n > ld || G < 1) return -1;
  std::vector<double> acc(ql::kThreads);
  for (int g = 0; g < G; ++g) {
    const float* row = rows + (size_t)g * (size_t)ld;
    for (double& a : acc) a = 0.0;
    int kept_before = 0;
    for (int base = 0; base < n; base += ql::kThreads) {
      unsigned long long ballot[ql::kWaves];
      int wave_total[ql::kWaves];
      for (int w = 0; w < ql::kWaves; ++w) {                      // phase 1: the ballots and the per-wave totals
        ballot[w] = 0;
        for (int lane = 0; lane < ql::kWave; ++lane) {
          const int i = base + w * ql::kWave + lane;
          if (i < n && ql::keep_below(row[i], threshold)) ballot[w] |= 1ull << lane;
        }
        wave_total[w] = __builtin_popcountll(ballot[w]);
      }
      for (int tid = 0; tid < ql::kThreads; ++tid) {              // phase 2: every kept pixel's term at its compacted index
        const int w = tid / ql::kWave, lane = tid % ql::kWave;
        if ((ballot[w] >> lane) & 1ull)
          acc[tid] += ql::below_term(row, flux, eflux, base + tid, kept_before + ql::wave_prefix(wave_total, w) + ql::lane_prefix(ballot[w], lane));
      }
      kept_before += ql::wave_prefix(wave_total, ql::kWaves);
    }
    chisq[g] = ql::block_sum_host(acc.data());
    n_kept[g] = kept_before;
  }
  return 0;
}

namespace {

template <class V> std::vector<V> read_bin(const std::string& dir, const char* name, size_t n) {
  std::vector<V> v(n);
  FILE* f = fopen((dir + "/" + name).c_str(), "rb");
  if (!f || fread(v.data(), sizeof(V), n, f) != n) { fprintf(stderr, "cannot read %zu values of %s\n", n, name); exit(2); }
  fclose(f);
  return v;
}

template <class V> void write_bin(const std::string& dir, const char* name, const std::vector<V>& v) {
  FILE* f = fopen((dir + "/" + name).c_str(), "wb");
  if (!f || fwrite(v.data(), sizeof(V), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", name); exit(2); }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "rv")) {
    const std::string dir = argv[2];
    const int nm = atoi(argv[3]), nobs = atoi(argv[4]), G = atoi(argv[5]);
    if (nm < 2 || nobs < 1 || G < 1) return 2;
    const auto modwave = read_bin<double>(dir, "modwave.bin", nm), modflux = read_bin<double>(dir, "modflux.bin", nm);
    const auto wave = read_bin<double>(dir, "wave.bin", nobs), flux = read_bin<double>(dir, "flux.bin", nobs);
    const auto eflux = read_bin<double>(dir, "eflux.bin", nobs), rv = read_bin<double>(dir, "rv.bin", G);
    std::vector<double> chisq(G);
    if (ql_emul_rv_scan(modwave.data(), modflux.data(), nm, wave.data(), flux.data(), eflux.data(), nobs, rv.data(), G, chisq.data())) return 3;
    write_bin(dir, "chisq.bin", chisq);
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "below")) {
    const std::string dir = argv[2];
    const int ld = atoi(argv[3]), n = atoi(argv[4]), G = atoi(argv[5]);
    const double threshold = atof(argv[6]);
    if (n < 1 || n > ld || G < 1) return 2;
    const auto rows = read_bin<float>(dir, "rows.bin", (size_t)G * ld);
    const auto flux = read_bin<double>(dir, "flux.bin", n), eflux = read_bin<double>(dir, "eflux.bin", n);
    std::vector<double> chisq(G);
    std::vector<int> kept(G);
    if (ql_emul_chisq_below(rows.data(), ld, n, G, flux.data(), eflux.data(), threshold, chisq.data(), kept.data())) return 3;
    write_bin(dir, "chisq.bin", chisq);
    write_bin(dir, "kept.bin", kept);
    return 0;
  }
  fprintf(stderr, "usage: quicklook_emul rv DIR nm nobs G | below DIR ld n G threshold\n");
  return 2;
}
