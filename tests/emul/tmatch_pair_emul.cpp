// tmatch_pair_emul.cpp -- thepayne_amd/csrc/tmatch_pair_core.hpp on the host: one payne_tmatch_match_pairs call (k_tmatch_pair.hip) in
// the kernels' order, moments, rows, chunk lists and merge, every buffer of exactly the size the caller's arrays have.  Built by
// tests/test_tmatch_pair.py with -fsanitize=address,undefined as a program of its own.
//   tmatch_pair_emul DIR   reads DIR/cfg.txt ("N M n ld_t ld_f kA topk want_all"), templates.bin (fp32 [M][ld_t]), flux.bin (fp32
//        [N][ld_f]), w.bin (fp64 [N][ld_f]), cand.bin (int32 [N][kA]); writes idx_a.bin, idx_b.bin (int32 [N][topk]), chisq.bin (fp64
//        [N][topk]), amp.bin (fp64 [N][topk][2]), all.bin (fp64 [N kA][M]; with want_all = 0 all is NULL and the file holds the
//        fill) and tile.txt (the rows and the templates of one workgroup).  Exit status 3: arguments the library rejects.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/tmatch_pair_core.hpp"

namespace tq = payne::tmatch;
namespace tr = payne::tmatch_pair;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "tmatch_pair_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "tmatch_pair_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: tmatch_pair_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int N, M, n, ld_t, ld_f, kA, topk, want_all;
  FILE* f = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d", &N, &M, &n, &ld_t, &ld_f, &kA, &topk, &want_all) != 8) {
    fprintf(stderr, "tmatch_pair_emul: cfg.txt\n");
    return 2;
  }
  fclose(f);
  f = fopen((dir + "/tile.txt").c_str(), "w");
  if (!f) return 2;
  fprintf(f, "%d %d\n", tr::kRows, tr::kChunk);
  fclose(f);
  if (N < 1 || M < 1 || n < 1 || ld_t < n || ld_f < n || topk < 1 || topk > tq::kMaxTopk || kA < 1 || kA > tr::kMaxPrimaries) {
    fprintf(stderr, "tmatch_pair_emul: arguments the library rejects\n");
    return 3;
  }
  const double nan = __builtin_nan("");
  const std::vector<float> templates = read_bin<float>(dir + "/templates.bin", (size_t)M * ld_t);
  const std::vector<float> flux = read_bin<float>(dir + "/flux.bin", (size_t)N * ld_f);
  const std::vector<double> w = read_bin<double>(dir + "/w.bin", (size_t)N * ld_f);
  const std::vector<int> cand = read_bin<int>(dir + "/cand.bin", (size_t)N * kA);
  const size_t entries = (size_t)tq::chunks_of(M) * N * kA * topk;
  std::vector<int> idx_a((size_t)N * topk, 12345), idx_b((size_t)N * topk, 12345), part_i(entries, 12345), src((size_t)topk, 12345);
  std::vector<double> chisq((size_t)N * topk, nan), amp((size_t)N * topk * 2, 0.5), all((size_t)N * kA * M, -777.25);
  std::vector<double> part_c(entries, nan), part_amp(2 * entries, nan), work(4 * (size_t)tq::steps_of(n) * tq::kStep + 5 * (size_t)M, nan);
  tr::match_pairs_host(templates.data(), ld_t, M, flux.data(), w.data(), ld_f, N, n, cand.data(), kA, topk, idx_a.data(), idx_b.data(), chisq.data(),
                       amp.data(), want_all ? all.data() : nullptr, M, part_c.data(), part_i.data(), part_amp.data(), work.data(), src.data());
  write_bin(dir + "/idx_a.bin", idx_a.data(), idx_a.size());
  write_bin(dir + "/idx_b.bin", idx_b.data(), idx_b.size());
  write_bin(dir + "/chisq.bin", chisq.data(), chisq.size());
  write_bin(dir + "/amp.bin", amp.data(), amp.size());
  write_bin(dir + "/all.bin", all.data(), all.size());
  return 0;
}
