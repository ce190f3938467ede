// tmatch_poly_emul.cpp -- thepayne_amd/csrc/tmatch_poly_core.hpp on the host: one payne_tmatch_match_poly call (k_tmatch_poly.hip) in
// the kernels' order, chunk lists and merge, every buffer of exactly the size the caller's arrays have.  Built by
// tests/test_tmatch_poly.py with -fsanitize=address,undefined as a program of its own.
//   tmatch_poly_emul DIR   reads DIR/cfg.txt ("N M n ld_t ld_f topk P"), templates.bin (fp32 [M][ld_t]), flux.bin (fp32 [N][ld_f]),
//        w.bin (fp64 [N][ld_f]), x.bin (fp64 [n]); writes idx.bin (int32 [N][topk]), chisq.bin (fp64 [N][topk]), coef.bin (fp64
//        [N][topk][P]), flags.bin (int32 [N][topk]), all.bin (fp64 [N][M]) and tile.txt (the stars and the templates of one
//        workgroup).  P = 0 is the plain search on the same arrays (tmatch_core.hpp's match_host; no coef.bin, no flags.bin).
//        Exit status 3: arguments the library rejects.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/tmatch_poly_core.hpp"

namespace tq = payne::tmatch;
namespace tp = payne::tmatch_poly;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "tmatch_poly_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "tmatch_poly_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: tmatch_poly_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int N, M, n, ld_t, ld_f, topk, P;
  FILE* f = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!f || fscanf(f, "%d %d %d %d %d %d %d", &N, &M, &n, &ld_t, &ld_f, &topk, &P) != 7) {
    fprintf(stderr, "tmatch_poly_emul: cfg.txt\n");
    return 2;
  }
  fclose(f);
  f = fopen((dir + "/tile.txt").c_str(), "w");
  if (!f) return 2;
  fprintf(f, "%d %d\n", tp::kStars, tp::kChunk);
  fclose(f);
  if (N < 1 || M < 1 || n < 1 || ld_t < n || ld_f < n || topk < 1 || topk > tq::kMaxTopk || P < 0 || P > tp::kMaxPoly) {
    fprintf(stderr, "tmatch_poly_emul: arguments the library rejects\n");
    return 3;
  }
  const double nan = __builtin_nan("");
  const std::vector<float> templates = read_bin<float>(dir + "/templates.bin", (size_t)M * ld_t);
  const std::vector<float> flux = read_bin<float>(dir + "/flux.bin", (size_t)N * ld_f);
  const std::vector<double> w = read_bin<double>(dir + "/w.bin", (size_t)N * ld_f);
  const std::vector<double> x = read_bin<double>(dir + "/x.bin", (size_t)n);
  std::vector<int> idx((size_t)N * topk, 12345);
  std::vector<double> chisq((size_t)N * topk, nan), all((size_t)N * M, nan);
  if (P == 0) {
    const size_t chunks = (size_t)tq::chunks_of(M);
    std::vector<int> part_i(chunks * N * topk, 12345);
    std::vector<double> part_c(chunks * N * topk, nan), work(3 * (size_t)tq::steps_of(n) * tq::kStep + (size_t)M, nan);
    tq::match_host(templates.data(), ld_t, M, flux.data(), w.data(), ld_f, N, n, topk, idx.data(), chisq.data(), all.data(), M, part_c.data(),
                   part_i.data(), work.data());
  } else {
    const size_t chunks = (size_t)tp::chunks_of(M);
    std::vector<int> part_i(chunks * N * topk, 12345), flags((size_t)N * topk, 12345);
    std::vector<double> part_c(chunks * N * topk, nan), part_coef(chunks * N * topk * P, nan), coef((size_t)N * topk * P, 0.5);
    std::vector<double> work((size_t)(tp::ops_of(P) + 1) * tq::steps_of(n) * tq::kStep + tp::area_doubles(P) + (size_t)M * (P + 1), nan);
    tp::match_poly_host(templates.data(), ld_t, M, flux.data(), w.data(), ld_f, N, n, x.data(), P, topk, idx.data(), chisq.data(), coef.data(),
                        flags.data(), all.data(), M, part_c.data(), part_i.data(), part_coef.data(), work.data());
    write_bin(dir + "/coef.bin", coef.data(), coef.size());
    write_bin(dir + "/flags.bin", flags.data(), flags.size());
  }
  write_bin(dir + "/idx.bin", idx.data(), idx.size());
  write_bin(dir + "/chisq.bin", chisq.data(), chisq.size());
  write_bin(dir + "/all.bin", all.data(), all.size());
  return 0;
}
