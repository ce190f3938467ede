// tmatch_emul.cpp -- thepayne_amd/csrc/tmatch_core.hpp on the host: one payne_tmatch_match call (k_tmatch.hip) in the kernel's pixel
// order, chunk lists and merge, every buffer of exactly the size the caller's arrays have.  Built by tests/test_tmatch.py with
// -fsanitize=address,undefined as a program of its own.
//   tmatch_emul DIR   reads DIR/cfg.txt ("N M n ld_t ld_f topk"), templates.bin (fp32 [M][ld_t]), flux.bin (fp32 [N][ld_f]), w.bin
//        (fp64 [N][ld_f]); writes idx.bin (int32 [N][topk]), chisq.bin (fp64 [N][topk]), all.bin (fp64 [N][M]) and chunk.txt
//        (the templates of one workgroup's list).  Exit status 3: arguments the library rejects.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/tmatch_core.hpp"

namespace tq = payne::tmatch;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "tmatch_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "tmatch_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: tmatch_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int N, M, n, ld_t, ld_f, topk;
  FILE* f = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!f || fscanf(f, "%d %d %d %d %d %d", &N, &M, &n, &ld_t, &ld_f, &topk) != 6) {
    fprintf(stderr, "tmatch_emul: cfg.txt\n");
    return 2;
  }
  fclose(f);
  f = fopen((dir + "/chunk.txt").c_str(), "w");
  if (!f) return 2;
  fprintf(f, "%d\n", tq::kChunk);
  fclose(f);
  if (N < 1 || M < 1 || n < 1 || ld_t < n || ld_f < n || topk < 1 || topk > tq::kMaxTopk) {
    fprintf(stderr, "tmatch_emul: arguments the library rejects\n");
    return 3;
  }
  const std::vector<float> templates = read_bin<float>(dir + "/templates.bin", (size_t)M * ld_t);
  const std::vector<float> flux = read_bin<float>(dir + "/flux.bin", (size_t)N * ld_f);
  const std::vector<double> w = read_bin<double>(dir + "/w.bin", (size_t)N * ld_f);
  const size_t chunks = (size_t)tq::chunks_of(M);
  std::vector<int> idx((size_t)N * topk, 12345), part_i(chunks * N * topk, 12345);
  std::vector<double> chisq((size_t)N * topk, __builtin_nan("")), part_c(chunks * N * topk, __builtin_nan("")), all((size_t)N * M, __builtin_nan(""));
  std::vector<double> work(3 * (size_t)tq::steps_of(n) * tq::kStep + (size_t)M, __builtin_nan(""));
  tq::match_host(templates.data(), ld_t, M, flux.data(), w.data(), ld_f, N, n, topk, idx.data(), chisq.data(), all.data(), M, part_c.data(),
                 part_i.data(), work.data());
  write_bin(dir + "/idx.bin", idx.data(), idx.size());
  write_bin(dir + "/chisq.bin", chisq.data(), chisq.size());
  write_bin(dir + "/all.bin", all.data(), all.size());
  return 0;
}
