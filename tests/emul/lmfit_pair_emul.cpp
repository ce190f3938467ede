// lmfit_pair_emul.cpp -- thepayne_amd/csrc/lmfit_pair_core.hpp on the host: payne_lmfit_begin and a sequence of
// payne_lmfit_update_pair calls (k_lmfit.hip) in the kernel's pixel groups and wave stripes, every buffer of exactly the size the
// caller's arrays have.  Built by tests/test_lmfit_pair.py with -fsanitize=address,undefined as a program of its own.
//   lmfit_pair_emul DIR   reads DIR/cfg.txt ("B K Kl P Ka Kb n ld ld_f T", then "lambda0 down up lambda_min lambda_max xtol maxiter"),
//        ia.bin, ib.bin (int32 [Kl]; a file that is missing is a null pointer), x0.bin (fp64 [B][K]: the Kl parameters, q, the P
//        coefficients), lo.bin, hi.bin (fp64 [K]), flux.bin (fp32 [B][ld_f]), w.bin (fp64 [B][ld_f]), x.bin (fp64 [n], with P > 0) and,
//        for update t = 0 .. T - 1, rowsa<t>.bin (fp32 [B][1 + Ka][ld]) and rowsb<t>.bin (fp32 [B][1 + Kb][ld]); writes state_begin.bin
//        and, per update, G<t>.bin (fp64 [B][16][16], zero for a star the update skipped) and state<t>.bin: fp64 [B][3 K + K K + 5] =
//        x_best, x_trial, A, g, chisq, lambda, status, niter, at_bound.  Exit status 3: arguments the library rejects.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/lmfit_pair_core.hpp"

namespace lm = payne::lmfit;

namespace {

bool exists(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (f) fclose(f);
  return f != nullptr;
}
template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || (n > 0 && fread(v.data(), sizeof(T), n, f) != n) || fgetc(f) != EOF) {
    fprintf(stderr, "lmfit_pair_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "lmfit_pair_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

struct Arrays {
  std::vector<double> x_best, x_trial, A, g, chisq, lambda;
  std::vector<int> status, niter;
  std::vector<unsigned> at_bound;
  Arrays(size_t B, size_t K) : x_best(B * K), x_trial(B * K), A(B * K * K), g(B * K), chisq(B), lambda(B), status(B), niter(B), at_bound(B) {}
  lm::State state() { return lm::State{x_best.data(), x_trial.data(), A.data(), g.data(), chisq.data(), lambda.data(), status.data(), niter.data(), at_bound.data()}; }
};

void dump(const std::string& path, const Arrays& a, size_t B, size_t K) {
  std::vector<double> out;
  for (size_t b = 0; b < B; ++b) {
    out.insert(out.end(), a.x_best.begin() + b * K, a.x_best.begin() + (b + 1) * K);
    out.insert(out.end(), a.x_trial.begin() + b * K, a.x_trial.begin() + (b + 1) * K);
    out.insert(out.end(), a.A.begin() + b * K * K, a.A.begin() + (b + 1) * K * K);
    out.insert(out.end(), a.g.begin() + b * K, a.g.begin() + (b + 1) * K);
    out.push_back(a.chisq[b]);
    out.push_back(a.lambda[b]);
    out.push_back((double)a.status[b]);
    out.push_back((double)a.niter[b]);
    out.push_back((double)a.at_bound[b]);
  }
  write_bin(path, out.data(), out.size());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: lmfit_pair_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int B, K, Kl, P, Ka, Kb, n, ld, ld_f, T;
  payne_lmfit_opts o;
  FILE* f = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d %d %d %lf %lf %lf %lf %lf %lf %d", &B, &K, &Kl, &P, &Ka, &Kb, &n, &ld, &ld_f, &T, &o.lambda0, &o.down,
                   &o.up, &o.lambda_min, &o.lambda_max, &o.xtol, &o.maxiter) != 17) {
    fprintf(stderr, "lmfit_pair_emul: cfg.txt\n");
    return 2;
  }
  fclose(f);
  if (B < 1 || K < 1 || K > lm::kMaxK || n < 1 || ld < n || ld_f < n || T < 0 || !lm::opts_ok(o) ||
      lm::check_pair_counts(K, Kl, P, Ka, Kb) != PAYNE_OK) {           // (before ia.bin is read as Kl values)
    fprintf(stderr, "lmfit_pair_emul: arguments the library rejects\n");
    return 3;
  }
  // (the sizes of ia / ib are the caller's claim, Kl, whatever check_pair makes of it)
  const bool have_ia = exists(dir + "/ia.bin"), have_ib = exists(dir + "/ib.bin");
  const std::vector<int> ia = have_ia ? read_bin<int>(dir + "/ia.bin", (size_t)(Kl > 0 ? Kl : 0)) : std::vector<int>();
  const std::vector<int> ib = have_ib ? read_bin<int>(dir + "/ib.bin", (size_t)(Kl > 0 ? Kl : 0)) : std::vector<int>();
  if (lm::check_pair(K, Kl, P, Ka, Kb, have_ia ? ia.data() : nullptr, have_ib ? ib.data() : nullptr) != PAYNE_OK) {
    fprintf(stderr, "lmfit_pair_emul: a parameter map the library rejects\n");
    return 3;
  }
  const lm::PairMap map = lm::pair_map(Kl, ia.data(), ib.data());
  const std::vector<double> x0 = read_bin<double>(dir + "/x0.bin", (size_t)B * K);
  const std::vector<double> lo = read_bin<double>(dir + "/lo.bin", (size_t)K), hi = read_bin<double>(dir + "/hi.bin", (size_t)K);
  const std::vector<float> flux = read_bin<float>(dir + "/flux.bin", (size_t)B * ld_f);
  const std::vector<double> w = read_bin<double>(dir + "/w.bin", (size_t)B * ld_f);
  const std::vector<double> x = P > 0 ? read_bin<double>(dir + "/x.bin", (size_t)n) : std::vector<double>();
  lm::Box box;
  for (int k = 0; k < lm::kMaxK; ++k) {
    box.lo[k] = k < K ? lo[k] : 0.0;
    box.hi[k] = k < K ? hi[k] : 1.0;
  }
  for (int k = 0; k < K; ++k)
    if (!lm::finite(lo[k]) || !lm::finite(hi[k]) || !(lo[k] < hi[k])) {
      fprintf(stderr, "lmfit_pair_emul: a box the library rejects\n");
      return 3;
    }
  Arrays arr((size_t)B, (size_t)K);
  const lm::State st = arr.state();
  for (int b = 0; b < B; ++b) lm::begin_star(st, (size_t)b, K, x0.data() + (size_t)b * K, box, o.lambda0);
  dump(dir + "/state_begin.bin", arr, (size_t)B, (size_t)K);
  std::vector<double> G((size_t)B * lm::kTileSize), work((size_t)lm::kWorkDoubles), coef((size_t)P);
  for (int t = 0; t < T; ++t) {
    const std::vector<float> ra = read_bin<float>(dir + "/rowsa" + std::to_string(t) + ".bin", (size_t)B * (1 + Ka) * ld);
    const std::vector<float> rb = read_bin<float>(dir + "/rowsb" + std::to_string(t) + ".bin", (size_t)B * (1 + Kb) * ld);
    for (int b = 0; b < B; ++b) {
      double* Gb = G.data() + (size_t)b * lm::kTileSize;
      for (int e = 0; e < lm::kTileSize; ++e) Gb[e] = 0.0;
      if (arr.status[b] != PAYNE_LMFIT_RUNNING) continue;           // (the workgroup returns)
      const double q = arr.x_trial[(size_t)b * K + (size_t)Kl];     // (the kernel's copy in LDS)
      for (int k = 0; k < P; ++k) coef[(size_t)k] = arr.x_trial[(size_t)b * K + (size_t)(Kl + 1 + k)];
      lm::tile_sums_pair_host(ra.data() + (size_t)b * (1 + Ka) * ld, rb.data() + (size_t)b * (1 + Kb) * ld, ld, flux.data() + (size_t)b * ld_f,
                              w.data() + (size_t)b * ld_f, x.data(), n, Kl, P, map, q, coef.data(), Gb);
      for (double& v : work) v = __builtin_nan("");               // (LDS holds whatever was there)
      lm::update_star(st, (size_t)b, K, Gb, o, box, work.data());
    }
    write_bin(dir + "/G" + std::to_string(t) + ".bin", G.data(), G.size());
    dump(dir + "/state" + std::to_string(t) + ".bin", arr, (size_t)B, (size_t)K);
  }
  return 0;
}
