// lmfit_phot_emul.cpp -- thepayne_amd/csrc/lmfit_core.hpp and lmfit_phot_core.hpp on the host: payne_lmfit_begin and a sequence of
// payne_lmfit_update_phot calls (k_lmfit.hip): the spectral tile in the kernel's pixel groups and wave stripes, the photometric block,
// the priors, update_star; every buffer of exactly the size the caller's arrays have.  Built by tests/test_lmfit_phot.py with
// -fsanitize=address,undefined as a program of its own.
//   lmfit_phot_emul DIR   reads DIR/cfg.txt ("B K Km Kp P n ld ld_f T F ncol prior", then "lambda0 down up lambda_min lambda_max xtol
//        maxiter"; prior 0: none, 1: mu.bin and sigma.bin, 2: only one of them, which the library rejects), x0.bin (fp64 [B][K]),
//        lo.bin, hi.bin (fp64 [K]), flux.bin (fp32 [B][ld_f]), w.bin (fp64 [B][ld_f]), x.bin (fp64 [n]), sed_col.bin (int32 [K]),
//        obs.bin, pw.bin (fp64 [B][F]), mu.bin, sigma.bin (fp64 [B][K]) and, for update t = 0 .. T - 1, rows<t>.bin (fp32
//        [B][1 + Km][ld]), mags<t>.bin (fp64 [B][F]), dmags<t>.bin (fp64 [B][F][ncol]); writes state_begin.bin and, per update,
//        G<t>.bin (fp64 [B][16][16], the tile update_star is given: its upper triangle holds the block; zero for a star the update
//        skipped) and state<t>.bin as lmfit_poly_emul does.  Exit status 3: arguments the library rejects as invalid, 4: as unsupported.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/lmfit_phot_core.hpp"

namespace lm = payne::lmfit;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "lmfit_phot_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "lmfit_phot_emul: cannot write %s\n", path.c_str());
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
    fprintf(stderr, "usage: lmfit_phot_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int B, K, Km, Kp, P, n, ld, ld_f, T, F, ncol, prior;
  payne_lmfit_opts o;
  FILE* f = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %lf %lf %lf %lf %lf %lf %d", &B, &K, &Km, &Kp, &P, &n, &ld, &ld_f, &T, &F, &ncol, &prior,
                   &o.lambda0, &o.down, &o.up, &o.lambda_min, &o.lambda_max, &o.xtol, &o.maxiter) != 19) {
    fprintf(stderr, "lmfit_phot_emul: cfg.txt\n");
    return 2;
  }
  fclose(f);
  if (B < 1 || K < 1 || K > lm::kMaxK || n < 1 || ld < n || ld_f < n || T < 0 || !lm::opts_ok(o)) {
    fprintf(stderr, "lmfit_phot_emul: arguments the library rejects\n");
    return 3;
  }
  const std::vector<double> lo = read_bin<double>(dir + "/lo.bin", (size_t)K), hi = read_bin<double>(dir + "/hi.bin", (size_t)K);
  const std::vector<int> sed_col = read_bin<int>(dir + "/sed_col.bin", (size_t)K);
  lm::Box box;
  for (int k = 0; k < lm::kMaxK; ++k) {
    box.lo[k] = k < K ? lo[k] : 0.0;
    box.hi[k] = k < K ? hi[k] : 1.0;
  }
  for (int k = 0; k < K; ++k)
    if (!lm::finite(lo[k]) || !lm::finite(hi[k]) || !(lo[k] < hi[k])) {
      fprintf(stderr, "lmfit_phot_emul: a box the library rejects\n");
      return 3;
    }
  const int rc = lm::check_phot(K, Km, Kp, P, F, ncol, sed_col.data(), box, prior != 0, prior == 1);
  if (rc != PAYNE_OK) {
    fprintf(stderr, "lmfit_phot_emul: arguments the library rejects (%d)\n", rc);
    return rc == PAYNE_E_UNSUPPORTED ? 4 : 3;
  }
  const std::vector<double> x0 = read_bin<double>(dir + "/x0.bin", (size_t)B * K);
  const std::vector<float> flux = read_bin<float>(dir + "/flux.bin", (size_t)B * ld_f);
  const std::vector<double> w = read_bin<double>(dir + "/w.bin", (size_t)B * ld_f);
  const std::vector<double> x = read_bin<double>(dir + "/x.bin", (size_t)n);
  const std::vector<double> obs = read_bin<double>(dir + "/obs.bin", (size_t)B * F), pw = read_bin<double>(dir + "/pw.bin", (size_t)B * F);
  std::vector<double> mu, sigma;
  if (prior) {
    mu = read_bin<double>(dir + "/mu.bin", (size_t)B * K);
    sigma = read_bin<double>(dir + "/sigma.bin", (size_t)B * K);
  }
  lm::PhotMap map;
  map.ncol = ncol;
  map.Kp = Kp;
  for (int k = 0; k < lm::kMaxK; ++k) map.sed_col[k] = k < K ? sed_col[(size_t)k] : -1;
  Arrays arr((size_t)B, (size_t)K);
  const lm::State st = arr.state();
  for (int b = 0; b < B; ++b) lm::begin_star(st, (size_t)b, K, x0.data() + (size_t)b * K, box, o.lambda0);
  dump(dir + "/state_begin.bin", arr, (size_t)B, (size_t)K);
  std::vector<double> G((size_t)B * lm::kTileSize), work((size_t)lm::kWorkDoubles), coef((size_t)P), res((size_t)F), pt((size_t)lm::kTileSize);
  for (int t = 0; t < T; ++t) {
    const std::vector<float> rows = read_bin<float>(dir + "/rows" + std::to_string(t) + ".bin", (size_t)B * (1 + Km) * ld);
    const std::vector<double> mags = read_bin<double>(dir + "/mags" + std::to_string(t) + ".bin", (size_t)B * F);
    const std::vector<double> dmags = read_bin<double>(dir + "/dmags" + std::to_string(t) + ".bin", (size_t)B * F * ncol);
    for (int b = 0; b < B; ++b) {
      double* Gb = G.data() + (size_t)b * lm::kTileSize;
      for (int e = 0; e < lm::kTileSize; ++e) Gb[e] = 0.0;
      if (arr.status[b] != PAYNE_LMFIT_RUNNING) continue;           // (the workgroup returns)
      for (int k = 0; k < P; ++k) coef[(size_t)k] = arr.x_trial[(size_t)b * K + (size_t)(Km + Kp + k)];   // (the kernel's copy in LDS)
      lm::tile_sums_gap_host(rows.data() + (size_t)b * (1 + Km) * ld, ld, flux.data() + (size_t)b * ld_f, w.data() + (size_t)b * ld_f, x.data(), n,
                             Km, Kp, P, coef.data(), Gb);
      lm::phot_block_host(map, K, F, mags.data() + (size_t)b * F, dmags.data() + (size_t)b * F * ncol, obs.data() + (size_t)b * F,
                          pw.data() + (size_t)b * F, res.data(), pt.data());
      lm::add_block(Gb, pt.data(), K, arr.x_trial.data() + (size_t)b * K, prior ? mu.data() + (size_t)b * K : nullptr,
                    prior ? sigma.data() + (size_t)b * K : nullptr);
      for (double& v : work) v = __builtin_nan("");               // (LDS holds whatever was there)
      lm::update_star(st, (size_t)b, K, Gb, o, box, work.data());
    }
    write_bin(dir + "/G" + std::to_string(t) + ".bin", G.data(), G.size());
    dump(dir + "/state" + std::to_string(t) + ".bin", arr, (size_t)B, (size_t)K);
  }
  return 0;
}
