// contfit_emul.cpp -- thepayne_amd/csrc/contfit_core.hpp on the host: payne_contfit_batch (k_contfit.hip) star by star in the
// kernel's passes, pixel groups and wave stripes, every buffer of exactly the size the caller's arrays have.  Built by
// tests/test_contfit.py with -fsanitize=address,undefined as a program of its own.
//   contfit_emul DIR   reads DIR/cfg.txt ("N n ld_f ld_m ld_o n_models has_index P nclip rescale drop_clipped kappa_lo kappa_hi
//        sentinel"), flux.bin (fp32 [N][ld_f]), w.bin (fp64 [N][ld_f]), model.bin (fp32 [n_models][ld_m]), x.bin (fp64 [n]) and, with
//        has_index, index.bin (int32 [N]); writes coef.bin (fp64 [N][P] and one more row of sentinels), chisq.bin (fp64 [N]), npix.bin,
//        status.bin, rounds.bin (int32 [N]), flux_out.bin (fp32 [N][ld_o]) and w_out.bin (fp64 [N][ld_o]), both pre-filled with the
//        sentinel, and per solve that succeeded, star after star, G.bin (fp64 [16][16]) and kept.bin (bytes [n]).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/contfit_core.hpp"

namespace cf = payne::contfit;
namespace lm = payne::lmfit;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "contfit_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const std::vector<T>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    fprintf(stderr, "contfit_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: contfit_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int N, n, ld_f, ld_m, ld_o, n_models, has_index;
  double sentinel;
  payne_contfit_opts o;
  FILE* f = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %lf %lf %lf", &N, &n, &ld_f, &ld_m, &ld_o, &n_models, &has_index, &o.P, &o.nclip,
                   &o.rescale, &o.drop_clipped, &o.kappa_lo, &o.kappa_hi, &sentinel) != 14) {
    fprintf(stderr, "contfit_emul: cfg.txt\n");
    return 2;
  }
  fclose(f);
  if (!cf::opts_ok(o) || N < 1 || n < 1 || n > cf::kMaxN || ld_f < n || ld_m < n || ld_o < n || n_models < 1 || (!has_index && n_models < N)) {
    fprintf(stderr, "contfit_emul: arguments the library rejects\n");
    return 3;
  }
  const std::vector<float> flux = read_bin<float>(dir + "/flux.bin", (size_t)N * ld_f);
  const std::vector<double> w = read_bin<double>(dir + "/w.bin", (size_t)N * ld_f);
  const std::vector<float> model = read_bin<float>(dir + "/model.bin", (size_t)n_models * ld_m);
  const std::vector<double> x = read_bin<double>(dir + "/x.bin", (size_t)n);
  std::vector<int> index;
  if (has_index) index = read_bin<int>(dir + "/index.bin", (size_t)N);
  const size_t P = (size_t)o.P;
  // The kernel's four-pixel forms (cheb4, poly4) give the values of the scalar forms the walk below uses, to the bit.
  for (int p = 0; p + 4 <= n; p += 4) {
    double T[4], pv[4], c[cf::kMaxP];
    for (int k = 0; k < cf::kMaxP; ++k) c[k] = 1.0 / (1.0 + k) - 0.3 * x[(size_t)p];
    cf::poly4(c, o.P, x.data() + p, pv);
    for (int i = 0; i <= o.P; ++i) {
      cf::cheb4(i < o.P ? i : 0, o.P, x.data() + p, T);
      for (int t = 0; t < 4; ++t) {
        const double T1 = cf::cheb(i < o.P ? i : 0, x[(size_t)(p + t)]), p1 = cf::poly_value(c, o.P, x[(size_t)(p + t)]);
        if (memcmp(&T[t], &T1, sizeof(double)) != 0 || memcmp(&pv[t], &p1, sizeof(double)) != 0) {
          fprintf(stderr, "contfit_emul: cheb4 / poly4 differ from cheb / poly_value at pixel %d\n", p + t);
          return 4;
        }
      }
    }
  }
  std::vector<double> coef((size_t)(N + 1) * P, sentinel), chisq((size_t)N, sentinel), w_out((size_t)N * ld_o, sentinel);
  std::vector<float> flux_out((size_t)N * ld_o, (float)sentinel);
  std::vector<int> npix((size_t)N, -1), status((size_t)N, -1), rounds((size_t)N, -1);
  cf::HostTrace trace;
  std::vector<double> G((size_t)lm::kTileSize), work((size_t)cf::kWorkDoubles), coef_lds((size_t)cf::kMaxP);
  std::vector<unsigned> mask((size_t)cf::mask_words(n));
  for (int s = 0; s < N; ++s) {
    for (double& v : G) v = __builtin_nan("");                      // (LDS holds whatever was there)
    for (double& v : work) v = __builtin_nan("");
    for (double& v : coef_lds) v = __builtin_nan("");
    memset(mask.data(), 0xa5, mask.size() * sizeof(unsigned));
    const int mi = has_index ? index[(size_t)s] : s;
    const float* row = mi < 0 || mi >= n_models ? nullptr : model.data() + (size_t)mi * ld_m;
    cf::fit_star_host(flux.data() + (size_t)s * ld_f, w.data() + (size_t)s * ld_f, row, x.data(), n, o, G.data(), work.data(), coef_lds.data(),
                      mask.data(), coef.data() + (size_t)s * P, &chisq[(size_t)s], &npix[(size_t)s], &status[(size_t)s], &rounds[(size_t)s],
                      flux_out.data() + (size_t)s * ld_o, w_out.data() + (size_t)s * ld_o, &trace);
  }
  write_bin(dir + "/coef.bin", coef);
  write_bin(dir + "/chisq.bin", chisq);
  write_bin(dir + "/npix.bin", npix);
  write_bin(dir + "/status.bin", status);
  write_bin(dir + "/rounds.bin", rounds);
  write_bin(dir + "/flux_out.bin", flux_out);
  write_bin(dir + "/w_out.bin", w_out);
  write_bin(dir + "/G.bin", trace.G);
  write_bin(dir + "/kept.bin", trace.kept);
  return 0;
}
