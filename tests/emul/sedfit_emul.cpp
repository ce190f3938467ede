// sedfit_emul.cpp -- thepayne_amd/csrc/sedfit_core.hpp on the host: payne_sedfit_jac and payne_sedfit_run (k_sedfit.hip) star by star,
// every buffer of exactly the size the caller's arrays have, the workspace filled with NaN before every star.  Built by
// tests/test_sedfit.py with -fsanitize=address,undefined as a program of its own.
//   sedfit_emul DIR   reads DIR/cfg.txt ("F H photscale B free_mask has_hiav has_prior", then "lambda0 down up lambda_min lambda_max
//        xtol maxiter"), the nets in fastANN's stacking w1.bin (fp32 [F][H][6]), b1.bin [F][H], w2.bin [F][H][H], b2.bin, w3.bin [F][H],
//        b3.bin [F], xmin.bin, xmax.bin (fp64 [6]), hiav.bin (fp64 [F][5], with has_hiav) and pars.bin (fp64 [B][P], P = 7 | 6).
//        Writes mags.bin (fp64 [B][F]) and dmags.bin (fp64 [B][F][P]) at pars.  With free_mask != 0 it also reads obs.bin, w.bin (fp64
//        [B][F]), lo.bin, hi.bin (fp64 [K]) and, with has_prior, mu.bin, sigma.bin (fp64 [B][K]), fits every star from pars and writes
//        G0.bin (fp64 [B][16][16]: the first evaluation's tile, priors included; zero where there was none) and fit.bin: fp64
//        [B][P + 1 + K K + 4] = pars, chisq, A, status, niter, at_bound, nfilt.  Exit code 3: arguments the library rejects.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/sedfit_core.hpp"

namespace sf = payne::sedfit;
namespace lm = payne::lmfit;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "sedfit_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "sedfit_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

struct Nets {
  int F, H;
  std::vector<float> w1, b1, w2, b2, w3, b3;
  std::vector<double> xmin, xden, hiav;
  bool has_hiav;
  sf::Net net(int f) const {
    const size_t h = (size_t)H;
    return sf::Net{H, w1.data() + f * h * 6, b1.data() + f * h, w2.data() + f * h * h, b2.data() + f * h, w3.data() + f * h, b3[f]};
  }
  const double* table(int f) const { return has_hiav ? hiav.data() + 5 * (size_t)f : nullptr; }
};

// the magnitude of filter f at `row` and dm [P]; net_work holds 2 H (1 + Kn) doubles, dbc 5
void filter_at(const Nets& N, const sf::Plan& pl, const sf::RowTerms& t, const sf::Row& r, int f, double* net_work, double* dbc_t, double* dbc,
               double* m, double* dm) {
  double bc;
  sf::net_forward(N.net(f), r.xs, N.xden.data(), pl.Kn, pl.tan_in, net_work, &bc, dbc_t);
  for (int d = 0; d < sf::kMaxTan; ++d) {
    const int tan = pl.tan_of[d < 4 ? d : pl.P - 1];
    dbc[d] = tan >= 0 ? dbc_t[tan] : 0.0;
  }
  sf::mag_grad(pl.photscale, t, r.av, bc, dbc, r.hi, N.table(f), m, dm);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: sedfit_emul DIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  int F, H, photscale, B, has_hiav, has_prior;
  unsigned free_mask;
  payne_lmfit_opts o;
  FILE* fh = fopen((dir + "/cfg.txt").c_str(), "r");
  if (!fh || fscanf(fh, "%d %d %d %d %u %d %d %lf %lf %lf %lf %lf %lf %d", &F, &H, &photscale, &B, &free_mask, &has_hiav, &has_prior, &o.lambda0,
                    &o.down, &o.up, &o.lambda_min, &o.lambda_max, &o.xtol, &o.maxiter) != 14) {
    fprintf(stderr, "sedfit_emul: cfg.txt\n");
    return 2;
  }
  fclose(fh);
  if (F < 1 || H < 1 || H > sf::kMaxH || B < 1 || (photscale != 0 && photscale != 1)) {
    fprintf(stderr, "sedfit_emul: arguments the library rejects\n");
    return 3;
  }
  const size_t f_n = (size_t)F, h = (size_t)H, b_n = (size_t)B;
  Nets N{F, H, read_bin<float>(dir + "/w1.bin", f_n * h * 6), read_bin<float>(dir + "/b1.bin", f_n * h), read_bin<float>(dir + "/w2.bin", f_n * h * h),
         read_bin<float>(dir + "/b2.bin", f_n * h), read_bin<float>(dir + "/w3.bin", f_n * h), read_bin<float>(dir + "/b3.bin", f_n),
         read_bin<double>(dir + "/xmin.bin", 6), read_bin<double>(dir + "/xmax.bin", 6),
         has_hiav ? read_bin<double>(dir + "/hiav.bin", 5 * f_n) : std::vector<double>(), has_hiav != 0};
  for (int d = 0; d < sf::kNetIn; ++d) {
    if (!sf::finite(N.xmin[d]) || !sf::finite(N.xden[d]) || !(N.xmin[d] < N.xden[d])) return 3;
    N.xden[d] = N.xden[d] - N.xmin[d];
  }
  const int P = sf::n_pars(photscale);
  const std::vector<double> pars = read_bin<double>(dir + "/pars.bin", b_n * P);
  const double nan = __builtin_nan("");
  // one workspace, NaN before every star: the net's 2 H (1 + 5) doubles, the tangents' sums, dBC [5], dm [7], R [8], G [256], update_star's
  const size_t o_net = 0, o_dbct = o_net + 2 * h * (1 + sf::kMaxTan), o_dbc = o_dbct + sf::kMaxTan, o_dm = o_dbc + sf::kMaxTan, o_R = o_dm + sf::kMaxK,
               o_G = o_R + sf::kMaxK + 1, o_work = o_G + lm::kTileSize, o_row = o_work + lm::kWorkDoubles, o_end = o_row + sf::kMaxK;
  std::vector<double> ws(o_end);
  // ---- payne_sedfit_jac
  {
    sf::Plan all;
    sf::make_plan(photscale, (1u << P) - 1u, &all);
    std::vector<double> mags(b_n * f_n), dmags(b_n * f_n * P);
    for (size_t b = 0; b < b_n; ++b) {
      for (double& v : ws) v = nan;
      sf::Row r;
      sf::encode(pars.data() + b * P, photscale, N.xmin.data(), N.xden.data(), &r);
      sf::RowTerms t;
      sf::row_terms(photscale, pars.data() + b * P, &t);
      for (int f = 0; f < F; ++f) {
        filter_at(N, all, t, r, f, &ws[o_net], &ws[o_dbct], &ws[o_dbc], &mags[b * f_n + f], &ws[o_dm]);
        for (int p = 0; p < P; ++p) dmags[(b * f_n + f) * P + p] = ws[o_dm + p];
      }
    }
    write_bin(dir + "/mags.bin", mags.data(), mags.size());
    write_bin(dir + "/dmags.bin", dmags.data(), dmags.size());
  }
  if (free_mask == 0u) return 0;
  // ---- payne_sedfit_run
  sf::Plan pl;
  if (!sf::make_plan(photscale, free_mask, &pl)) {
    fprintf(stderr, "sedfit_emul: arguments the library rejects\n");
    return 3;
  }
  const int K = pl.K;
  const size_t k = (size_t)K;
  const std::vector<double> lo = read_bin<double>(dir + "/lo.bin", k), hi = read_bin<double>(dir + "/hi.bin", k);
  if (sf::check_run(photscale, free_mask, lo.data(), hi.data(), &o) != PAYNE_OK) {
    fprintf(stderr, "sedfit_emul: arguments the library rejects\n");
    return 3;
  }
  const std::vector<double> obs = read_bin<double>(dir + "/obs.bin", b_n * f_n), w = read_bin<double>(dir + "/w.bin", b_n * f_n);
  std::vector<double> mu, sigma;
  if (has_prior) {
    mu = read_bin<double>(dir + "/mu.bin", b_n * k);
    sigma = read_bin<double>(dir + "/sigma.bin", b_n * k);
  }
  lm::Box box;
  for (int i = 0; i < lm::kMaxK; ++i) {
    box.lo[i] = i < K ? lo[i] : 0.0;
    box.hi[i] = i < K ? hi[i] : 1.0;
  }
  const size_t rec = (size_t)P + 1 + k * k + 4;
  std::vector<double> G0(b_n * lm::kTileSize, 0.0), out(b_n * rec);
  for (size_t b = 0; b < b_n; ++b) {
    for (double& v : ws) v = nan;
    // the star's state, as the kernel holds it in LDS: arrays of exactly one star
    std::vector<double> xb(k, nan), xt(k, nan), A(k * k, nan), g(k, nan), chisq(1, nan), lambda(1, nan);
    std::vector<int> status(1, -1), niter(1, -1);
    std::vector<unsigned> at_bound(1, 0u);
    const lm::State st{xb.data(), xt.data(), A.data(), g.data(), chisq.data(), lambda.data(), status.data(), niter.data(), at_bound.data()};
    double* row = &ws[o_row];
    for (int p = 0; p < P; ++p) row[p] = pars[b * P + p];
    for (int i = 0; i < K; ++i) xb[i] = row[pl.par[i]];
    lm::begin_star(st, 0, K, xb.data(), box, o.lambda0);
    const double* sg = has_prior ? sigma.data() + b * k : nullptr;
    const double* m0 = has_prior ? mu.data() + b * k : nullptr;
    const int nf = sf::count_filters(w.data() + b * f_n, F);
    if (sf::too_few(nf, K, sg)) {
      status[0] = PAYNE_SEDFIT_TOO_FEW;
      chisq[0] = nan;
    }
    double* G = &ws[o_G];
    for (int eval = 0; eval < o.maxiter; ++eval) {
      if (status[0] != PAYNE_LMFIT_RUNNING) break;
      for (int e = 0; e < sf::tile_doubles(K); ++e) G[e] = 0.0;
      for (int i = 0; i < K; ++i) row[pl.par[i]] = xt[i];
      sf::Row r;
      sf::encode(row, photscale, N.xmin.data(), N.xden.data(), &r);
      sf::RowTerms t;
      sf::row_terms(photscale, row, &t);
      for (int f = 0; f < F; ++f) {
        double m;
        filter_at(N, pl, t, r, f, &ws[o_net], &ws[o_dbct], &ws[o_dbc], &m, &ws[o_dm]);
        const double wf = w[b * f_n + f];
        sf::residual_row(pl, m, &ws[o_dm], wf != 0.0 ? obs[b * f_n + f] : 0.0, &ws[o_R]);
        if (wf != 0.0)
          for (int i = 0; i <= K; ++i)
            for (int j = 0; j <= K; ++j) G[i * lm::kTile + j] = sf::tile_add(G[i * lm::kTile + j], ws[o_R + i], ws[o_R + j], wf);
      }
      sf::add_priors(G, K, xt.data(), m0, sg);
      if (eval == 0)
        for (int e = 0; e < sf::tile_doubles(K); ++e) G0[b * lm::kTileSize + e] = G[e];
      lm::update_star(st, 0, K, G, o, box, &ws[o_work]);
    }
    for (int i = 0; i < K; ++i) row[pl.par[i]] = xb[i];
    double* rec_b = out.data() + b * rec;
    for (int p = 0; p < P; ++p) rec_b[p] = row[p];
    rec_b[P] = chisq[0];
    for (size_t e = 0; e < k * k; ++e) rec_b[P + 1 + e] = A[e];
    rec_b[P + 1 + k * k] = (double)status[0];
    rec_b[P + 2 + k * k] = (double)niter[0];
    rec_b[P + 3 + k * k] = (double)at_bound[0];
    rec_b[P + 4 + k * k] = (double)nf;
  }
  write_bin(dir + "/G0.bin", G0.data(), G0.size());
  write_bin(dir + "/fit.bin", out.data(), out.size());
  return 0;
}
