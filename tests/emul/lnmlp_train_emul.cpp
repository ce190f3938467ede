// lnmlp_train_emul.cpp -- thepayne_amd/csrc/lnmlp_train_core.hpp on the host: the training step of k_lnmlp_train.hip (forward in
// training mode, loss, backward, weight gradients, RAdam, the three stored copies of the weights) in the kernels' tiles and
// orders, every buffer of exactly the size payne_lnmlp_train_create allocates.  Built by tests/test_trainphot.py with
// -fsanitize=address,undefined as a program of its own.
//   lnmlp_train_emul DIR N steps seed   reads DIR/net.txt ("n_layers", then "n_in n_out dropout_p" per layer), DIR/w<l>.bin
//        (fp32 [n_out][n_in]), b<l>.bin, and on every layer but the last g<l>.bin, be<l>.bin (fp32 [n_out]), x.bin (fp32
//        [N][D_in]), t.bin (fp32 [N][D_out]); takes `steps` full-batch RAdam(lr = 1e-3) steps and writes loss.bin (fp64
//        [steps], the loss before each update), y0.bin (fp32 [N][D_out], the first step's forward), for step s the gradients G<s>_{w,b,g,be}<l>.bin and the updated parameters
//        P<s>_{w,b,g,be}<l>.bin (row-major fp32), mask<l>.bin (uint8 [N][n_out], step 0) for every layer with a dropout, and
//        after the last step the stored copies wp<l>.bin, wt<l>.bin
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/lnmlp_train_core.hpp"

using namespace payne;
namespace ln = payne::lnmlp;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "lnmlp_train_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "lnmlp_train_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

// act[64][stride] times the stored weights -> act[64][npad] (+ bias): tile_product of k_lnmlp_train.hip
void tile_product(float* act, int stride, const float* w, int KB, int npad, const float* bias, std::vector<float>& z) {
  for (int r = 0; r < ln::kTileRows; ++r) {
    float* a = act + (size_t)r * stride;
    for (int j = 0; j < npad; ++j) z[j] = bias ? ln::dot_packed(a, w, j, KB) + bias[j] : ln::dot_packed(a, w, j, KB);
    for (int j = 0; j < npad; ++j) a[j] = z[j];
  }
}

// payne_lnmlp_train_kernel, one tile after the other
void forward_backward(const ln::TrainNet& net, const float* x, int ld_x, const float* t, int ld_t, int N, int train,
                      unsigned long long seed, unsigned long long step, float scale, float* y_out) {
  const int stride = ln::train_stride(net), nl = net.n_layers, tiles = (N + ln::kTileRows - 1) / ln::kTileRows;
  std::vector<float> act((size_t)ln::kTileRows * stride), z((size_t)stride);
  for (int tile = 0; tile < tiles; ++tile) {
    const int row0 = tile * ln::kTileRows;
    for (float& v : act) v = 0.0f;
    const int d_in = net.L[0].n_in, K0 = ln::k_blocks(d_in) * ln::kKBlock, w0 = ln::pad32(d_in);
    for (int r = 0; r < ln::kTileRows; ++r)
      for (int k = 0; k < K0; ++k) {
        const float v = row0 + r < N && k < d_in ? x[(size_t)(row0 + r) * ld_x + k] : 0.0f;
        act[(size_t)r * stride + k] = v;
        net.L[0].a_in[(size_t)(row0 + r) * w0 + k] = v;
      }
    for (int l = 0; l < nl; ++l) {
      const ln::TrainLayer& L = net.L[l];
      const int npad = ln::pad32(L.n_out), n = L.n_out;
      tile_product(act.data(), stride, L.wp, ln::k_blocks(L.n_in), npad, L.vec, z);
      if (l + 1 == nl) break;
      for (int r = 0; r < ln::kTileRows; ++r) {
        float* zr = act.data() + (size_t)r * stride;
        const size_t grow = (size_t)(row0 + r);
        float p[ln::kParts], q[ln::kParts];
        for (int c = 0; c < ln::kParts; ++c) p[c] = ln::partial_sum(zr, c, n);
        const float mean = ln::mean_of(ln::combine_parts(p[0], p[1], p[2], p[3]), n);
        for (int c = 0; c < ln::kParts; ++c) q[c] = ln::partial_sqdev(zr, c, n, mean);
        const float rstd = ln::rstd_of(ln::combine_parts(q[0], q[1], q[2], q[3]), n);
        L.rs[grow] = rstd;
        for (int c = 0; c < ln::kParts; ++c)
          ln::row_ln_silu_train(zr, c, n, mean, rstd, L.vec + npad, L.vec + 2 * npad, train ? L.p : 0.0f, ln::mask_stream(seed, step, l),
                                (int)grow, L.xh + grow * npad, net.L[l + 1].a_in + grow * npad);
      }
    }
    {
      const ln::TrainLayer& L = net.L[nl - 1];
      const int npad = ln::pad32(L.n_out), n = L.n_out;
      double acc = 0.0;
      for (int r = 0; r < ln::kTileRows; ++r) {
        float* yr = act.data() + (size_t)r * stride;
        if (row0 + r < N) {
          if (y_out)
            for (int j = 0; j < n; ++j) y_out[(size_t)(row0 + r) * n + j] = yr[j];
          acc += ln::row_loss_grad(yr, t + (size_t)(row0 + r) * ld_t, n, scale);
        } else {
          for (int j = 0; j < n; ++j) yr[j] = 0.0f;
        }
      }
      net.loss_slab[tile] = acc;
      if (!train) continue;
      for (int r = 0; r < ln::kTileRows; ++r)
        for (int j = 0; j < npad; ++j) L.dz[(size_t)(row0 + r) * npad + j] = act[(size_t)r * stride + j];
      for (int j = 0; j < n; ++j) {
        float sum = 0.0f;
        for (int r = 0; r < ln::kTileRows; ++r) sum += act[(size_t)r * stride + j];
        L.slab[((size_t)tile * 3 + 0) * npad + j] = sum;
      }
    }
    for (int l = nl - 1; l >= 1; --l) {
      const ln::TrainLayer& L = net.L[l];
      const ln::TrainLayer& P = net.L[l - 1];
      const int n = P.n_out, npad = ln::pad32(n);
      tile_product(act.data(), stride, L.wt, ln::k_blocks(L.n_out), ln::pad32(L.n_in), nullptr, z);
      std::vector<float> m1(ln::kTileRows), m2(ln::kTileRows);
      for (int r = 0; r < ln::kTileRows; ++r) {
        const size_t grow = (size_t)(row0 + r);
        float s1[ln::kParts], s2[ln::kParts];
        for (int c = 0; c < ln::kParts; ++c)
          ln::row_act_backward(act.data() + (size_t)r * stride, P.xh + grow * npad, P.vec + npad, P.vec + 2 * npad, c, n, P.p,
                               ln::mask_stream(seed, step, l - 1), (int)grow, &s1[c], &s2[c]);
        m1[r] = ln::mean_of(ln::combine_parts(s1[0], s1[1], s1[2], s1[3]), n);
        m2[r] = ln::mean_of(ln::combine_parts(s2[0], s2[1], s2[2], s2[3]), n);
      }
      for (int j = 0; j < n; ++j) {
        float sg = 0.0f, sb = 0.0f;
        for (int r = 0; r < ln::kTileRows; ++r) {
          const float du = act[(size_t)r * stride + j];
          sg = fmaf(du, P.xh[(size_t)(row0 + r) * npad + j], sg);
          sb += du;
        }
        P.slab[((size_t)tile * 3 + 1) * npad + j] = sg;
        P.slab[((size_t)tile * 3 + 2) * npad + j] = sb;
      }
      for (int r = 0; r < ln::kTileRows; ++r) {
        const size_t grow = (size_t)(row0 + r);
        for (int c = 0; c < ln::kParts; ++c)
          ln::row_ln_backward(act.data() + (size_t)r * stride, P.xh + grow * npad, P.vec + npad, c, n, P.rs[grow], m1[r], m2[r],
                              P.dz + grow * npad);
      }
      for (int j = 0; j < n; ++j) {
        float sum = 0.0f;
        for (int r = 0; r < ln::kTileRows; ++r) sum += act[(size_t)r * stride + j];
        P.slab[((size_t)tile * 3 + 0) * npad + j] = sum;
      }
    }
  }
}

// payne_mlp_dw_kernel and payne_mlp_update_kernel (csrc/mlp_train_tail.hpp)
void update(const ln::TrainNet& net, int N, const ln::RadamStep& rs) {
  const int tiles = (N + ln::kTileRows - 1) / ln::kTileRows, rows = tiles * ln::kTileRows;
  for (int l = 0; l < net.n_layers; ++l) {
    const ln::TrainLayer& L = net.L[l];
    const int npad = ln::pad32(L.n_out), kpad = ln::pad32(L.n_in);
    for (int n = 0; n < L.n_out; ++n)
      for (int k = 0; k < L.n_in; ++k) {
        float c[ln::kWaves] = {0.0f, 0.0f, 0.0f, 0.0f};                  // wave w: the 16-row groups w, w + 4, ...
        for (int r = 0; r < rows; ++r) {
          float& acc = c[(r / ln::kDwGroup) % ln::kWaves];
          acc = fmaf(L.dz[(size_t)r * npad + n], L.a_in[(size_t)r * kpad + k], acc);
        }
        L.gw[(size_t)n * L.n_in + k] = ln::combine_parts(c[0], c[1], c[2], c[3]);
      }
    for (int n = 0; n < L.n_out; ++n)
      for (int k = 0; k < L.n_in; ++k) {
        const size_t idx = (size_t)n * L.n_in + k;
        const float w = ln::radam_update(L.wm[idx], L.gw[idx], L.mw + idx, L.vw + idx, rs);
        L.wm[idx] = w;
        L.wp[ln::packed_at(n, k, L.n_in)] = w;
        L.wt[ln::packed_t_at(n, k, L.n_out)] = w;
      }
    for (int which = 0; which < (l + 1 == net.n_layers ? 1 : 3); ++which)
      for (int j = 0; j < L.n_out; ++j) {
        float g = 0.0f;
        for (int t = 0; t < tiles; ++t) g += L.slab[((size_t)t * 3 + which) * npad + j];
        const int o = which * npad + j;
        L.gvec[o] = g;
        L.vec[o] = ln::radam_update(L.vec[o], g, L.mvec + o, L.vvec + o, rs);
      }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: lnmlp_train_emul DIR N steps seed\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const int N = atoi(argv[2]), steps = atoi(argv[3]);
  const unsigned long long seed = strtoull(argv[4], nullptr, 10);
  FILE* f = fopen((dir + "net.txt").c_str(), "r");
  ln::TrainNet net{};
  if (!f || fscanf(f, "%d", &net.n_layers) != 1 || net.n_layers < 2 || net.n_layers > ln::kMaxLayers) return 2;
  for (int l = 0; l < net.n_layers; ++l) {
    ln::TrainLayer& L = net.L[l];
    if (fscanf(f, "%d %d %f", &L.n_in, &L.n_out, &L.p) != 3 || L.n_in < 1 || L.n_out < 1 || L.n_out > ln::kMaxWidth || L.p < 0.0f || L.p >= 1.0f)
      return 2;
  }
  fclose(f);
  if (net.L[0].n_in > ln::kMaxIn || N < 1 || steps < 1) return 2;
  const size_t rows = (size_t)(N + ln::kTileRows - 1) / ln::kTileRows * ln::kTileRows, tiles = rows / ln::kTileRows;
  std::vector<std::vector<float>> keep;
  keep.reserve((size_t)net.n_layers * 16);                               // (the pointers below stay valid)
  auto floats = [&](size_t n) {
    keep.emplace_back(n, 0.0f);
    return keep.back().data();
  };
  for (int l = 0; l < net.n_layers; ++l) {
    ln::TrainLayer& L = net.L[l];
    const std::string id = std::to_string(l);
    const size_t nw = (size_t)L.n_in * L.n_out, npad = (size_t)ln::pad32(L.n_out), kpad = (size_t)ln::pad32(L.n_in);
    L.wm = floats(nw);
    L.gw = floats(nw);
    L.mw = floats(nw);
    L.vw = floats(nw);
    L.wp = floats(ln::packed_floats(L.n_in, L.n_out));
    L.wt = floats(ln::packed_floats(L.n_out, L.n_in));
    L.vec = floats(3 * npad);
    L.gvec = floats(3 * npad);
    L.mvec = floats(3 * npad);
    L.vvec = floats(3 * npad);
    if (l == 0) L.a_in = floats(rows * kpad);
    L.xh = floats(rows * npad);
    L.rs = floats(rows);
    L.dz = floats(rows * npad);
    L.slab = floats(tiles * 3 * npad);
    if (l + 1 < net.n_layers) net.L[l + 1].a_in = floats(rows * npad);
    const std::vector<float> w = read_bin<float>(dir + "w" + id + ".bin", nw);
    std::vector<float> tr(nw);
    for (int n = 0; n < L.n_out; ++n)
      for (int k = 0; k < L.n_in; ++k) {
        L.wm[(size_t)n * L.n_in + k] = w[(size_t)n * L.n_in + k];
        tr[(size_t)k * L.n_out + n] = w[(size_t)n * L.n_in + k];
      }
    ln::pack_weights(w.data(), L.n_in, L.n_out, L.wp);
    ln::pack_weights(tr.data(), L.n_out, L.n_in, L.wt);
    const char* tags[3] = {"b", "g", "be"};
    for (int which = 0; which < (l + 1 == net.n_layers ? 1 : 3); ++which) {
      const std::vector<float> v = read_bin<float>(dir + tags[which] + id + ".bin", (size_t)L.n_out);
      for (int j = 0; j < L.n_out; ++j) L.vec[which * npad + j] = v[j];
    }
  }
  std::vector<double> loss_slab(tiles), loss((size_t)steps);
  net.loss_slab = loss_slab.data();
  const int d_in = net.L[0].n_in, d_out = net.L[net.n_layers - 1].n_out;
  const std::vector<float> x = read_bin<float>(dir + "x.bin", (size_t)N * d_in), t = read_bin<float>(dir + "t.bin", (size_t)N * d_out);

  for (int l = 0; l + 1 < net.n_layers; ++l)
    if (net.L[l].p > 0.0f) {
      std::vector<unsigned char> m((size_t)N * net.L[l].n_out);
      for (int r = 0; r < N; ++r)
        for (int c = 0; c < net.L[l].n_out; ++c) m[(size_t)r * net.L[l].n_out + c] = ln::keep(seed, 0, l, r, c, net.L[l].p) ? 1 : 0;
      write_bin(dir + "mask" + std::to_string(l) + ".bin", m.data(), m.size());
    }

  std::vector<float> y0((size_t)N * d_out);
  for (int s = 0; s < steps; ++s) {
    forward_backward(net, x.data(), d_in, t.data(), d_out, N, 1, seed, (unsigned long long)s, ln::loss_grad_scale(N, d_out),
                     s == 0 ? y0.data() : nullptr);
    double acc = 0.0;
    for (size_t i = 0; i < tiles; ++i) acc += loss_slab[i];
    loss[(size_t)s] = acc / ((double)N * (double)d_out);
    update(net, N, ln::radam_scalars(1e-3, 0.9, 0.999, 1e-8, s + 1));
    for (int l = 0; l < net.n_layers; ++l) {
      const ln::TrainLayer& L = net.L[l];
      const size_t npad = (size_t)ln::pad32(L.n_out);
      const std::string id = std::to_string(l), sp = std::to_string(s);
      write_bin(dir + "G" + sp + "_w" + id + ".bin", L.gw, (size_t)L.n_in * L.n_out);
      write_bin(dir + "P" + sp + "_w" + id + ".bin", L.wm, (size_t)L.n_in * L.n_out);
      const char* tags[3] = {"b", "g", "be"};
      for (int which = 0; which < (l + 1 == net.n_layers ? 1 : 3); ++which) {
        write_bin(dir + "G" + sp + "_" + tags[which] + id + ".bin", L.gvec + which * npad, (size_t)L.n_out);
        write_bin(dir + "P" + sp + "_" + tags[which] + id + ".bin", L.vec + which * npad, (size_t)L.n_out);
      }
    }
  }
  write_bin(dir + "loss.bin", loss.data(), loss.size());
  write_bin(dir + "y0.bin", y0.data(), y0.size());
  for (int l = 0; l < net.n_layers; ++l) {
    const ln::TrainLayer& L = net.L[l];
    write_bin(dir + "wp" + std::to_string(l) + ".bin", L.wp, ln::packed_floats(L.n_in, L.n_out));
    write_bin(dir + "wt" + std::to_string(l) + ".bin", L.wt, ln::packed_floats(L.n_out, L.n_in));
  }
  return 0;
}
