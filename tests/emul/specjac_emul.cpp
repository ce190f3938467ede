// specjac_emul.cpp -- thepayne_amd/csrc/specjac_core.hpp on the host: the two launches of payne_specjac_eval (k_specjac.hip) in the
// kernels' tiles, rows and orders, every buffer of exactly the size payne_specjac_create allocates.  Built by tests/test_specjac.py
// with -fsanitize=address,undefined as a program of its own.
//   specjac_emul DIR N FLAGS   reads DIR/net.txt ("n_layers act", then "n_in n_out" per layer; act 0 = LeakyReLU, 1 = sigmoid),
//        DIR/w<l>.bin (fp32 [n_out][n_in]), b<l>.bin (fp32 [n_out]), xmin.bin, xmax.bin (fp64 [D_in]), x.bin (fp64 [N][D_in], raw
//        labels); writes y.bin (fp32 [N][D_out]) and jac.bin (fp32 [N][D_in][D_out]; FLAGS = 1: PAYNE_JAC_ENCODED)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/specjac_core.hpp"

using namespace payne;
namespace sj = payne::specjac;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "specjac_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "specjac_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

// payne_specjac_hidden_kernel, one tile after the other
void hidden_launch(const sj::JacNet& net, const double* x, int ld_x, int N) {
  const int stride = sj::jac_hidden_stride(net), d_in = net.L[0].n_in, S = sj::stars_per_tile(d_in);
  const int kpad = sj::pad32(net.L[net.n_layers - 1].n_in);
  std::vector<float> act((size_t)sj::kTileRows * stride), z((size_t)stride);
  for (int tile = 0; tile < sj::tiles_of(N, d_in); ++tile) {
    const long long star0 = (long long)tile * S;
    for (float& v : act) v = -777.0f;                               // (what the image held before is never read)
    for (int r = 0; r < sj::kTileRows; ++r)
      for (int k = 0; k < sj::kKBlock; ++k) {
        const int m = r / S;
        const long long star = star0 + (r - m * S);
        act[(size_t)r * stride + k] = m <= d_in && star < N ? sj::input_value(m, k, d_in, x + (size_t)star * ld_x, net.xmin, net.xmax) : 0.0f;
      }
    for (int l = 0; l + 1 < net.n_layers; ++l) {
      const sj::JacLayer& L = net.L[l];
      const int npad = sj::pad32(L.n_out), KB = sj::k_blocks(L.n_in);
      for (int r = 0; r < sj::kTileRows; ++r) {                     // the product; the bias on the primal rows only
        float* a = act.data() + (size_t)r * stride;
        for (int j = 0; j < npad; ++j) z[j] = r < S ? sj::dot_packed(a, L.w, j, KB) + L.b[j] : sj::dot_packed(a, L.w, j, KB);
        for (int j = 0; j < npad; ++j) a[j] = z[j];
      }
      for (int s = 0; s < S; ++s)
        for (int j = 0; j < L.n_out; ++j)
          sj::unit_forward(act.data() + (size_t)s * stride + j, act.data() + (size_t)(S + s) * stride + j, S * stride, d_in, net.act);
    }
    for (int r = 0; r < sj::kTileRows; ++r)
      for (int c = 0; c < kpad; ++c) net.a_last[((size_t)tile * sj::kTileRows + r) * kpad + c] = act[(size_t)r * stride + c];
  }
}

// payne_specjac_out_kernel: per (tile, chunk of 128 columns) the image of A_last, a wave a column tile
void out_launch(const sj::JacNet& net, int N, float* y, int ld_y, float* jac, int ld_j) {
  const sj::JacLayer& L = net.L[net.n_layers - 1];
  const int stride = sj::jac_out_stride(net), d_in = net.L[0].n_in, kpad = sj::pad32(L.n_in), KB = sj::k_blocks(L.n_in);
  std::vector<float> act((size_t)sj::kTileRows * stride);
  for (int tile = 0; tile < sj::tiles_of(N, d_in); ++tile)
    for (int chunk = 0; chunk < sj::out_chunks(L.n_out); ++chunk) {
      for (int r = 0; r < sj::kTileRows; ++r)
        for (int k = 0; k < kpad; ++k) act[(size_t)r * stride + k] = net.a_last[((size_t)tile * sj::kTileRows + r) * kpad + k];
      for (int tid = 0; tid < sj::kThreads; ++tid) {
        const int lane = tid % sj::kWave, wave = tid / sj::kWave, ct = chunk * sj::kWaves + wave;
        const int col = ct * sj::kTile + (lane & 31);
        if (ct >= sj::col_tiles(L.n_out) || col >= L.n_out) continue;
        for (int h = 0; h < 2; ++h)
          for (int i = 0; i < 16; ++i) {
            const int r = h * sj::kTile + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            sj::store_output(sj::dot_packed(act.data() + (size_t)r * stride, L.w, col, KB), r, d_in, (long long)tile * sj::stars_per_tile(d_in),
                             N, col, L.b[col], net.scale, y, ld_y, jac, ld_j);
          }
      }
    }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: specjac_emul DIR N FLAGS\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int N = atoi(argv[2]);
  const unsigned flags = (unsigned)atoi(argv[3]);
  FILE* f = fopen((dir + "/net.txt").c_str(), "r");
  sj::JacNet net{};
  if (!f || fscanf(f, "%d %d", &net.n_layers, &net.act) != 2 || net.n_layers < 2 || net.n_layers > sj::kMaxLayers) {
    fprintf(stderr, "specjac_emul: bad net.txt\n");
    return 2;
  }
  std::vector<std::vector<float>> packed(net.n_layers), bias(net.n_layers);
  for (int l = 0; l < net.n_layers; ++l) {
    sj::JacLayer& L = net.L[l];
    if (fscanf(f, "%d %d", &L.n_in, &L.n_out) != 2 || L.n_in < 1 || L.n_out < 1) return 2;
    const std::vector<float> w = read_bin<float>(dir + "/w" + std::to_string(l) + ".bin", (size_t)L.n_in * L.n_out);
    const std::vector<float> b = read_bin<float>(dir + "/b" + std::to_string(l) + ".bin", (size_t)L.n_out);
    packed[l].assign(sj::packed_floats(L.n_in, L.n_out), 0.0f);
    sj::pack_weights(w.data(), L.n_in, L.n_out, packed[l].data());
    bias[l].assign((size_t)sj::pad32(L.n_out), 0.0f);
    for (int j = 0; j < L.n_out; ++j) bias[l][j] = b[j];
    L.w = packed[l].data();
    L.b = bias[l].data();
  }
  fclose(f);
  const int d_in = net.L[0].n_in, d_out = net.L[net.n_layers - 1].n_out;
  if (d_in > sj::kMaxLabels || N < 1) return 2;
  const std::vector<double> xmin = read_bin<double>(dir + "/xmin.bin", (size_t)d_in), xmax = read_bin<double>(dir + "/xmax.bin", (size_t)d_in);
  for (int k = 0; k < sj::kMaxLabels; ++k) {
    net.xmin[k] = k < d_in ? xmin[k] : 0.0;
    net.xmax[k] = k < d_in ? xmax[k] : 1.0;
    net.scale[k] = (flags & sj::kFlagEncoded) ? 1.0f : sj::label_scale(net.xmin[k], net.xmax[k]);
  }
  const std::vector<double> x = read_bin<double>(dir + "/x.bin", (size_t)N * d_in);
  std::vector<float> a_last((size_t)sj::tiles_of(N, d_in) * sj::kTileRows * sj::pad32(net.L[net.n_layers - 1].n_in), 0.0f);
  net.a_last = a_last.data();
  std::vector<float> y((size_t)N * d_out), jac((size_t)N * d_in * d_out);
  hidden_launch(net, x.data(), d_in, N);
  out_launch(net, N, y.data(), d_out, jac.data(), d_out);
  write_bin(dir + "/y.bin", y.data(), y.size());
  write_bin(dir + "/jac.bin", jac.data(), jac.size());
  return 0;
}
