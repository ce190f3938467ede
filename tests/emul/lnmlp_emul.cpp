// lnmlp_emul.cpp -- thepayne_amd/csrc/lnmlp_core.hpp on the host: the network of payne_lnmlp_kernel (k_lnmlp.hip) one row at
// a time through row_forward, on weights stored by pack_weights in the kernel's order and on bias / LayerNorm vectors padded
// as payne_lnmlp_create pads them, every buffer of exactly the size the kernel is given.  Built by tests/test_lnmlp.py with
// -fsanitize=address,undefined as a program of its own (a sanitizer runtime wants to be the first thing a process loads):
//   lnmlp_emul DIR N ld_x norm   reads DIR/net.txt ("n_layers", then "n_in n_out" per layer), DIR/w<l>.bin (fp32
//                                [n_out][n_in]), b<l>.bin, and on every layer but the last g<l>.bin, be<l>.bin (fp32 [n_out]),
//                                x.bin (fp64 [N][ld_x]) and, with norm = 1, norm.bin (fp64: in_mid, in_std [D_in], out_mid,
//                                out_std [D_out]); writes y.bin (fp32 [N][D_out])
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/lnmlp_core.hpp"

using namespace payne;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "lnmlp_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}

std::vector<float> padded(const std::vector<float>& v, int n_pad) {
  std::vector<float> p((size_t)n_pad, 0.0f);
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: lnmlp_emul DIR N ld_x norm\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const int N = atoi(argv[2]), ld_x = atoi(argv[3]), norm = atoi(argv[4]);
  FILE* f = fopen((dir + "net.txt").c_str(), "r");
  lnmlp::NetArgs net{};
  if (!f || fscanf(f, "%d", &net.n_layers) != 1 || net.n_layers < 2 || net.n_layers > lnmlp::kMaxLayers) return 2;
  std::vector<std::vector<float>> keep;
  for (int l = 0; l < net.n_layers; ++l) {
    lnmlp::LayerArgs& L = net.L[l];
    if (fscanf(f, "%d %d", &L.n_in, &L.n_out) != 2 || L.n_in < 1 || L.n_out < 1 || L.n_out > lnmlp::kMaxWidth) return 2;
  }
  fclose(f);
  if (net.L[0].n_in > lnmlp::kMaxIn || N < 0 || ld_x < net.L[0].n_in) return 2;
  keep.reserve((size_t)net.n_layers * 4);                               // (the pointers below stay valid)
  for (int l = 0; l < net.n_layers; ++l) {
    lnmlp::LayerArgs& L = net.L[l];
    const std::string id = std::to_string(l);
    const int n_pad = lnmlp::col_tiles(L.n_out) * lnmlp::kTile;
    const std::vector<float> w = read_bin<float>(dir + "w" + id + ".bin", (size_t)L.n_in * L.n_out);
    keep.emplace_back(lnmlp::packed_floats(L.n_in, L.n_out));
    lnmlp::pack_weights(w.data(), L.n_in, L.n_out, keep.back().data());
    L.w = keep.back().data();
    keep.push_back(padded(read_bin<float>(dir + "b" + id + ".bin", (size_t)L.n_out), n_pad));
    L.b = keep.back().data();
    if (l + 1 < net.n_layers) {
      keep.push_back(padded(read_bin<float>(dir + "g" + id + ".bin", (size_t)L.n_out), n_pad));
      L.gain = keep.back().data();
      keep.push_back(padded(read_bin<float>(dir + "be" + id + ".bin", (size_t)L.n_out), n_pad));
      L.beta = keep.back().data();
    }
  }
  const int d_in = net.L[0].n_in, d_out = net.L[net.n_layers - 1].n_out;
  std::vector<double> nm;
  if (norm) {
    nm = read_bin<double>(dir + "norm.bin", (size_t)2 * d_in + (size_t)2 * d_out);
    net.in_mid = nm.data();
    net.in_std = nm.data() + d_in;
    net.out_mid = nm.data() + 2 * d_in;
    net.out_std = nm.data() + 2 * d_in + d_out;
  }
  const std::vector<double> x = read_bin<double>(dir + "x.bin", (size_t)N * ld_x);
  std::vector<float> y((size_t)N * d_out), buf((size_t)2 * lnmlp::act_stride(net));
  for (int i = 0; i < N; ++i) lnmlp::row_forward(net, x.data() + (size_t)i * ld_x, y.data() + (size_t)i * d_out, buf.data());
  FILE* o = fopen((dir + "y.bin").c_str(), "wb");
  if (!o || fwrite(y.data(), sizeof(float), y.size(), o) != y.size()) return 2;
  fclose(o);
  return 0;
}
