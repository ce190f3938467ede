// specmlp_train_emul.cpp -- thepayne_amd/csrc/specmlp_train_core.hpp on the host: the forward, the loss and dY, the activations'
// backward, the chunked dA_last accumulation and the weight gradients of k_specmlp_train.hip in the kernels' tiles, chunks and
// orders, every buffer of exactly the size payne_specmlp_train_create allocates.  Built by tests/test_trainspec.py with
// -fsanitize=address,undefined as a program of its own.
//   specmlp_train_emul DIR N   reads DIR/net.txt ("n_layers act", then "n_in n_out" per layer; act 0 = LeakyReLU, 1 = sigmoid),
//        DIR/w<l>.bin (fp32 [n_out][n_in]), b<l>.bin (fp32 [n_out]), x.bin (fp32 [N][D_in], encoded rows), t.bin (fp32
//        [N][D_out]); writes loss.bin (fp64 [1], the sum of squares), y.bin (fp32 [N][D_out]) and the gradients G_w<l>.bin,
//        G_b<l>.bin (row-major fp32)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../thepayne_amd/csrc/specmlp_train_core.hpp"

using namespace payne;
namespace sp = payne::specmlp;

namespace {

template <class T> std::vector<T> read_bin(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n || fgetc(f) != EOF) {
    fprintf(stderr, "specmlp_train_emul: %s does not hold %zu elements\n", path.c_str(), n);
    exit(2);
  }
  fclose(f);
  return v;
}
template <class T> void write_bin(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "specmlp_train_emul: cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

// act[64][stride] times the stored weights -> act[64][npad] (+ bias): tile_product of k_specmlp_train.hip
void tile_product(float* act, int stride, const float* w, int KB, int npad, const float* bias, std::vector<float>& z) {
  for (int r = 0; r < sp::kTileRows; ++r) {
    float* a = act + (size_t)r * stride;
    for (int j = 0; j < npad; ++j) z[j] = bias ? sp::dot_packed(a, w, j, KB) + bias[j] : sp::dot_packed(a, w, j, KB);
    for (int j = 0; j < npad; ++j) a[j] = z[j];
  }
}

// payne_specmlp_hidden_kernel, one tile after the other
void hidden_forward(const sp::SpecNet& net, const float* x, int ld_x, int N) {
  const int stride = sp::hidden_stride(net, false), tiles = (N + sp::kTileRows - 1) / sp::kTileRows;
  std::vector<float> act((size_t)sp::kTileRows * stride), z((size_t)stride);
  for (int tile = 0; tile < tiles; ++tile) {
    const int row0 = tile * sp::kTileRows;
    for (float& v : act) v = 0.0f;
    const int d_in = net.L[0].n_in, K0 = sp::k_blocks(d_in) * sp::kKBlock, w0 = sp::pad32(d_in);
    for (int r = 0; r < sp::kTileRows; ++r)
      for (int k = 0; k < K0; ++k) {
        const float v = row0 + r < N && k < d_in ? x[(size_t)(row0 + r) * ld_x + k] : 0.0f;
        act[(size_t)r * stride + k] = v;
        net.L[0].a_in[(size_t)(row0 + r) * w0 + k] = v;
      }
    for (int l = 0; l + 1 < net.n_layers; ++l) {
      const sp::SpecLayer& L = net.L[l];
      const int npad = sp::pad32(L.n_out);
      tile_product(act.data(), stride, L.wp, sp::k_blocks(L.n_in), npad, L.vec, z);
      for (int r = 0; r < sp::kTileRows; ++r)
        for (int c = 0; c < sp::kParts; ++c)
          sp::row_act_forward(act.data() + (size_t)r * stride, c, L.n_out, net.act, net.L[l + 1].a_in + (size_t)(row0 + r) * npad);
    }
  }
}

// payne_specmlp_out_kernel: per (tile, chunk of 128 columns) the image of A_last, then of the chunk's dY
void output_layer(const sp::SpecNet& net, const float* t, int ld_t, float* y, int N) {
  const sp::SpecLayer& L = net.L[net.n_layers - 1];
  const int stride = sp::out_stride(net), tiles = (N + sp::kTileRows - 1) / sp::kTileRows, chunks = sp::out_chunks(L.n_out);
  const int npad = sp::pad32(L.n_out), kpad = sp::pad32(L.n_in), KB = sp::k_blocks(L.n_in);
  std::vector<float> act((size_t)sp::kTileRows * stride), stage((size_t)sp::kTileRows * stride);
  for (int tile = 0; tile < tiles; ++tile)
    for (int chunk = 0; chunk < chunks; ++chunk) {
      const int row0 = tile * sp::kTileRows;
      for (int r = 0; r < sp::kTileRows; ++r)
        for (int k = 0; k < kpad; ++k) act[(size_t)r * stride + k] = L.a_in[(size_t)(row0 + r) * kpad + k];
      // a thread's 32 elements first, the 256 threads in index order
      std::vector<double> part(sp::kThreads, 0.0);
      for (int tid = 0; tid < sp::kThreads; ++tid) {
        const int lane = tid % sp::kWave, wave = tid / sp::kWave, ct = chunk * sp::kWaves + wave;
        if (ct >= sp::col_tiles(L.n_out)) continue;
        const int col = ct * sp::kTile + (lane & 31), lc = wave * sp::kTile + (lane & 31);
        for (int h = 0; h < 2; ++h)
          for (int i = 0; i < 16; ++i) {
            const int r = h * sp::kTile + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), gr = row0 + r;
            float dy = 0.0f;
            if (col < L.n_out && gr < N) {
              const float yv = sp::dot_packed(act.data() + (size_t)r * stride, L.wp, col, KB) + L.vec[col];
              y[(size_t)gr * L.n_out + col] = yv;
              dy = sp::elem_loss_grad(yv, t[(size_t)gr * ld_t + col], sp::kLossGradScale, &part[tid]);
            }
            L.dz[(size_t)gr * npad + col] = dy;
            stage[(size_t)r * stride + lc] = dy;
          }
      }
      double s = 0.0;
      for (int tid = 0; tid < sp::kThreads; ++tid) s += part[tid];
      net.loss_slab[(size_t)tile * chunks + chunk] = s;
      for (int c = 0; c < sp::kOutChunk; ++c) {
        const int col = chunk * sp::kOutChunk + c;
        if (col >= L.n_out) continue;
        float sum = 0.0f;
        for (int r = 0; r < sp::kTileRows; ++r) sum += stage[(size_t)r * stride + c];
        L.slab[(size_t)tile * npad + col] = sum;
      }
    }
}

// payne_specmlp_back_kernel
void backward(const sp::SpecNet& net, int N) {
  const int stride = sp::hidden_stride(net, true), tiles = (N + sp::kTileRows - 1) / sp::kTileRows, nl = net.n_layers;
  std::vector<float> act((size_t)sp::kTileRows * stride), z((size_t)stride);
  for (int tile = 0; tile < tiles; ++tile) {
    const size_t row0 = (size_t)tile * sp::kTileRows;
    {
      const sp::SpecLayer& L = net.L[nl - 1];
      const int npad = sp::pad32(L.n_out), KB = sp::k_blocks(L.n_out), wpad = sp::pad32(L.n_in);
      std::vector<float> acc((size_t)sp::kTileRows * wpad, 0.0f);
      for (int c0 = 0; c0 < npad; c0 += sp::kBackChunk) {             // dY through the image, one chain across the chunks
        const int cw = npad - c0 < sp::kBackChunk ? npad - c0 : sp::kBackChunk;
        for (int r = 0; r < sp::kTileRows; ++r)
          for (int c = 0; c < cw; ++c) act[(size_t)r * stride + c] = L.dz[(row0 + r) * npad + c0 + c];
        const int kb0 = c0 / sp::kKBlock, nkb = KB - kb0 < cw / sp::kKBlock ? KB - kb0 : cw / sp::kKBlock;
        for (int r = 0; r < sp::kTileRows; ++r)
          for (int j = 0; j < wpad; ++j)
            acc[(size_t)r * wpad + j] = sp::dot_packed_range(act.data() + (size_t)r * stride, L.wt, j, kb0, kb0 + nkb, KB, acc[(size_t)r * wpad + j]);
      }
      for (int r = 0; r < sp::kTileRows; ++r)
        for (int j = 0; j < wpad; ++j) act[(size_t)r * stride + j] = acc[(size_t)r * wpad + j];
    }
    for (int l = nl - 2; l >= 0; --l) {
      const sp::SpecLayer& L = net.L[l];
      const int n = L.n_out, npad = sp::pad32(n);
      for (int r = 0; r < sp::kTileRows; ++r)
        for (int c = 0; c < sp::kParts; ++c)
          sp::row_act_backward(act.data() + (size_t)r * stride, net.L[l + 1].a_in + (row0 + r) * npad, c, n, net.act, L.dz + (row0 + r) * npad);
      for (int j = 0; j < n; ++j) {
        float sum = 0.0f;
        for (int r = 0; r < sp::kTileRows; ++r) sum += act[(size_t)r * stride + j];
        L.slab[(size_t)tile * npad + j] = sum;
      }
      if (l > 0) tile_product(act.data(), stride, L.wt, sp::k_blocks(L.n_out), sp::pad32(L.n_in), nullptr, z);
    }
  }
}

// payne_mlp_dw_kernel and the update kernel's slab sums (csrc/mlp_train_tail.hpp)
void gradients(const sp::SpecNet& net, int N) {
  const int tiles = (N + sp::kTileRows - 1) / sp::kTileRows, rows = tiles * sp::kTileRows;
  for (int l = 0; l < net.n_layers; ++l) {
    const sp::SpecLayer& L = net.L[l];
    const int npad = sp::pad32(L.n_out), kpad = sp::pad32(L.n_in);
    for (int n = 0; n < L.n_out; ++n)
      for (int k = 0; k < L.n_in; ++k) {
        float c[sp::kWaves] = {0.0f, 0.0f, 0.0f, 0.0f};                  // wave w: the 16-row groups w, w + 4, ...
        for (int r = 0; r < rows; ++r) {
          float& acc = c[(r / sp::kDwGroup) % sp::kWaves];
          acc = fmaf(L.dz[(size_t)r * npad + n], L.a_in[(size_t)r * kpad + k], acc);
        }
        L.gw[(size_t)n * L.n_in + k] = sp::combine_parts(c[0], c[1], c[2], c[3]);
      }
    for (int j = 0; j < L.n_out; ++j) {
      float g = 0.0f;
      for (int t = 0; t < tiles; ++t) g += L.slab[(size_t)t * npad + j];
      L.gvec[j] = g;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: specmlp_train_emul DIR N\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const int N = atoi(argv[2]);
  FILE* f = fopen((dir + "net.txt").c_str(), "r");
  sp::SpecNet net{};
  if (!f || fscanf(f, "%d %d", &net.n_layers, &net.act) != 2 || net.n_layers < 2 || net.n_layers > sp::kMaxLayers) return 2;
  if (net.act != sp::kActLeaky && net.act != sp::kActSigmoid) return 2;
  for (int l = 0; l < net.n_layers; ++l) {
    sp::SpecLayer& L = net.L[l];
    if (fscanf(f, "%d %d", &L.n_in, &L.n_out) != 2 || L.n_in < 1 || L.n_out < 1) return 2;
    if (L.n_out > (l + 1 == net.n_layers ? sp::kMaxOut : sp::kMaxWidth)) return 2;
  }
  fclose(f);
  if (net.L[0].n_in > sp::kMaxIn || N < 1) return 2;
  const size_t rows = (size_t)(N + sp::kTileRows - 1) / sp::kTileRows * sp::kTileRows, tiles = rows / sp::kTileRows;
  std::vector<std::vector<float>> keep;
  keep.reserve((size_t)net.n_layers * 16);                               // (the pointers below stay valid)
  auto floats = [&](size_t n) {
    keep.emplace_back(n, 0.0f);
    return keep.back().data();
  };
  for (int l = 0; l < net.n_layers; ++l) {
    sp::SpecLayer& L = net.L[l];
    const std::string id = std::to_string(l);
    const size_t nw = (size_t)L.n_in * L.n_out, npad = (size_t)sp::pad32(L.n_out), kpad = (size_t)sp::pad32(L.n_in);
    L.wm = floats(nw);
    L.gw = floats(nw);
    L.wp = floats(sp::packed_floats(L.n_in, L.n_out));
    L.wt = floats(sp::packed_floats(L.n_out, L.n_in));
    L.vec = floats(npad);
    L.gvec = floats(npad);
    if (l == 0) L.a_in = floats(rows * kpad);
    L.dz = floats(rows * npad);
    L.slab = floats(tiles * npad);
    if (l + 1 < net.n_layers) net.L[l + 1].a_in = floats(rows * npad);
    const std::vector<float> w = read_bin<float>(dir + "w" + id + ".bin", nw), b = read_bin<float>(dir + "b" + id + ".bin", (size_t)L.n_out);
    std::vector<float> tr(nw);
    for (int n = 0; n < L.n_out; ++n)
      for (int k = 0; k < L.n_in; ++k) {
        L.wm[(size_t)n * L.n_in + k] = w[(size_t)n * L.n_in + k];
        tr[(size_t)k * L.n_out + n] = w[(size_t)n * L.n_in + k];
      }
    sp::pack_weights(w.data(), L.n_in, L.n_out, L.wp);
    sp::pack_weights(tr.data(), L.n_out, L.n_in, L.wt);
    for (int j = 0; j < L.n_out; ++j) L.vec[j] = b[j];
  }
  const int d_in = net.L[0].n_in, d_out = net.L[net.n_layers - 1].n_out;
  std::vector<double> loss_slab(tiles * (size_t)sp::out_chunks(d_out));
  net.loss_slab = loss_slab.data();
  const std::vector<float> x = read_bin<float>(dir + "x.bin", (size_t)N * d_in), t = read_bin<float>(dir + "t.bin", (size_t)N * d_out);
  std::vector<float> y((size_t)N * d_out);

  hidden_forward(net, x.data(), d_in, N);
  output_layer(net, t.data(), d_out, y.data(), N);
  backward(net, N);
  gradients(net, N);

  double loss = 0.0;
  const size_t parts = (size_t)((N + sp::kTileRows - 1) / sp::kTileRows) * sp::out_chunks(d_out);
  for (size_t i = 0; i < parts; ++i) loss += loss_slab[i];
  write_bin(dir + "loss.bin", &loss, 1);
  write_bin(dir + "y.bin", y.data(), y.size());
  for (int l = 0; l < net.n_layers; ++l) {
    const std::string id = std::to_string(l);
    write_bin(dir + "G_w" + id + ".bin", net.L[l].gw, (size_t)net.L[l].n_in * net.L[l].n_out);
    write_bin(dir + "G_b" + id + ".bin", net.L[l].gvec, (size_t)net.L[l].n_out);
  }
  return 0;
}
