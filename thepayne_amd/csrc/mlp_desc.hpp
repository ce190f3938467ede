// mlp_desc.hpp -- what the MLP entry points (mlp_api.hip) check and prepare on the host before anything touches the device: the
// descriptors' rules, the optimiser constants, and the two stored copies of a layer's weights.  Pure host code, no HIP calls, so
// that it also compiles into a stand-alone program (tests/test_mlp_desc.py, under ASan / UBSan).
// Every check takes the name of the entry point it serves and returns that entry point's code and message.  The checks come in
// the order the entry points apply them: the layers first, then whatever the caller checks of its own, then the limits.
#pragma once
#include <string>
#include <vector>

#include "../../include/payne_hip.h"
#include "specmlp_train_core.hpp"

namespace payne {
namespace mlp_desc {

struct Status {
  int code = PAYNE_OK;
  std::string msg;
  explicit operator bool() const { return code != PAYNE_OK; }       // true: refused
};
inline Status refuse(int code, const char* fn, const std::string& what) { return Status{code, std::string(fn) + ": " + what}; }

// n_layers, and per layer the widths, the chain of widths and the weight pointers, then the descriptor's own rule for the layer
template <class Desc, class LayerRule>
Status check_chain(const char* fn, const Desc* d, LayerRule&& rule) {
  if (d->n_layers < 2 || d->n_layers > lnmlp::kMaxLayers) return refuse(PAYNE_E_UNSUPPORTED, fn, "2 to 8 linear layers");
  for (int l = 0; l < d->n_layers; ++l) {
    const auto& L = d->layers[l];
    if (L.n_in < 1 || L.n_out < 1 || !L.w || !L.b || (l > 0 && L.n_in != d->layers[l - 1].n_out))
      return refuse(PAYNE_E_INVALID, fn, "layer " + std::to_string(l) + ": bad widths or null weights");
    if (Status s = rule(L, l + 1 == d->n_layers)) return s;
  }
  return Status{};
}

// A payne_lnmlp_desc: the layers, LayerNorm's vectors on every layer but the last, and the normalisations (both halves of each,
// or none at all where the caller takes normalised data).
inline Status check_lnmlp_layers(const char* fn, const payne_lnmlp_desc* d, bool norms_allowed) {
  const Status chain = check_chain(fn, d, [&](const payne_lnmlp_layer& L, bool last) {
    return (last ? (L.ln_gain || L.ln_bias) : (!L.ln_gain || !L.ln_bias))
               ? refuse(PAYNE_E_INVALID, fn, "LayerNorm gain and bias on every layer but the last") : Status{};
  });
  if (chain) return chain;
  if (norms_allowed) {
    if (!d->in_mid != !d->in_std || !d->out_mid != !d->out_std) return refuse(PAYNE_E_INVALID, fn, "a normalisation needs both mid and std");
  } else if (d->in_mid || d->in_std || d->out_mid || d->out_std) {
    return refuse(PAYNE_E_INVALID, fn, "training data arrive normalised; the descriptor must hold no norms");
  }
  return Status{};
}
inline Status check_lnmlp_limits(const char* fn, const payne_lnmlp_desc* d) {
  if (d->layers[0].n_in > lnmlp::kMaxIn) return refuse(PAYNE_E_UNSUPPORTED, fn, "more than 32 inputs");
  for (int l = 0; l < d->n_layers; ++l)
    if (d->layers[l].n_out > lnmlp::kMaxWidth) return refuse(PAYNE_E_UNSUPPORTED, fn, "a width above 512");
  return Status{};
}

// A payne_specmlp_desc: the layers and the activation; then the limits, of which the inputs' is the caller's (max_in of `in_noun`).
inline Status check_specmlp_layers(const char* fn, const payne_specmlp_desc* d) {
  if (Status s = check_chain(fn, d, [](const payne_specmlp_layer&, bool) { return Status{}; })) return s;
  if (d->act != PAYNE_SPECMLP_LEAKY && d->act != PAYNE_SPECMLP_SIGMOID)
    return refuse(PAYNE_E_INVALID, fn, "the activation is PAYNE_SPECMLP_LEAKY or PAYNE_SPECMLP_SIGMOID");
  return Status{};
}
inline Status check_specmlp_limits(const char* fn, const payne_specmlp_desc* d, int max_in, const char* in_noun) {
  if (d->layers[0].n_in > max_in) return refuse(PAYNE_E_UNSUPPORTED, fn, "more than " + std::to_string(max_in) + " " + in_noun);
  for (int l = 0; l + 1 < d->n_layers; ++l)
    if (d->layers[l].n_out > specmlp::kMaxWidth) return refuse(PAYNE_E_UNSUPPORTED, fn, "a hidden width above 512");
  if (d->layers[d->n_layers - 1].n_out > specmlp::kMaxOut) return refuse(PAYNE_E_UNSUPPORTED, fn, "more than 65536 outputs");
  return Status{};
}

// The workspace's rows and RAdam's constants of a training handle
inline Status check_optimiser(const char* fn, int max_rows, double lr, double beta1, double beta2, double eps) {
  if (max_rows < 1 || !(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
    return refuse(PAYNE_E_INVALID, fn, "max_rows < 1 or an optimiser constant out of range");
  return Status{};
}

// W [n_out][n_in] in the forward's stored order (packed_at) and W^T in the same order (packed_t_at): what a training handle keeps
// beside the row-major master copy.
inline void pack_both(const float* w, int n_in, int n_out, std::vector<float>& packed, std::vector<float>& packed_t) {
  std::vector<float> tr((size_t)n_in * (size_t)n_out);
  for (int n = 0; n < n_out; ++n)
    for (int k = 0; k < n_in; ++k) tr[(size_t)k * n_out + n] = w[(size_t)n * n_in + k];
  packed.assign(lnmlp::packed_floats(n_in, n_out), 0.0f);
  packed_t.assign(lnmlp::packed_floats(n_out, n_in), 0.0f);
  lnmlp::pack_weights(w, n_in, n_out, packed.data());
  lnmlp::pack_weights(tr.data(), n_out, n_in, packed_t.data());
}

}  // namespace mlp_desc
}  // namespace payne
