"""csrc/mlp_desc.hpp, the host-side checks and weight packing of the MLP entry points (csrc/mlp_api.hip), built into a stand-alone
program with g++ -fsanitize=address,undefined and run on a table of descriptors: one good and one of every kind of bad per
descriptor type, through the checks in the order the entry point named applies them.  The codes and the message texts below
are the ones the entry points returned before the checks were shared; they are part of the ABI (payne_last_error)."""
import os
import subprocess

INVALID, UNSUPPORTED = -1, -2

# (case, entry point, code, message)
EXPECTED = [
    # payne_lnmlp_desc
    ("ln good", "payne_lnmlp_create", 0, ""),
    ("ln good with norms", "payne_lnmlp_create", 0, ""),
    ("ln null weight", "payne_lnmlp_create", INVALID, "payne_lnmlp_create: layer 1: bad widths or null weights"),
    ("ln mismatched widths", "payne_lnmlp_create", INVALID, "payne_lnmlp_create: layer 2: bad widths or null weights"),
    ("ln gain on the last layer", "payne_lnmlp_create", INVALID, "payne_lnmlp_create: LayerNorm gain and bias on every layer but the last"),
    ("ln hidden layer without gain", "payne_lnmlp_create", INVALID, "payne_lnmlp_create: LayerNorm gain and bias on every layer but the last"),
    ("ln mid without std", "payne_lnmlp_create", INVALID, "payne_lnmlp_create: a normalisation needs both mid and std"),
    ("ln std without mid on the output", "payne_lnmlp_create", INVALID, "payne_lnmlp_create: a normalisation needs both mid and std"),
    ("ln 9 layers", "payne_lnmlp_create", UNSUPPORTED, "payne_lnmlp_create: 2 to 8 linear layers"),
    ("ln 1 layer", "payne_lnmlp_create", UNSUPPORTED, "payne_lnmlp_create: 2 to 8 linear layers"),
    ("ln 33 inputs", "payne_lnmlp_create", UNSUPPORTED, "payne_lnmlp_create: more than 32 inputs"),
    ("ln width 513", "payne_lnmlp_create", UNSUPPORTED, "payne_lnmlp_create: a width above 512"),
    ("ln 65537 outputs", "payne_lnmlp_create", UNSUPPORTED, "payne_lnmlp_create: a width above 512"),
    ("lt good", "payne_lnmlp_train_create", 0, ""),
    ("lt norms present", "payne_lnmlp_train_create", INVALID,
     "payne_lnmlp_train_create: training data arrive normalised; the descriptor must hold no norms"),
    ("lt mid alone", "payne_lnmlp_train_create", INVALID,
     "payne_lnmlp_train_create: training data arrive normalised; the descriptor must hold no norms"),
    ("lt null weight", "payne_lnmlp_train_create", INVALID, "payne_lnmlp_train_create: layer 1: bad widths or null weights"),
    ("lt gain on the last layer", "payne_lnmlp_train_create", INVALID,
     "payne_lnmlp_train_create: LayerNorm gain and bias on every layer but the last"),
    ("lt 9 layers", "payne_lnmlp_train_create", UNSUPPORTED, "payne_lnmlp_train_create: 2 to 8 linear layers"),
    ("lt lr = 0", "payne_lnmlp_train_create", INVALID, "payne_lnmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("lt beta2 = 1", "payne_lnmlp_train_create", INVALID, "payne_lnmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("lt max_rows = 0", "payne_lnmlp_train_create", INVALID, "payne_lnmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("lt lr = 0 and 33 inputs", "payne_lnmlp_train_create", INVALID,
     "payne_lnmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("lt 33 inputs", "payne_lnmlp_train_create", UNSUPPORTED, "payne_lnmlp_train_create: more than 32 inputs"),
    ("lt width 513", "payne_lnmlp_train_create", UNSUPPORTED, "payne_lnmlp_train_create: a width above 512"),
    # payne_specmlp_desc
    ("st good", "payne_specmlp_train_create", 0, ""),
    ("st good sigmoid, 65536 outputs", "payne_specmlp_train_create", 0, ""),
    ("st null weight", "payne_specmlp_train_create", INVALID, "payne_specmlp_train_create: layer 1: bad widths or null weights"),
    ("st null bias", "payne_specmlp_train_create", INVALID, "payne_specmlp_train_create: layer 0: bad widths or null weights"),
    ("st mismatched widths", "payne_specmlp_train_create", INVALID, "payne_specmlp_train_create: layer 2: bad widths or null weights"),
    ("st 9 layers", "payne_specmlp_train_create", UNSUPPORTED, "payne_specmlp_train_create: 2 to 8 linear layers"),
    ("st 33 inputs", "payne_specmlp_train_create", UNSUPPORTED, "payne_specmlp_train_create: more than 32 inputs"),
    ("st width 513", "payne_specmlp_train_create", UNSUPPORTED, "payne_specmlp_train_create: a hidden width above 512"),
    ("st 65537 outputs", "payne_specmlp_train_create", UNSUPPORTED, "payne_specmlp_train_create: more than 65536 outputs"),
    ("st bad activation", "payne_specmlp_train_create", INVALID,
     "payne_specmlp_train_create: the activation is PAYNE_SPECMLP_LEAKY or PAYNE_SPECMLP_SIGMOID"),
    ("st lr = 0", "payne_specmlp_train_create", INVALID, "payne_specmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("st beta2 = 1", "payne_specmlp_train_create", INVALID, "payne_specmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("st max_rows = 0", "payne_specmlp_train_create", INVALID, "payne_specmlp_train_create: max_rows < 1 or an optimiser constant out of range"),
    ("sj good", "payne_specjac_create", 0, ""),
    ("sj 9 labels", "payne_specjac_create", UNSUPPORTED, "payne_specjac_create: more than 8 labels"),
    ("sj width 513", "payne_specjac_create", UNSUPPORTED, "payne_specjac_create: a hidden width above 512"),
    ("sj 65537 outputs", "payne_specjac_create", UNSUPPORTED, "payne_specjac_create: more than 65536 outputs"),
    ("sj bad activation", "payne_specjac_create", INVALID, "payne_specjac_create: the activation is PAYNE_SPECMLP_LEAKY or PAYNE_SPECMLP_SIGMOID"),
    ("sj 9 layers", "payne_specjac_create", UNSUPPORTED, "payne_specjac_create: 2 to 8 linear layers"),
]

MAIN = r'''
#include <cstdio>
#include <vector>
#include "thepayne_amd/csrc/mlp_desc.hpp"
using namespace payne;
namespace md = payne::mlp_desc;

static float F[4];                                   // what the pointers of a descriptor point at: the checks never read it
static double D8[8];

struct Opt { int max_rows; double lr, beta1, beta2, eps; };
static const Opt kOpt = {64, 1e-3, 0.9, 0.999, 1e-8};

static payne_lnmlp_desc ln_net(std::vector<int> dims) {
  payne_lnmlp_desc d{};
  d.n_layers = (int)dims.size() - 1;
  for (int l = 0; l + 1 < (int)dims.size() && l < PAYNE_LNMLP_MAX_LAYERS; ++l) {
    const bool hidden = l + 2 < (int)dims.size();
    d.layers[l] = payne_lnmlp_layer{dims[l], dims[l + 1], F, F, hidden ? F : nullptr, hidden ? F : nullptr};
  }
  return d;
}
static payne_specmlp_desc sp_net(std::vector<int> dims, int act = PAYNE_SPECMLP_LEAKY) {
  payne_specmlp_desc d{};
  d.n_layers = (int)dims.size() - 1;
  d.act = act;
  for (int l = 0; l + 1 < (int)dims.size() && l < PAYNE_LNMLP_MAX_LAYERS; ++l) {
    d.layers[l].n_in = dims[l];
    d.layers[l].n_out = dims[l + 1];
    d.layers[l].w = F;
    d.layers[l].b = F;
  }
  return d;
}

// the checks in the order of payne_lnmlp_create (opt == NULL) / payne_lnmlp_train_create
static md::Status ln_verdict(const char* fn, const payne_lnmlp_desc& d, const Opt* o) {
  if (md::Status s = md::check_lnmlp_layers(fn, &d, o == nullptr)) return s;
  if (o)
    if (md::Status s = md::check_optimiser(fn, o->max_rows, o->lr, o->beta1, o->beta2, o->eps)) return s;
  return md::check_lnmlp_limits(fn, &d);
}
// ... of payne_specmlp_train_create (opt != NULL) / payne_specjac_create
static md::Status sp_verdict(const char* fn, const payne_specmlp_desc& d, const Opt* o) {
  if (md::Status s = md::check_specmlp_layers(fn, &d)) return s;
  if (o) {
    if (md::Status s = md::check_optimiser(fn, o->max_rows, o->lr, o->beta1, o->beta2, o->eps)) return s;
    return md::check_specmlp_limits(fn, &d, specmlp::kMaxIn, "inputs");
  }
  return md::check_specmlp_limits(fn, &d, 8, "labels");
}
static void say(const char* name, const md::Status& s) { std::printf("%s\t%d\t%s\n", name, s.code, s.msg.c_str()); }

int main() {
  const char* lc = "payne_lnmlp_create";
  const char* lt = "payne_lnmlp_train_create";
  const char* st = "payne_specmlp_train_create";
  const char* sj = "payne_specjac_create";
  const std::vector<int> dims = {6, 40, 24, 8}, nine = {6, 8, 8, 8, 8, 8, 8, 8, 8, 8};
  payne_lnmlp_desc d = ln_net(dims);
  say("ln good", ln_verdict(lc, d, nullptr));
  d.in_mid = d.in_std = d.out_mid = d.out_std = D8;
  say("ln good with norms", ln_verdict(lc, d, nullptr));
  say("lt norms present", ln_verdict(lt, d, &kOpt));
  d = ln_net(dims); d.layers[1].w = nullptr;
  say("ln null weight", ln_verdict(lc, d, nullptr));
  say("lt null weight", ln_verdict(lt, d, &kOpt));
  d = ln_net(dims); d.layers[2].n_in = 23;
  say("ln mismatched widths", ln_verdict(lc, d, nullptr));
  d = ln_net(dims); d.layers[2].ln_gain = F;
  say("ln gain on the last layer", ln_verdict(lc, d, nullptr));
  say("lt gain on the last layer", ln_verdict(lt, d, &kOpt));
  d = ln_net(dims); d.layers[0].ln_gain = nullptr;
  say("ln hidden layer without gain", ln_verdict(lc, d, nullptr));
  d = ln_net(dims); d.in_mid = D8;
  say("ln mid without std", ln_verdict(lc, d, nullptr));
  say("lt mid alone", ln_verdict(lt, d, &kOpt));
  d = ln_net(dims); d.out_std = D8;
  say("ln std without mid on the output", ln_verdict(lc, d, nullptr));
  d = ln_net(nine);
  say("ln 9 layers", ln_verdict(lc, d, nullptr));
  say("lt 9 layers", ln_verdict(lt, d, &kOpt));
  say("ln 1 layer", ln_verdict(lc, ln_net({6, 8}), nullptr));
  say("ln 33 inputs", ln_verdict(lc, ln_net({33, 16, 8}), nullptr));
  say("lt 33 inputs", ln_verdict(lt, ln_net({33, 16, 8}), &kOpt));
  say("ln width 513", ln_verdict(lc, ln_net({6, 513, 8}), nullptr));
  say("lt width 513", ln_verdict(lt, ln_net({6, 513, 8}), &kOpt));
  say("ln 65537 outputs", ln_verdict(lc, ln_net({6, 16, 65537}), nullptr));
  say("lt good", ln_verdict(lt, ln_net(dims), &kOpt));
  Opt o = kOpt; o.lr = 0.0;
  say("lt lr = 0", ln_verdict(lt, ln_net(dims), &o));
  say("lt lr = 0 and 33 inputs", ln_verdict(lt, ln_net({33, 16, 8}), &o));
  say("st lr = 0", sp_verdict(st, sp_net(dims), &o));
  o = kOpt; o.beta2 = 1.0;
  say("lt beta2 = 1", ln_verdict(lt, ln_net(dims), &o));
  say("st beta2 = 1", sp_verdict(st, sp_net(dims), &o));
  o = kOpt; o.max_rows = 0;
  say("lt max_rows = 0", ln_verdict(lt, ln_net(dims), &o));
  say("st max_rows = 0", sp_verdict(st, sp_net(dims), &o));

  payne_specmlp_desc s = sp_net(dims);
  say("st good", sp_verdict(st, s, &kOpt));
  say("sj good", sp_verdict(sj, s, nullptr));
  say("st good sigmoid, 65536 outputs", sp_verdict(st, sp_net({32, 512, 65536}, PAYNE_SPECMLP_SIGMOID), &kOpt));
  s = sp_net(dims); s.layers[1].w = nullptr;
  say("st null weight", sp_verdict(st, s, &kOpt));
  s = sp_net(dims); s.layers[0].b = nullptr;
  say("st null bias", sp_verdict(st, s, &kOpt));
  s = sp_net(dims); s.layers[2].n_in = 25;
  say("st mismatched widths", sp_verdict(st, s, &kOpt));
  say("st 9 layers", sp_verdict(st, sp_net(nine), &kOpt));
  say("sj 9 layers", sp_verdict(sj, sp_net(nine), nullptr));
  say("st 33 inputs", sp_verdict(st, sp_net({33, 16, 8}), &kOpt));
  say("sj 9 labels", sp_verdict(sj, sp_net({9, 16, 8}), nullptr));
  say("st width 513", sp_verdict(st, sp_net({6, 513, 8}), &kOpt));
  say("sj width 513", sp_verdict(sj, sp_net({6, 513, 8}), nullptr));
  say("st 65537 outputs", sp_verdict(st, sp_net({6, 16, 65537}), &kOpt));
  say("sj 65537 outputs", sp_verdict(sj, sp_net({6, 16, 65537}), nullptr));
  say("st bad activation", sp_verdict(st, sp_net(dims, 2), &kOpt));
  say("sj bad activation", sp_verdict(sj, sp_net(dims, 2), nullptr));

  // the two stored copies of a 5 x 3 layer (n_out = 5, n_in = 3): every element where packed_at / packed_t_at say, zeros elsewhere
  int bad = 0;
  const int n_out = 5, n_in = 3;
  std::vector<float> w((size_t)n_out * n_in), pk, pt;
  for (size_t i = 0; i < w.size(); ++i) w[i] = 1.0f + (float)i;
  md::pack_both(w.data(), n_in, n_out, pk, pt);
  if (pk.size() != lnmlp::packed_floats(n_in, n_out) || pt.size() != lnmlp::packed_floats(n_out, n_in)) ++bad;
  std::vector<float> want_pk(pk.size(), 0.0f), want_pt(pt.size(), 0.0f);
  for (int n = 0; n < n_out; ++n)
    for (int k = 0; k < n_in; ++k) {
      want_pk.at(lnmlp::packed_at(n, k, n_in)) = w[(size_t)n * n_in + k];
      want_pt.at(lnmlp::packed_t_at(n, k, n_out)) = w[(size_t)n * n_in + k];
    }
  for (size_t i = 0; i < pk.size(); ++i) bad += pk[i] != want_pk[i];
  for (size_t i = 0; i < pt.size(); ++i) bad += pt[i] != want_pt[i];
  std::printf("pack bad=%d\n", bad);
  return bad != 0;
}
'''


def test_descriptor_checks_and_packing_under_address_and_ub_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = tmp_path / "main.cpp"
    main.write_text(MAIN)
    exe = tmp_path / "mlp_desc_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", root,
                    "-I", os.path.join(root, "include"), str(main), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "pack bad=0" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    got = {}
    for line in res.stdout.splitlines():
        if "\t" in line:
            name, code, msg = line.split("\t")
            assert name not in got, name
            got[name] = (int(code), msg)
    assert sorted(got) == sorted(name for name, _, _, _ in EXPECTED)
    for name, fn, code, msg in EXPECTED:
        assert got[name] == (code, msg), (name, got[name])
        assert code == 0 or msg.startswith(fn + ": ")
