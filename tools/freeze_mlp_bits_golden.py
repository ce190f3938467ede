#!/usr/bin/env python
"""Freeze the bits of the four MLP kernel families as tests/golden/g21_mlp_bits.npz: per case of the table below, the sha256 of
every result's bytes and its fp64 sum (for a readable failure message), obtained through the public ABI only.

Run on the MI355X with PAYNE_HIP_LIB pointing at a library built from a known-good commit (the one named on the command line):

    PAYNE_HIP_LIB=/path/to/known-good/libpayne_hip.so python tools/freeze_mlp_bits_golden.py <commit hash> [out.npz]

tests/test_mlp_bits_gpu.py runs the same table (CASES, run_case) on the tree's library and demands equal digests.  The inputs
come from np.random.default_rng seeds alone.  The shapes are the smallest that reach every form of the shared matrix product
(csrc/mlp_tile.hpp) and of the training tail (csrc/mlp_train_tail.hpp):
    hidden widths (40,), (256, 256, 256), (300, 300, 300): 1, 2 and 4 column tiles a wave; 40 has an odd number of k-blocks (5) and
        a ragged column tile; an input of 6 (or 4, or 1) is a single k-block
    N = 1, 65, 130: a lone row, one tile and a row, three tiles with a two-row tail; 200 rows through a workspace of 130: two passes
    payne_lnmlp_eval      D_in 6, D_out 8, with and without norms: y
    payne_lnmlp_train_*   dropout 0 on every width set and 0.3 on the first; max_rows 130; three steps at N = 130 and, on a second
                          handle, three at N = 65: the losses, PARAMS and GRADS after the third step, _train_loss on 200 rows
    payne_specmlp_train_* SMLP and LinNet, D_in 4, D_out 1100 (three chunks of dY in the backward, the last ragged; nine output
                          chunks); three steps at N = 130: the losses, PARAMS, GRADS, _train_predict on 200 rows
    payne_specjac_eval    D_in 1, 4, 8 (S = 32, 12, 7 stars a tile), hidden (40,) and (300, 300), D_out 300, both activations;
                          N = 1, S + 1, 2 S + 3 with max_rows = S + 1; flags 0 and PAYNE_JAC_ENCODED, with and without y: y, J
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g21_mlp_bits.npz")

WIDTHS = ((40,), (256, 256, 256), (300, 300, 300))
ROWS = (1, 65, 130)
MANY = 200                                           # rows of the calls that pass the 130-row workspace twice


def _cases():
    out = []
    for hw in WIDTHS:
        for norm in (False, True):
            out.append(("lnmlp_eval", dict(hidden=hw, norm=norm)))
    for hw in WIDTHS:
        for p in ((0.0, 0.3) if hw == WIDTHS[0] else (0.0,)):
            out.append(("lnmlp_train", dict(hidden=hw, p=p)))
    for kind in ("SMLP", "LinNet"):
        for hw in WIDTHS:
            out.append(("specmlp_train", dict(hidden=hw, kind=kind)))
    for d_in in (1, 4, 8):
        for hw in ((40,), (300, 300)):
            for kind in ("SMLP", "LinNet"):
                out.append(("specjac", dict(hidden=hw, kind=kind, d_in=d_in)))
    return out


CASES = _cases()


def case_id(case):
    fam, kw = case
    return fam + "/" + ",".join("%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in sorted(kw.items()))


def _seed(case):
    return int.from_bytes(hashlib.sha256(case_id(case).encode()).digest()[:4], "little")


def _net(rng, dims, layernorm):
    """[(W, b, gain | None, beta | None)] in fp32, nn.Linear's uniform initialisation; LayerNorm vectors about (1, 0)."""
    layers = []
    for i in range(len(dims) - 1):
        k = 1.0 / np.sqrt(dims[i])
        W = rng.uniform(-k, k, (dims[i + 1], dims[i])).astype(np.float32)
        b = rng.uniform(-k, k, dims[i + 1]).astype(np.float32)
        hidden = layernorm and i < len(dims) - 2
        layers.append((W, b, (1 + rng.normal(0, 0.3, dims[i + 1])).astype(np.float32) if hidden else None,
                       rng.normal(0, 0.3, dims[i + 1]).astype(np.float32) if hidden else None))
    return layers


def _ln_desc(layers, norm=None):
    from thepayne_amd import _lib
    d = _lib.LnmlpDesc()
    d.n_layers = len(layers)
    for i, (W, b, g, be) in enumerate(layers):
        L = d.layers[i]
        L.n_out, L.n_in = W.shape
        L.w, L.b = W.ctypes.data, b.ctypes.data
        L.ln_gain, L.ln_bias = (g.ctypes.data, be.ctypes.data) if g is not None else (None, None)
    if norm is not None:
        d.in_mid, d.in_std, d.out_mid, d.out_std = (a.ctypes.data for a in norm)
    return d


def _sp_desc(layers, kind):
    from thepayne_amd import _lib
    d = _lib.SpecmlpDesc()
    d.n_layers, d.act = len(layers), _lib.SPECMLP_SIGMOID if kind == "LinNet" else _lib.SPECMLP_LEAKY
    for i, L in enumerate(layers):
        d.layers[i].n_out, d.layers[i].n_in = L[0].shape
        d.layers[i].w, d.layers[i].b = L[0].ctypes.data, L[1].ctypes.data
    return d


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _flat(layers):
    return np.concatenate([a.ravel() for L in layers for a in L if a is not None])


def _run_lnmlp_eval(lib, rng, hidden, norm):
    import torch
    layers = _net(rng, (6,) + hidden + (8,), True)
    nv = None
    if norm:
        nv = [rng.normal(0, 1, 6), rng.uniform(0.5, 2, 6), rng.normal(0, 1, 8), rng.uniform(0.5, 2, 8)]
    x = rng.normal(0, 1.5, (max(ROWS), 6))
    h = C.c_void_p()
    assert lib.payne_lnmlp_create(0, C.byref(_ln_desc(layers, nv)), C.byref(h)) == 0
    res = {}
    try:
        x_d = _dev(x)
        for N in ROWS:
            y_d = torch.zeros((N, 8), dtype=torch.float32, device="cuda:0")
            assert lib.payne_lnmlp_eval(h, x_d.data_ptr(), 6, N, y_d.data_ptr(), 8, None) == 0
            res["y/N=%d" % N] = _host(y_d)
    finally:
        lib.payne_lnmlp_destroy(h)
    return res


def _train_run(lib, fam, create, layers, x, t, N, res, tag, extra):
    """Three steps at N on a fresh handle of max_rows 130: the losses, PARAMS and GRADS into res; then extra(h)."""
    import torch
    from thepayne_amd import _lib
    h = C.c_void_p()
    assert create(C.byref(h)) == 0
    step, get, destroy = (getattr(lib, "payne_%s_train_%s" % (fam, f)) for f in ("step", "get", "destroy"))
    try:
        x_d, t_d = _dev(x), _dev(t)
        loss_d = torch.zeros(3, dtype=torch.float64, device="cuda:0")
        for s in range(3):
            assert step(h, x_d.data_ptr(), x.shape[1], t_d.data_ptr(), t.shape[1], N, loss_d[s:].data_ptr(), None) == 0
        res[tag + "/losses"] = _host(loss_d)
        for what, name in ((_lib.LNMLP_PARAMS, "params"), (_lib.LNMLP_GRADS, "grads")):
            out = [tuple(None if a is None else np.zeros_like(a) for a in L) for L in layers]
            d = _ln_desc(out) if fam == "lnmlp" else _sp_desc(out, "SMLP")
            assert get(h, what, C.byref(d)) == 0
            res[tag + "/" + name] = _flat(out)
        if extra:
            extra(h)
    finally:
        destroy(h)


def _run_lnmlp_train(lib, rng, hidden, p):
    import torch
    from thepayne_amd import _lib
    layers = _net(rng, (6,) + hidden + (8,), True)
    x = rng.normal(0, 1.0, (MANY, 6)).astype(np.float32)
    t = rng.normal(0, 1.0, (MANY, 8)).astype(np.float32)
    o = _lib.LnmlpTrainOpts()
    o.lr, o.beta1, o.beta2, o.eps, o.seed, o.max_rows = 1e-3, 0.9, 0.999, 1e-8, 7, 130
    for i in range(len(hidden)):
        o.dropout_p[i] = p
    d = _ln_desc(layers)
    res = {}

    def loss_many(h):
        x_d, t_d = _dev(x), _dev(t)
        loss_d = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        assert lib.payne_lnmlp_train_loss(h, x_d.data_ptr(), 6, t_d.data_ptr(), 8, MANY, loss_d.data_ptr(), None) == 0
        res["loss/N=%d" % MANY] = _host(loss_d)
    create = lambda hp: lib.payne_lnmlp_train_create(0, C.byref(d), C.byref(o), hp)
    _train_run(lib, "lnmlp", create, layers, x, t, 130, res, "N=130", loss_many)
    _train_run(lib, "lnmlp", create, layers, x, t, 65, res, "N=65", None)
    return res


def _run_specmlp_train(lib, rng, hidden, kind):
    import torch
    from thepayne_amd import _lib
    d_out = 1100
    layers = [L[:2] for L in _net(rng, (4,) + hidden + (d_out,), False)]
    x = rng.uniform(-0.5, 0.5, (MANY, 4)).astype(np.float32)
    t = (1 + 0.1 * rng.normal(0, 1, (MANY, d_out))).astype(np.float32)
    o = _lib.SpecmlpTrainOpts()
    o.lr, o.beta1, o.beta2, o.eps, o.max_rows = 1e-4, 0.9, 0.999, 1e-8, 130
    d = _sp_desc(layers, kind)
    res = {}

    def predict_many(h):
        x_d = _dev(x)
        y_d = torch.zeros((MANY, d_out), dtype=torch.float32, device="cuda:0")
        assert lib.payne_specmlp_train_predict(h, x_d.data_ptr(), 4, MANY, y_d.data_ptr(), d_out, None) == 0
        res["predict/N=%d" % MANY] = _host(y_d)
    create = lambda hp: lib.payne_specmlp_train_create(0, C.byref(d), C.byref(o), hp)
    _train_run(lib, "specmlp", create, layers, x, t, 130, res, "N=130", predict_many)
    return res


def _run_specjac(lib, rng, hidden, kind, d_in):
    import torch
    from thepayne_amd import _lib
    d_out, S = 300, 64 // (1 + d_in)
    layers = [L[:2] for L in _net(rng, (d_in,) + hidden + (d_out,), False)]
    xmin, xmax = rng.uniform(-3, -1, d_in), rng.uniform(1, 3, d_in)
    x = rng.uniform(xmin, xmax, (2 * S + 3, d_in))
    h = C.c_void_p()
    assert lib.payne_specjac_create(0, C.byref(_sp_desc(layers, kind)), xmin.ctypes.data, xmax.ctypes.data, S + 1, C.byref(h)) == 0
    res = {}
    try:
        x_d = _dev(x)
        for N in (1, S + 1, 2 * S + 3):
            for flags in (0, _lib.JAC_ENCODED):
                for want_y in (True, False):
                    y_d = torch.zeros((N, d_out), dtype=torch.float32, device="cuda:0")
                    j_d = torch.zeros((N, d_in, d_out), dtype=torch.float32, device="cuda:0")
                    assert lib.payne_specjac_eval(h, x_d.data_ptr(), d_in, N, y_d.data_ptr() if want_y else None, d_out, j_d.data_ptr(), d_out,
                                                  flags, None) == 0
                    tag = "N=%d,flags=%d,y=%d" % (N, flags, want_y)
                    res["y/" + tag], res["jac/" + tag] = _host(y_d), _host(j_d)
    finally:
        lib.payne_specjac_destroy(h)
    return res


_RUN = {"lnmlp_eval": _run_lnmlp_eval, "lnmlp_train": _run_lnmlp_train, "specmlp_train": _run_specmlp_train, "specjac": _run_specjac}


def run_case(lib, case):
    """{result name: ndarray} of one case of CASES on the loaded library."""
    fam, kw = case
    return _RUN[fam](lib, np.random.default_rng(_seed(case)), **kw)


def digests(lib):
    """(keys, sha256 hex digests, fp64 sums) over all of CASES, in order."""
    keys, sha, sums = [], [], []
    for case in CASES:
        for name, a in run_case(lib, case).items():
            keys.append(case_id(case) + "::" + name)
            sha.append(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
            sums.append(float(np.sum(a, dtype=np.float64)))
    return keys, sha, sums


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch
    from thepayne_amd import _lib
    if len(sys.argv) < 2 or not os.environ.get("PAYNE_HIP_LIB"):
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    keys, sha, sums = digests(_lib.load())
    assert len(set(keys)) == len(keys) and all(np.isfinite(sums)), "duplicate keys or non-finite results"
    np.savez_compressed(out, keys=np.array(keys), sha256=np.array(sha), sums=np.array(sums, dtype=np.float64),
                        parent_commit=np.array(sys.argv[1]), rocm_version=np.array(str(torch.version.hip)))
    print("%d digests of %d cases from %s (commit %s, ROCm %s) -> %s" % (len(keys), len(CASES), os.environ["PAYNE_HIP_LIB"], sys.argv[1],
                                                                          torch.version.hip, out))
