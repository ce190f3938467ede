"""Payne.predict.photANN_new (the photometric LayerNorm + SiLU networks MLP_v0 / MLP_v1) -- what runs without a GPU: the import
names, the loader, a numpy fp64 restatement of the forward pass tied to the reference by tests/golden/g18_lnmlp.npz, and the
kernel's per-row arithmetic (csrc/lnmlp_core.hpp) executed on the host under ASan / UBSan.  The kernel itself and the classes
on the device: tests/test_lnmlp_gpu.py, which shares the helpers defined here.

g18_lnmlp.npz: MLP_v0(5, 40, 72, 33, 3) and MLP_v1(6, 64, 32, 96, 8) of the reference's NNmodels_new.py in eval(), every
LayerNorm gain and bias perturbed by N(0, 0.3); x = 257 rows of N(0, 1.5) (MLP_v0 reads its first five columns); y32 = the
module as it is on x.float(), y64 = the same module in .double() on those same fp32 values, dev = max|y32 - y64|."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G18 = {"v0": "MLP_v0", "v1": "MLP_v1"}
BOUND_FACTOR = 4.0                                   # max|y - y64| <= 4 x the fixture's dev: the margin for another summation order


def g18_net(g, name):
    """One network of the fixture as a file's arrays (+ labels and norms, which the fixture does not hold), its x, y64, dev."""
    arrs = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/model/")}
    d_in = arrs["model/mlp.lin1.weight"].shape[1]
    out_name = "lin6" if name == "v0" else "linout"
    d_out = arrs["model/mlp.%s.bias" % out_name].shape[0]
    rng = np.random.default_rng(18)
    arrs["label_i"] = np.array([("in%d" % i).encode() for i in range(d_in)])
    arrs["label_o"] = np.array([("band%d" % i).encode() for i in range(d_out)])
    for i in range(d_in):
        arrs["norm_i/in%d" % i] = np.array([rng.normal(0, 2.0), rng.uniform(0.5, 3.0)])
    for i in range(d_out):
        arrs["norm_o/band%d" % i] = np.array([rng.normal(5.0, 3.0), rng.uniform(0.5, 4.0)])
    return arrs, np.ascontiguousarray(g["x"][:, :d_in]), g[name + "/y64"], float(g[name + "/dev"])


def layers_of(arrs, nntype):
    """[(W, b, gain | None, beta | None)] from the file's arrays, in the order of the reference's Sequential."""
    n_hidden, out_name = {"MLP_v0": (5, "lin6"), "MLP_v1": (3, "linout")}[nntype]
    k = lambda s: arrs["model/mlp." + s]
    out = [(k("lin%d.weight" % i), k("lin%d.bias" % i), k("ln%d.weight" % i), k("ln%d.bias" % i)) for i in range(1, n_hidden + 1)]
    return out + [(k(out_name + ".weight"), k(out_name + ".bias"), None, None)]


def forward64(layers, x):
    """The forward pass in numpy fp64: Linear, nn.LayerNorm (mean, biased variance about it, eps = 1e-5, gain, bias), SiLU
    z / (1 + exp(-z)); the last layer Linear only.  x: the fp32 values the network is given, [N, D_in]."""
    a = np.asarray(x, dtype=np.float32).astype(np.float64)
    for W, b, g, be in layers:
        z = a @ W.astype(np.float64).T + b.astype(np.float64)
        if g is None:
            return z
        mean = z.mean(axis=1, keepdims=True)
        var = ((z - mean) ** 2).mean(axis=1, keepdims=True)
        z = (z - mean) / np.sqrt(var + 1e-5) * g.astype(np.float64) + be.astype(np.float64)
        a = z / (1.0 + np.exp(-z))


def norm_in(x, norm_i):
    """ANN.eval's input normalisation: (x - mid) / std in fp64, then one rounding to fp32."""
    x = np.array(x, dtype=np.float64)
    for ii, n in enumerate(norm_i):
        x[:, ii] = (x[:, ii] - n[0]) / n[1]
    return x.astype(np.float32)


def norm_out(y32, norm_o):
    """ANN.eval's output normalisation: the fp32 y times std plus mid in fp64, stored to the fp32 array."""
    y = np.array(y32, dtype=np.float32)
    for ii, n in enumerate(norm_o):
        y[:, ii] = y[:, ii].astype(np.float64) * n[1] + n[0]
    return y


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lnmlp")


def test_reference_import_names_resolve_to_this_build():
    import Payne
    from Payne.predict.photANN_new import modpred, ANN, readNN
    import thepayne_amd.predict.photANN_new as pn
    assert Payne.predict.photANN_new is pn and modpred is pn.modpred and ANN is pn.ANN and readNN is pn.readNN
    import inspect
    sig = inspect.signature(modpred.__init__)
    assert list(sig.parameters)[1:4] == ["nnpath", "nntype", "norm"]
    assert sig.parameters["nntype"].default == "MLP_v0" and sig.parameters["norm"].default is False
    with pytest.raises(IOError, match="Must provide a path to the ANN model"):
        modpred()
    with pytest.raises(IOError, match="Must provide a path to the ANN model"):
        ANN()


def test_restatement_matches_the_reference_in_fp64(g18):
    """The numpy forward pass of this file against the reference's module in .double(): 1e-12 relative."""
    for name, nntype in G18.items():
        arrs, x, y64, dev = g18_net(g18, name)
        y = forward64(layers_of(arrs, nntype), x)
        assert y.shape == y64.shape == (257, arrs["label_o"].shape[0])
        assert np.abs(y - y64).max() <= 1e-12 * np.abs(y64).max(), name
        assert 1e-8 < dev / np.abs(y64).max() < 3e-6                 # an fp32 evaluation's distance, not zero and not a wrong net


def test_loader_infers_widths_and_checks_the_type(g18, tmp_path):
    from thepayne_amd import synth
    from thepayne_amd.predict import photANN_new as pn
    for name, nntype, dims in (("v0", "MLP_v0", (5, 40, 72, 33, 3)), ("v1", "MLP_v1", (6, 64, 32, 96, 8))):
        arrs = g18_net(g18, name)[0]
        m = pn.readNN(arrs, nntype)
        assert (m.D_in, m.H1, m.H2, m.H3, m.D_out) == dims and m.nntype == nntype
        assert len(m.layers) == (6 if nntype == "MLP_v0" else 4)
        assert m.layers[-1][2] is None and all(L[0].dtype == np.float32 for L in m.layers)
        with pytest.raises(KeyError):                               # lin6 / linout do not match the type asked for
            pn.readNN(arrs, "MLP_v1" if nntype == "MLP_v0" else "MLP_v0")
    with pytest.raises(ValueError):
        pn.readNN(arrs, "MLP")
    with pytest.raises(ValueError):
        pn.ANN(nnpath=arrs, nntype="CNN")
    # a synthetic file of either type, through the .npz container
    for nntype, n_lin in (("MLP_v0", 6), ("MLP_v1", 4)):
        path = str(tmp_path / (nntype + ".npz"))
        net = synth.phot_mlp(path, nntype=nntype, D_in=6, H=(24, 40, 17), D_out=5, seed=3)
        A = pn.ANN(nnpath=path, nntype=nntype, norm=True)
        assert (A.model.D_in, A.model.H1, A.model.H2, A.model.H3, A.model.D_out) == (6, 24, 40, 17, 5)
        assert len(A.model.layers) == n_lin and A.nnpath == path
        assert list(A.label_i) == ['teff', 'logg', 'feh', 'afe', 'av', 'rv'] and A.label_i.dtype.kind == "U"
        assert list(A.label_o) == synth.PHOT_FILTERS[:5]
        # the norms in label order, whatever order the file holds them in
        assert all(np.array_equal(n, net["norm_i/" + k]) for n, k in zip(A.norm_i, A.label_i)) and len(A.norm_i) == 6
        assert all(np.array_equal(n, net["norm_o/" + k]) for n, k in zip(A.norm_o, A.label_o)) and len(A.norm_o) == 5
        B = pn.ANN(nnpath=path, nntype=nntype)
        assert not hasattr(B, "norm_i") and not hasattr(B, "norm_o") and B.norm is False
        assert np.array_equal(pn.modpred(nnpath=path, nntype=nntype).modpararr, A.label_o)
    with pytest.raises(ValueError):
        synth.phot_mlp(nntype="MLP")


def test_eval_shapes_and_argument_unchanged(g18, monkeypatch):
    """eval's host side with the device pass replaced by the fp64 restatement: list, 1-D and 2-D inputs, squeezed fp32 out, the
    caller's array as it was; getPhot's keys and shapes."""
    from thepayne_amd.predict import photANN_new as pn
    arrs, x, y64, _ = g18_net(g18, "v1")
    layers = layers_of(arrs, "MLP_v1")
    seen = []

    def forward(self, xx):
        seen.append(np.array(xx))
        return forward64(layers, xx).astype(np.float32)
    monkeypatch.setattr(pn.LNMLP, "forward", forward)
    P = pn.modpred(nnpath=arrs, nntype="MLP_v1")
    x2 = x[:7].copy()
    y = P.pred(x2)
    assert y.dtype == np.float32 and y.shape == (7, 8) and np.array_equal(x2, x[:7])
    assert seen[-1].dtype == np.float64 and seen[-1].shape == (7, 6)
    assert np.array_equal(y, y64[:7].astype(np.float32))
    y1 = P.pred(list(x[3]))
    assert y1.shape == (8,) and np.array_equal(y1, y[3]) and seen[-1].shape == (1, 6)
    assert P.pred(x[3:4]).shape == (8,)                              # squeezed, as the reference's .squeeze()
    out = P.getPhot(x[3])
    assert list(out) == list(P.anns.label_i) + list(P.anns.label_o)
    assert all(np.ndim(v) == 0 for v in out.values()) and out["in2"] == x[3, 2] and out["band7"] == y[3, 7]
    out = P.getPhot(x2)
    assert list(out) == list(P.anns.label_i) + list(P.anns.label_o) and all(v.shape == (7,) for v in out.values())
    assert np.array_equal(out["in5"], x[:7, 5]) and np.array_equal(out["band0"], y[:, 0]) and np.array_equal(x2, x[:7])


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/lnmlp_emul.cpp built with the sanitizers; returns run(layers, x, ld_x, norm) -> y fp32 [N][D_out]."""
    build = tmp_path_factory.mktemp("lnmlp_emul")
    exe = str(build / "lnmlp_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "lnmlp_emul.cpp")],
                   check=True)
    count = [0]

    def run(layers, x, norm=None):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        with open(str(d / "net.txt"), "w") as f:
            f.write("%d\n" % len(layers) + "".join("%d %d\n" % (W.shape[1], W.shape[0]) for W, _, _, _ in layers))
        for l, (W, b, g, be) in enumerate(layers):
            for tag, a in (("w", W), ("b", b), ("g", g), ("be", be)):
                if a is not None:
                    np.ascontiguousarray(a, dtype=np.float32).tofile(str(d / ("%s%d.bin" % (tag, l))))
        np.ascontiguousarray(x, dtype=np.float64).tofile(str(d / "x.bin"))
        if norm is not None:
            ni, no = (np.asarray(n, dtype=np.float64) for n in norm)
            np.concatenate([ni[:, 0], ni[:, 1], no[:, 0], no[:, 1]]).tofile(str(d / "norm.bin"))
        res = subprocess.run([exe, str(d), str(x.shape[0]), str(x.shape[1]), str(int(norm is not None))], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        return np.fromfile(str(d / "y.bin"), dtype=np.float32).reshape(x.shape[0], layers[-1][0].shape[0])
    return run


@pytest.mark.parametrize("N", (1, 65))
def test_row_arithmetic_on_the_host(emul, g18, N):
    """lnmlp_core.hpp's row_forward (the kernel's order of sums, its stored weight order, its padding) against the reference in
    fp64, both networks: max|y - y64| <= 4 dev; x with padding columns that must not be read as inputs; norm = 1 equals the
    plain pass wrapped in the reference's fp64 arithmetic, bit for bit."""
    for name, nntype in G18.items():
        arrs, x, y64, dev = g18_net(g18, name)
        layers = layers_of(arrs, nntype)
        xp = np.full((N, x.shape[1] + 3), 1e30)
        xp[:, :x.shape[1]] = x[:N]
        y = emul(layers, xp)
        err = np.abs(y.astype(np.float64) - y64[:N]).max()
        print("emulator %s N=%d: max|y - y64| = %.3g = %.2f dev" % (name, N, err, err / dev))
        assert err <= BOUND_FACTOR * dev, (name, err / dev)
        ni = [arrs["norm_i/" + k.decode()] for k in arrs["label_i"]]
        no = [arrs["norm_o/" + k.decode()] for k in arrs["label_o"]]
        yn = emul(layers, x[:N], norm=(ni, no))
        plain = emul(layers, norm_in(x[:N], ni).astype(np.float64))
        assert np.array_equal(yn.view(np.uint32), norm_out(plain, no).view(np.uint32)), name
