"""Payne.train.trainphot (training the photometric LayerNorm + SiLU networks) -- what runs without a GPU: a torch restatement of
the reference's training step tied to the reference by tests/golden/g19_trainphot.npz, the kernels' arithmetic
(csrc/lnmlp_train_core.hpp) executed on the host under ASan / UBSan (tests/emul/lnmlp_train_emul.cpp), the dropout mask's host
export, and TrainMod's host logic with the device trainer replaced by the restatement.  The kernels themselves:
tests/test_trainphot_gpu.py, which shares the helpers defined here.

Yardstick.  For a set of named tensors (gradients or parameters) the pooled deviation is
    E(a) = max over tensors T of max|a_T - a64_T| / max|a64_T|,
a64 being torch autograd / torch.optim.RAdam on the CPU in .double() on the same fp32 inputs.  Every bound is
    E(ours) <= BOUND_FACTOR x E(torch CPU fp32),
the factor of tests/test_lnmlp.py with its meaning: the margin for another summation order and nothing else.  Pooled because a
per-tensor ratio is not stable where torch's own deviation on a three-element bias happens to be tiny.

g19_trainphot.npz (tools/freeze_trainphot_golden.py): MLP_v0(5, 40, 72, 33, 3) and MLP_v1(6, 64, 32, 96, 8) of the reference's
NNmodels_new.py in train() with d1.p = 0, every LayerNorm gain and bias perturbed by N(0, 0.3); x, t: 257 rows fp32; at N = 257
the fp64 loss, every parameter's fp64 gradient and torch fp32's pooled deviation; a 12-step full-batch RAdam(lr = 1e-3)
trajectory: fp64 losses, final fp64 parameters, torch fp32's pooled deviations."""
import os
import subprocess

import numpy as np
import pytest

from test_lnmlp import BOUND_FACTOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = {"v0": "MLP_v0", "v1": "MLP_v1"}
TAGS = ("w", "b", "g", "be")


def names_of(nntype):
    n_hidden, out = {"MLP_v0": (5, "lin6"), "MLP_v1": (3, "linout")}[nntype]
    return [("lin%d" % i, "ln%d" % i) for i in range(1, n_hidden + 1)] + [(out, None)]


def layers_from(g, prefix, nntype):
    """[(W, b, gain | None, beta | None)] from the keys <prefix>mlp.<name>.{weight,bias} of a fixture."""
    k = lambda s: g[prefix + "mlp." + s]
    return [(k(lin + ".weight"), k(lin + ".bias"), k(lnm + ".weight") if lnm else None, k(lnm + ".bias") if lnm else None)
            for lin, lnm in names_of(nntype)]


def g19_net(g, name):
    """(initial layers, x [257, D_in], t [257, D_out]) of one fixture network."""
    layers = layers_from(g, name + "/model/", G19[name])
    return layers, np.ascontiguousarray(g["x"][:, :layers[0][0].shape[1]]), g[name + "/t"]


def flat(layers):
    """{'w0': W, 'b0': b, 'g0': gain, 'be0': beta, ...}: the named tensors the pooled deviation runs over."""
    return {"%s%d" % (tag, l): np.asarray(a) for l, L in enumerate(layers) for tag, a in zip(TAGS, L) if a is not None}


def pooled(a, a64):
    return max(float(np.abs(np.asarray(a[k], dtype=np.float64) - a64[k]).max() / np.abs(a64[k]).max()) for k in a64)


def drop_scale(mask, p):
    """What multiplies the block's output: the uint8 mask times 1 / (1 - p) in fp32, as lnmlp_train_core.hpp's drop_factor."""
    return mask.astype(np.float32) * (np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def restatement(layers, dtype, masks=None):
    """The reference's module restated: a torch Sequential built from the arrays, with an explicit multiply by masks[block]
    (fp32 [N, width], the scaled mask) where a dropout sits.  Returns (module, its parameters as [(W, b, gain, beta)])."""
    import torch

    class MaskMul(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = torch.as_tensor(m).to(dtype)

        def forward(self, a):
            return a * self.m
    mods, pars = [], []
    for l, (W, b, g, be) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
        lin.weight.data, lin.bias.data = torch.as_tensor(np.array(W)).to(dtype), torch.as_tensor(np.array(b)).to(dtype)
        mods.append(lin)
        if g is None:
            pars.append((lin.weight, lin.bias, None, None))
            continue
        ln = torch.nn.LayerNorm(W.shape[0]).to(dtype)
        ln.weight.data, ln.bias.data = torch.as_tensor(np.array(g)).to(dtype), torch.as_tensor(np.array(be)).to(dtype)
        mods += [ln, torch.nn.SiLU()]
        if masks is not None and masks.get(l) is not None:
            mods.append(MaskMul(masks[l]))
        pars.append((lin.weight, lin.bias, ln.weight, ln.bias))
    return torch.nn.Sequential(*mods), pars


def torch_loss_grads(layers, x, t, dtype, masks=None):
    """(loss, gradients as layers) of MSELoss(reduction='mean') by torch autograd on the CPU in `dtype`."""
    import torch
    model, pars = restatement(layers, dtype, masks)
    loss = torch.nn.MSELoss(reduction='mean')(model(torch.as_tensor(np.array(x)).to(dtype)), torch.as_tensor(np.array(t)).to(dtype))
    loss.backward()
    return loss.item(), [tuple(None if p is None else p.grad.numpy().copy() for p in L) for L in pars]


class TorchRadam(object):
    """torch.optim.RAdam(lr) on the CPU in `dtype`, fed gradients from outside: .step(grads as layers) -> parameters as layers."""

    def __init__(self, layers, dtype, lr=1e-3):
        import torch
        self.pars = [tuple(None if a is None else torch.nn.Parameter(torch.as_tensor(np.array(a)).to(dtype)) for a in L) for L in layers]
        self.opt = torch.optim.RAdam([p for L in self.pars for p in L if p is not None], lr=lr)
        self.dtype = dtype

    def step(self, grads):
        import torch
        for L, G in zip(self.pars, grads):
            for p, g in zip(L, G):
                if p is not None:
                    p.grad = torch.as_tensor(np.array(g)).to(self.dtype)
        self.opt.step()
        return [tuple(None if p is None else p.detach().numpy().copy() for p in L) for L in self.pars]


def loss_of_residuals(y32, t32):
    """The fp64 mean of the squares of the fp32 residuals y - t."""
    r = np.asarray(y32, dtype=np.float32) - np.asarray(t32, dtype=np.float32)
    return float(np.mean(r.astype(np.float64) ** 2))


def packed_slots(n_in, n_out):
    """Index into the forward's stored order (lnmlp_core.hpp's packed_index) of W[n][k], as an [n_out, n_in] array, and the
    stored copy's length."""
    KB, CT = (n_in + 7) // 8, (n_out + 31) // 32
    n, k = np.meshgrid(np.arange(n_out), np.arange(n_in), indexing="ij")
    lane = (n % 32) + 32 * ((k % 8) // 4)
    return (((n // 32) * KB + k // 8) * 64 + lane) * 4 + k % 4, CT * KB * 64 * 4


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_trainphot")


def test_reference_import_names_resolve_to_this_build():
    import Payne
    from Payne.train.trainphot import TrainMod, EarlyStopping, defmod
    import thepayne_amd.train.trainphot as tp
    assert Payne.train.trainphot is tp and TrainMod is tp.TrainMod and EarlyStopping is tp.EarlyStopping and defmod is tp.defmod
    m = defmod(6, 16, 24, 8, 5, NNtype="MLP_v1", seed=1)
    assert (m.D_in, m.H1, m.H2, m.H3, m.D_out) == (6, 16, 24, 8, 5) and len(m.layers) == 4
    assert np.all(m.layers[0][2] == 1) and np.all(m.layers[0][3] == 0)
    assert np.abs(m.layers[1][0]).max() <= 1 / 4.0 and np.abs(m.layers[1][1]).max() <= 1 / 4.0      # U(+-1/sqrt(16))
    assert len(defmod(6, 16, 24, 8, 5, NNtype="MLP_v0").layers) == 6


def test_restatement_matches_the_reference_in_fp64(g19):
    """This file's torch restatement against the reference's own modules in .double(): loss and every gradient to 1e-12."""
    import torch
    for name, nntype in G19.items():
        layers, x, t = g19_net(g19, name)
        loss, grads = torch_loss_grads(layers, x, t, torch.float64)
        assert abs(loss - float(g19[name + "/loss64"])) <= 1e-12 * loss, name
        want = flat(layers_from(g19, name + "/grad64/", nntype))
        got = flat(grads)
        assert sorted(got) == sorted(want)
        assert pooled(got, want) <= 1e-12, (name, pooled(got, want))
        l32, g32 = torch_loss_grads(layers, x, t, torch.float32)
        dev = pooled(flat(g32), want)
        print("%s: torch fp32's pooled deviation of the gradients %.3g (fixture %.3g)" % (name, dev, float(g19[name + "/grad_dev"])))
        assert 1e-9 < float(g19[name + "/grad_dev"]) < 1e-5


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/lnmlp_train_emul.cpp built with the sanitizers; run(layers, p per layer, x, t, steps, seed) -> the files it
    wrote, as a reader r(name, dtype)."""
    build = tmp_path_factory.mktemp("lnmlp_train_emul")
    exe = str(build / "lnmlp_train_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "lnmlp_train_emul.cpp")],
                   check=True)
    count = [0]

    def run(layers, p, x, t, steps, seed=0):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        with open(str(d / "net.txt"), "w") as f:
            f.write("%d\n" % len(layers) + "".join("%d %d %r\n" % (L[0].shape[1], L[0].shape[0], float(pp)) for L, pp in zip(layers, p)))
        for l, L in enumerate(layers):
            for tag, a in zip(TAGS, L):
                if a is not None:
                    np.ascontiguousarray(a, dtype=np.float32).tofile(str(d / ("%s%d.bin" % (tag, l))))
        np.ascontiguousarray(x, dtype=np.float32).tofile(str(d / "x.bin"))
        np.ascontiguousarray(t, dtype=np.float32).tofile(str(d / "t.bin"))
        res = subprocess.run([exe, str(d), str(x.shape[0]), str(steps), str(seed)], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])

        def read(name, dtype=np.float32):
            return np.fromfile(str(d / (name + ".bin")), dtype=dtype)

        def step_layers(kind, s):
            return [tuple(None if a is None else read("%s%d_%s%d" % (kind, s, tag, l)).reshape(a.shape) for tag, a in zip(TAGS, L))
                    for l, L in enumerate(layers)]
        read.layers = step_layers
        return read
    return run


def radam_isolated(layers, grads_per_step, params_per_step, what):
    """fp64 and fp32 torch RAdam driven by the given gradients: after every step E(ours) <= 4 E(torch fp32) on the parameters."""
    import torch
    o64, o32 = TorchRadam(layers, torch.float64), TorchRadam(layers, torch.float32)
    worst = 0.0
    for s, (G, P) in enumerate(zip(grads_per_step, params_per_step)):
        p64, p32 = flat(o64.step(G)), flat(o32.step(G))
        e, e32 = pooled(flat(P), p64), pooled(p32, p64)
        worst = max(worst, e / e32)
        print("%s RAdam step %d: E = %.3g = %.2f x torch fp32's %.3g" % (what, s + 1, e, e / e32, e32))
        assert e <= BOUND_FACTOR * e32, (what, s + 1, e / e32)
    return worst


@pytest.mark.parametrize("N", (1, 65))
def test_training_arithmetic_on_the_host(emul, g19, N):
    """lnmlp_train_core.hpp in the kernels' tiles and orders, both networks, dropout off: the loss is the fp64 mean of squares of
    its own fp32 residuals to N D_out 2^-52 relative; gradients within
    the pooled bound; 8 RAdam steps, each checked against fp64 RAdam on the emulator's own gradients (steps 5 -> 6 cross the
    rectification switch); the padding of both stored weight copies exactly zero afterwards."""
    import torch
    for name, nntype in G19.items():
        layers, x, t = g19_net(g19, name)
        x, t = x[:N], t[:N]
        r = emul(layers, [0.0] * len(layers), x, t, 8)
        loss = r("loss", np.float64)
        l64, g64 = torch_loss_grads(layers, x, t, torch.float64)
        l32, g32 = torch_loss_grads(layers, x, t, torch.float32)
        G0 = r.layers("G", 0)
        own = loss_of_residuals(r("y0").reshape(t.shape), t)
        print("emulator %s N=%d: loss %.17g, the fp64 mean of its fp32 residuals' squares %.17g; |L - L64| / L64 = %.3g (torch fp32 %.3g)"
              % (name, N, loss[0], own, abs(loss[0] - l64) / l64, abs(l32 - l64) / l64))
        assert abs(loss[0] - own) <= N * t.shape[1] * 2.0 ** -52 * own, (name, N)
        e, e32 = pooled(flat(G0), flat(g64)), pooled(flat(g32), flat(g64))
        print("emulator %s N=%d: gradients E = %.3g = %.2f x torch fp32's %.3g" % (name, N, e, e / e32, e32))
        assert e <= BOUND_FACTOR * e32, (name, N, e / e32)
        radam_isolated(layers, [r.layers("G", s) for s in range(8)], [r.layers("P", s) for s in range(8)], "emulator %s N=%d" % (name, N))
        last = r.layers("P", 7)
        for l, L in enumerate(last):
            n_out, n_in = L[0].shape
            for tag, W, shape in (("wp", L[0], (n_in, n_out)), ("wt", L[0].T, (n_out, n_in))):
                slots, size = packed_slots(*shape)
                stored = r("%s%d" % (tag, l))
                assert stored.shape == (size,)
                assert np.array_equal(stored[slots].view(np.uint32), np.ascontiguousarray(W).view(np.uint32)), (name, tag, l)
                pad = np.ones(size, dtype=bool)
                pad[slots.ravel()] = False
                assert np.all(stored[pad].view(np.uint32) == 0), (name, tag, l)


def test_dropout_gradients_on_the_host(emul, g19):
    """MLP_v0 with p = 0.3 behind block 3, N = 65: the emulator's gradients against the restatement multiplied by the mask the
    emulator dumped; and the dump equals payne_lnmlp_dropout_mask."""
    import torch
    from thepayne_amd.train import trainphot as tp
    layers, x, t = g19_net(g19, "v0")
    x, t = x[:65], t[:65]
    p = [0.0, 0.0, 0.3, 0.0, 0.0, 0.0]
    r = emul(layers, p, x, t, 1, seed=77)
    mask = r("mask2", np.uint8).reshape(65, layers[2][0].shape[0])
    assert np.array_equal(mask, tp.dropout_mask(77, 0, 2, 65, layers[2][0].shape[0], 0.3))
    masks = {2: drop_scale(mask, 0.3)}
    l64, g64 = torch_loss_grads(layers, x, t, torch.float64, masks)
    l32, g32 = torch_loss_grads(layers, x, t, torch.float32, masks)
    e, e32 = pooled(flat(r.layers("G", 0)), flat(g64)), pooled(flat(g32), flat(g64))
    print("emulator v0 p=0.3 N=65: gradients E = %.3g = %.2f x torch fp32's %.3g" % (e, e / e32, e32))
    assert e <= BOUND_FACTOR * e32, e / e32
    assert abs(r("loss", np.float64)[0] - l64) <= BOUND_FACTOR * max(abs(l32 - l64), 2.0 ** -24 * l64)


def test_dropout_mask_host_export():
    from thepayne_amd.train import trainphot as tp
    m = tp.dropout_mask(5, 3, 2, 257, 72, 0.3)
    assert m.dtype == np.uint8 and m.shape == (257, 72) and set(np.unique(m)) == {0, 1}
    assert np.array_equal(m, tp.dropout_mask(5, 3, 2, 257, 72, 0.3))                       # reproducible
    assert np.array_equal(m[:65, :40], tp.dropout_mask(5, 3, 2, 65, 40, 0.3))              # a function of (row, column), not of the shape
    for other in (tp.dropout_mask(5, 4, 2, 257, 72, 0.3), tp.dropout_mask(5, 3, 1, 257, 72, 0.3), tp.dropout_mask(6, 3, 2, 257, 72, 0.3)):
        assert 0.3 < np.mean(other != m) < 0.55                                            # another step, layer, seed: 2 p (1 - p) = 0.42
    n = m.size
    for p in (0.3, 0.01, 0.9):
        kept = tp.dropout_mask(5, 3, 2, 257, 72, p).mean()
        print("p = %.2f: kept %.4f, %.2f sigma" % (p, kept, (kept - (1 - p)) / np.sqrt(p * (1 - p) / n)))
        assert abs(kept - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n)
    assert np.all(tp.dropout_mask(5, 3, 2, 257, 72, 0.0) == 1)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            tp.dropout_mask(5, 3, 2, 4, 4, bad)


# ---- TrainMod's host logic, the device trainer replaced by the torch restatement on the CPU ----------------------------------
class CpuTrainer(object):
    """What thepayne_amd.train.trainphot.Trainer offers, by torch on the CPU in fp32 (dropout off)."""
    created = []

    def __init__(self, layers, dropout_p, lr=1e-3, seed=0, max_rows=2048, device=None, **kw):
        import torch
        self.model, self.pars = restatement(layers, torch.float32)
        self.opt = torch.optim.RAdam(self.model.parameters(), lr=lr)
        self.dropout_p, self.max_rows, self.steps, self.batch_rows = list(dropout_p), max_rows, 0, []
        CpuTrainer.created.append(self)

    def step(self, x, t, loss_out=None):
        import torch
        assert x.shape[0] <= self.max_rows
        loss = torch.nn.MSELoss(reduction='mean')(self.model(x), t)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        self.steps += 1
        self.batch_rows.append(x.shape[0])
        if loss_out is not None:
            loss_out[0] = loss.item()

    def loss(self, x, t, loss_out):
        import torch
        with torch.no_grad():
            loss_out[0] = torch.nn.MSELoss(reduction='mean')(self.model(x), t).item()

    def params(self):
        return [tuple(None if p is None else p.detach().numpy().copy() for p in L) for L in self.pars]

    def close(self):
        pass


@pytest.fixture()
def grid(tmp_path):
    from thepayne_amd import synth
    path = str(tmp_path / "grid.npz")
    arrays, label_o, teacher = synth.phot_grid(path, 1000, nntype="MLP_v1", H=(16, 16, 16), D_out=5, seed=4)
    return path, arrays, label_o


def test_trainmod_host_logic(grid, tmp_path, monkeypatch):
    from thepayne_amd import nnio
    from thepayne_amd.predict import photANN_new as pn
    from thepayne_amd.train import trainphot as tp
    monkeypatch.setattr(tp, "Trainer", CpuTrainer)
    path, arrays, label_o = grid
    out = str(tmp_path / "net.npz")
    kw = dict(modpath=path, label_o=label_o, NNtype="MLP_v1", H1=16, H2=24, H3=8, batchsize=100, numepochs=12, output=out,
              device="cpu", logplot=False, seed=3, parrange={"logg": [0.0, 6.0], "Teff": [0.0, 1.0]})
    T = tp.TrainMod(**kw)
    # normfactor: over the whole table, before the cut; the cut: logg only ('Teff' is not a label)
    pars = arrays["parameters"]
    assert T.normfactor["logg"] == [np.mean(pars["logg"]), np.std(pars["logg"])]
    assert T.normfactor["2MASS_J"] == [np.mean(arrays["2MASS"]["J"]), np.std(arrays["2MASS"]["J"])]
    n = int(np.sum((pars["logg"] >= 0.0) & (pars["logg"] <= 6.0)))
    assert 0 < n < 1000
    # the split: disjoint, the stated sizes
    n_test = int(np.rint(0.1 * n))
    n_train = int(np.rint(0.7 * (n - n_test)))
    assert (len(T.testind), len(T.trainind), len(T.validind)) == (n_test, n_train, n - n_test - n_train)
    allind = np.concatenate([T.testind, T.trainind, T.validind])
    assert len(np.unique(allind)) == n and np.all(pars["logg"][allind] >= 0.0)
    assert np.array_equal(T.testind, tp.TrainMod(**kw).testind) and not np.array_equal(T.testind, tp.TrainMod(**dict(kw, seed=4)).testind)
    xs, ys = T.set_data("train")
    assert xs.dtype == np.float32 and xs.shape == (n_train, 6) and ys.shape == (n_train, 5)
    want = ((pars["av"][T.trainind] - T.normfactor["av"][0]) / T.normfactor["av"][1]).astype(np.float32)
    assert np.array_equal(xs[:, 4], want)
    assert T.test_labelsin.shape == (6, n_test) and np.array_equal(T.test_labelsin[1], pars["logg"][T.testind].astype(np.float32))
    # epoch_order: a permutation, reproducible, another per epoch
    o0, o1 = T.epoch_order(0).numpy(), T.epoch_order(1).numpy()
    assert np.array_equal(np.sort(o0), np.arange(n_train)) and np.array_equal(o0, T.epoch_order(0).numpy()) and not np.array_equal(o0, o1)
    assert len(T.epoch_order(0, "valid")) == len(T.validind)
    # dryrun
    CpuTrainer.created.clear()
    model, trainer, elapsed = T.run(dryrun=True)
    assert isinstance(model, pn.LNMLP) and isinstance(trainer, CpuTrainer) and trainer.steps == 0 and elapsed.total_seconds() >= 0
    assert trainer.dropout_p == [0.0, 0.01, 0.0] and tp.TrainMod(**dict(kw, dropout=0)).dropout_p() == [0.0, 0.0, 0.0]
    assert tp.TrainMod(**dict(kw, NNtype="MLP_v0", dropout=0.2)).dropout_p() == [0.0, 0.0, 0.2, 0.0, 0.0]
    assert (model.H1, model.H2, model.H3) == (16, 24, 8)
    # a run: drop_last batches, the six curves, the file
    net = T.run()
    trainer = CpuTrainer.created[-1]
    nb = n_train // 100
    assert T.nbatches == nb and trainer.steps == 12 * nb and set(trainer.batch_rows) == {100}
    assert T.nvalid == len(T.validind) // 100
    assert len(T.batchloss_arr) == len(T.validloss_arr) == 12 and len(T.batchloss_std) == len(T.validloss_med) == 12
    rl = T.running_loss[-1]
    assert np.isclose(T.batchloss_arr[-1], rl.mean()) and np.isclose(T.batchloss_std[-1], rl.std() / nb) and np.isclose(T.batchloss_med[-1], np.median(rl) / nb)
    assert T.batchloss_arr[-1] < T.batchloss_arr[0] and T.validloss_arr[-1] < T.validloss_arr[0]
    arrs = nnio.load_arrays(out)
    want_keys = {"testlabels_in", "testlabels_out", "label_i", "label_o"} | {"norm_i/" + k for k in T.label_i} | {"norm_o/" + k for k in label_o}
    want_keys |= {"model/mlp.%s.%s" % (m, k) for m in ("lin1", "lin2", "lin3", "ln1", "ln2", "ln3", "linout") for k in ("weight", "bias")}
    assert set(arrs) == want_keys
    A = pn.ANN(nnpath=out, nntype="MLP_v1", norm=True)
    assert list(A.label_o) == label_o and np.array_equal(A.norm_o[0], T.normfactor[label_o[0]])
    assert all(np.array_equal(a, b) for La, Lb in zip(A.model.layers, trainer.params()) for a, b in zip(La, Lb) if a is not None)
    assert all(np.array_equal(a, b) for La, Lb in zip(net.layers, A.model.layers) for a, b in zip(La, Lb) if a is not None)
    # restartfile: starts from the file's parameters
    CpuTrainer.created.clear()
    model2, trainer2, _ = tp.TrainMod(**dict(kw, restartfile=out, output=str(tmp_path / "net2.npz"))).run(dryrun=True)
    assert all(np.array_equal(a, b) for La, Lb in zip(model2.layers, A.model.layers) for a, b in zip(La, Lb) if a is not None)
    assert all(np.array_equal(a, b) for La, Lb in zip(trainer2.params(), A.model.layers) for a, b in zip(La, Lb) if a is not None)


def test_early_stopping_on_a_scripted_sequence(grid, tmp_path, monkeypatch):
    """EarlyStopping(50, 1e-4) created once: improvements smaller than min_delta count as none, the 50th of them in a row stops
    the run -- which the reference's stopper, re-created every epoch, never does."""
    from thepayne_amd.train import trainphot as tp
    s = tp.EarlyStopping(patience=3, min_delta=1e-4, verbose=False)
    seq = [1.0, 0.9, 0.89995, 0.8999, 0.5, 0.6, 0.7, 0.8]
    assert [s.step(v) for v in seq] == [False, False, False, False, False, False, False, True]
    assert s.best_loss == 0.5 and s.counter == 3

    class Scripted(CpuTrainer):
        def loss(self, x, t, loss_out):
            loss_out[0] = 1.0 if self.steps > 2 * self.per_epoch else 2.0 - 0.5 * self.steps / self.per_epoch
    monkeypatch.setattr(tp, "Trainer", Scripted)
    path, arrays, label_o = grid
    T = tp.TrainMod(modpath=path, label_o=label_o, NNtype="MLP_v1", H1=8, H2=8, H3=8, batchsize=100, numepochs=200,
                    output=str(tmp_path / "n.npz"), device="cpu", logplot=False)
    Scripted.per_epoch = len(T.trainind) // 100
    T.run()
    # epochs 1, 2 improve (1.5, 1.0), epoch 3 on stay at 1.0: 50 epochs without improvement -> stops after epoch 52
    assert T.stopped_early and len(T.validloss_arr) == 52 and os.path.exists(T.outpath)
