"""Payne.train.trainspec (training the spectral networks SMLP and LinNet) -- what runs without a GPU: a torch restatement of the
reference's training step tied to the reference by tests/golden/g20_trainspec.npz, the kernels' arithmetic
(csrc/specmlp_train_core.hpp) executed on the host under ASan / UBSan (tests/emul/specmlp_train_emul.cpp), and TrainMod's host
logic with the device trainer replaced by the restatement.  The kernels themselves: tests/test_trainspec_gpu.py, which shares
the helpers defined here.

Yardstick: the project's (tests/test_trainphot.py).  For a set of named tensors the pooled deviation is
    E(a) = max over tensors T of max|a_T - a64_T| / max|a64_T|,
a64 being torch autograd / torch.optim.RAdam on the CPU in .double() on the same fp32 inputs, and every bound is
    E(ours) <= BOUND_FACTOR x E(torch CPU fp32).

g20_trainspec.npz (tools/freeze_trainspec_golden.py): SMLP(5, 40, 72, 33, 150) and LinNet(4, 48, 40, 56, 150) of the reference's
NNmodels.py; x: 130 encoded rows in [-0.5, 0.5), t = 1 + 0.1 N(0, 1); at N = 130 the fp64 MSELoss(reduction='sum'), every
parameter's fp64 gradient and torch fp32's pooled deviation; a 12-step full-batch RAdam(lr = 1e-4) trajectory: fp64 losses, final
fp64 parameters, torch fp32's pooled deviations.  The fp64 arrays are stored as byte planes (g20_array)."""
import os
import subprocess

import numpy as np
import pytest

from test_lnmlp import BOUND_FACTOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20 = {"smlp": "SMLP", "linnet": "LinNet"}
ACT = {"SMLP": 0, "LinNet": 1}
LR = 1e-4


def names_of(nntype):
    return ["features.%d" % i for i in (0, 2, 4, 6)] if nntype == "SMLP" else ["lin%d" % i for i in range(1, 7)]


def g20_array(g, key, base=None):
    """A fixture array: byte planes uint8 [4 | 8, *shape] back to fp32 / fp64 (XOR the bits of `base` in fp64, where the tool
    stored them so); anything else as it is."""
    a = g[key]
    if a.dtype != np.uint8:
        return a
    v = np.ascontiguousarray(np.moveaxis(a, 0, -1)).view(np.float32 if a.shape[0] == 4 else np.float64)[..., 0]
    if base is not None:
        v = (np.ascontiguousarray(v).view(np.uint64) ^ np.ascontiguousarray(base, dtype=np.float64).view(np.uint64)).view(np.float64)
    return np.ascontiguousarray(v)


def layers_from(g, prefix, nntype, base=None):
    """[(W, b)] from the keys <prefix><name>.{weight,bias} of the fixture."""
    return [tuple(g20_array(g, prefix + n + "." + k, None if base is None else base[l][i]) for i, k in enumerate(("weight", "bias")))
            for l, n in enumerate(names_of(nntype))]


def g20_net(g, name):
    """(initial layers, x fp32 [130, D_in], t fp32 [130, 150]) of one fixture network."""
    layers = layers_from(g, name + "/model/", G20[name])
    return layers, np.ascontiguousarray(g["x"][:, :layers[0][0].shape[1]].astype(np.float32)), g["t"].astype(np.float32)


def flat(layers):
    """{'w0': W, 'b0': b, ...}: the named tensors the pooled deviation runs over."""
    return {"%s%d" % (tag, l): np.asarray(a) for l, L in enumerate(layers) for tag, a in zip(("w", "b"), L)}


def pooled(a, a64):
    return max(float(np.abs(np.asarray(a[k], dtype=np.float64) - a64[k]).max() / np.abs(a64[k]).max()) for k in a64)


def restatement(layers, nntype, dtype):
    """The reference's module restated on encoded rows: a torch Sequential of Linear + LeakyReLU() (SMLP) or Linear + Sigmoid
    (LinNet) and a closing Linear, built from the arrays.  Returns (module, its parameters as [(W, b)])."""
    import torch
    mods, pars = [], []
    for l, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
        lin.weight.data, lin.bias.data = torch.as_tensor(np.array(W)).to(dtype), torch.as_tensor(np.array(b)).to(dtype)
        mods.append(lin)
        pars.append((lin.weight, lin.bias))
        if l + 1 < len(layers):
            mods.append(torch.nn.LeakyReLU() if nntype == "SMLP" else torch.nn.Sigmoid())
    return torch.nn.Sequential(*mods), pars


def torch_loss_grads(layers, nntype, x, t, dtype):
    """(loss, gradients as layers) of MSELoss(reduction='sum') by torch autograd on the CPU in `dtype`."""
    import torch
    model, pars = restatement(layers, nntype, dtype)
    loss = torch.nn.MSELoss(reduction='sum')(model(torch.as_tensor(np.array(x)).to(dtype)), torch.as_tensor(np.array(t)).to(dtype))
    loss.backward()
    return loss.item(), [tuple(p.grad.numpy().copy() for p in L) for L in pars]


def torch_predict(layers, nntype, x, dtype):
    import torch
    with torch.no_grad():
        return restatement(layers, nntype, dtype)[0](torch.as_tensor(np.array(x)).to(dtype)).numpy()


def torch_trajectory(layers, nntype, x, t, dtype, steps=12, lr=LR):
    import torch
    model, pars = restatement(layers, nntype, dtype)
    opt = torch.optim.RAdam(model.parameters(), lr=lr)
    xx, tt = torch.as_tensor(np.array(x)).to(dtype), torch.as_tensor(np.array(t)).to(dtype)
    losses = []
    for _ in range(steps):
        loss = torch.nn.MSELoss(reduction='sum')(model(xx), tt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses), [tuple(p.detach().numpy().copy() for p in L) for L in pars]


class TorchRadam(object):
    """torch.optim.RAdam(lr) on the CPU in `dtype`, fed gradients from outside: .step(grads as layers) -> parameters as layers."""

    def __init__(self, layers, dtype, lr=LR):
        import torch
        self.pars = [tuple(torch.nn.Parameter(torch.as_tensor(np.array(a)).to(dtype)) for a in L) for L in layers]
        self.opt = torch.optim.RAdam([p for L in self.pars for p in L], lr=lr)
        self.dtype = dtype

    def step(self, grads):
        import torch
        for L, G in zip(self.pars, grads):
            for p, g in zip(L, G):
                p.grad = torch.as_tensor(np.array(g)).to(self.dtype)
        self.opt.step()
        return [tuple(p.detach().numpy().copy() for p in L) for L in self.pars]


def radam_isolated(layers, grads_per_step, params_per_step, what):
    """fp64 and fp32 torch RAdam driven by the given gradients: after every step E(ours) <= 4 E(torch fp32) on the parameters."""
    import torch
    o64, o32 = TorchRadam(layers, torch.float64), TorchRadam(layers, torch.float32)
    for s, (G, P) in enumerate(zip(grads_per_step, params_per_step)):
        p64, p32 = flat(o64.step(G)), flat(o32.step(G))
        e, e32 = pooled(flat(P), p64), pooled(p32, p64)
        print("%s RAdam step %d: E = %.3g = %.2f x torch fp32's %.3g" % (what, s + 1, e, e / e32, e32))
        assert e <= BOUND_FACTOR * e32, (what, s + 1, e / e32)


def sum_of_squares(y32, t32):
    """The fp64 sum of the squares of the fp32 residuals y - t."""
    r = np.asarray(y32, dtype=np.float32) - np.asarray(t32, dtype=np.float32)
    return float(np.sum(r.astype(np.float64) ** 2))


def random_net(rng, dims):
    layers = []
    for i in range(len(dims) - 1):
        k = 1.0 / np.sqrt(dims[i])
        layers.append((rng.uniform(-k, k, (dims[i + 1], dims[i])).astype(np.float32), rng.uniform(-k, k, dims[i + 1]).astype(np.float32)))
    return layers


def random_batch(rng, N, d_in, d_out):
    return rng.uniform(-0.5, 0.5, (N, d_in)).astype(np.float32), (1.0 + 0.1 * rng.normal(0, 1, (N, d_out))).astype(np.float32)


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_trainspec")


def test_reference_import_names_resolve_to_this_build():
    import Payne
    from Payne.train.trainspec import TrainMod, defmod, slicebatch
    import thepayne_amd.train.trainspec as ts
    assert Payne.train.trainspec is ts and TrainMod is ts.TrainMod and defmod is ts.defmod and slicebatch is ts.slicebatch
    assert slicebatch(list(range(7)), 3) == [[0, 1, 2], [3, 4, 5], [6]]
    m = defmod(4, 16, 24, 8, 50, NNtype="SMLP", seed=1)
    assert sorted(m) == sorted("model/features.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias"))
    assert m["model/features.2.weight"].shape == (24, 16) and m["model/features.6.bias"].shape == (50,)
    assert np.abs(m["model/features.2.weight"]).max() <= 1 / 4.0 and np.abs(m["model/features.2.bias"]).max() <= 1 / 4.0   # U(+-1/sqrt(16))
    assert all(np.array_equal(a, b) for a, b in zip(m.values(), defmod(4, 16, 24, 8, 50, NNtype="SMLP", seed=1).values()))
    n = defmod(4, 16, 24, 8, 50, np.zeros(4), np.ones(4), NNtype="LinNet")
    assert [n["model/lin%d.weight" % i].shape for i in range(1, 7)] == [(16, 4), (16, 16), (24, 16), (24, 24), (8, 24), (50, 8)]
    assert np.array_equal(n["xmax"], np.ones(4))
    with pytest.raises(IOError):
        defmod(4, 16, 24, 8, 50, NNtype="ResNet")


def test_restatement_matches_the_reference_in_fp64(g20):
    """This file's torch restatement against the reference's own modules in .double(): the loss, every gradient, the 12-step loss
    curve and the final parameters to 1e-12 relative."""
    import torch
    for name, nntype in G20.items():
        layers, x, t = g20_net(g20, name)
        assert x.min() >= -0.5 and x.max() < 0.5 and x.shape[0] == t.shape[0] == 130 and t.shape[1] == 150
        loss, grads = torch_loss_grads(layers, nntype, x, t, torch.float64)
        assert abs(loss - float(g20[name + "/loss64"])) <= 1e-12 * loss, name
        want, got = flat(layers_from(g20, name + "/grad64/", nntype)), flat(grads)
        assert sorted(got) == sorted(want)
        assert pooled(got, want) <= 1e-12, (name, pooled(got, want))
        L64, p64 = torch_trajectory(layers, nntype, x, t, torch.float64)
        assert np.abs(L64 - g20[name + "/traj_loss64"]).max() <= 1e-12 * L64.max(), name
        final = flat(layers_from(g20, name + "/traj_final64/", nntype, base=layers))
        assert pooled(flat(p64), final) <= 1e-12, (name, pooled(flat(p64), final))
        g32 = torch_loss_grads(layers, nntype, x, t, torch.float32)[1]
        print("%s: torch fp32's pooled deviation of the gradients %.3g (fixture %.3g)" % (name, pooled(flat(g32), want), float(g20[name + "/grad_dev"])))
        for k in ("/grad_dev", "/traj_par_dev", "/traj_loss_dev"):
            assert 1e-10 < float(g20[name + k]) < 1e-5
        assert g20[name + "/traj_loss64"][-1] < g20[name + "/traj_loss64"][0]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/specmlp_train_emul.cpp built with the sanitizers; run(layers, nntype, x, t) -> (loss, y, gradients as layers)."""
    build = tmp_path_factory.mktemp("specmlp_train_emul")
    exe = str(build / "specmlp_train_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "specmlp_train_emul.cpp")],
                   check=True)
    count = [0]

    def run(layers, nntype, x, t):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        with open(str(d / "net.txt"), "w") as f:
            f.write("%d %d\n" % (len(layers), ACT[nntype]) + "".join("%d %d\n" % (W.shape[1], W.shape[0]) for W, b in layers))
        for l, (W, b) in enumerate(layers):
            np.ascontiguousarray(W, dtype=np.float32).tofile(str(d / ("w%d.bin" % l)))
            np.ascontiguousarray(b, dtype=np.float32).tofile(str(d / ("b%d.bin" % l)))
        np.ascontiguousarray(x, dtype=np.float32).tofile(str(d / "x.bin"))
        np.ascontiguousarray(t, dtype=np.float32).tofile(str(d / "t.bin"))
        res = subprocess.run([exe, str(d), str(x.shape[0])], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        read = lambda nm, dt=np.float32: np.fromfile(str(d / (nm + ".bin")), dtype=dt)
        grads = [(read("G_w%d" % l).reshape(W.shape), read("G_b%d" % l)) for l, (W, b) in enumerate(layers)]
        return read("loss", np.float64)[0], read("y").reshape(t.shape), grads
    return run


def check_emul(emul, what, layers, nntype, x, t, g64=None):
    import torch
    loss, y, grads = emul(layers, nntype, x, t)
    own = sum_of_squares(y, t)
    assert abs(loss - own) <= t.size * 2.0 ** -52 * own, what
    if g64 is None:
        g64 = torch_loss_grads(layers, nntype, x, t, torch.float64)[1]
    g32 = torch_loss_grads(layers, nntype, x, t, torch.float32)[1]
    e, e32 = pooled(flat(grads), flat(g64)), pooled(flat(g32), flat(g64))
    print("emulator %s: gradients E = %.3g = %.2f x torch fp32's %.3g" % (what, e, e / e32, e32))
    assert e <= BOUND_FACTOR * e32, (what, e / e32)
    y64, y32 = torch_predict(layers, nntype, x, torch.float64), torch_predict(layers, nntype, x, torch.float32)
    ey, ey32 = np.abs(y - y64).max() / np.abs(y64).max(), np.abs(y32 - y64).max() / np.abs(y64).max()
    print("emulator %s: y E = %.3g = %.2f x torch fp32's %.3g" % (what, ey, ey / ey32, ey32))
    assert ey <= BOUND_FACTOR * ey32, (what, ey / ey32)


@pytest.mark.parametrize("name", sorted(G20))
def test_training_arithmetic_on_the_host(emul, g20, name):
    """specmlp_train_core.hpp in the kernels' tiles, chunks and orders on the fixture: at N = 130 against the fixture's fp64
    gradients, at N = 1 and 65 against the restatement."""
    layers, x, t = g20_net(g20, name)
    check_emul(emul, "g20 %s N=130" % name, layers, G20[name], x, t, g64=layers_from(g20, name + "/grad64/", G20[name]))
    for N in (1, 65):
        check_emul(emul, "g20 %s N=%d" % (name, N), layers, G20[name], x[:N], t[:N])


@pytest.mark.parametrize("nntype", sorted(ACT))
def test_chunked_output_layer_on_the_host(emul, nntype):
    """D_out = 1100: nine 128-column chunks of the output layer, three 512-column chunks of the dA_last stream, both ragged."""
    rng = np.random.default_rng(1100)
    layers = random_net(rng, [4, 33, 40, 1100] if nntype == "SMLP" else [4, 20, 33, 40, 1100])
    x, t = random_batch(rng, 65, 4, 1100)
    check_emul(emul, "%s D_out=1100 N=65" % nntype, layers, nntype, x, t)


# ---- TrainMod's host logic, the device trainer replaced by the torch restatement on the CPU ----------------------------------
class CpuTrainer(object):
    """What thepayne_amd.train.trainspec.Trainer offers, by torch on the CPU in fp32."""
    created = []

    def __init__(self, layers, NNtype='SMLP', lr=1e-4, max_rows=512, device=None, **kw):
        import torch
        self.model, self.pars = restatement(layers, NNtype, torch.float32)
        self.opt = torch.optim.RAdam(self.model.parameters(), lr=lr)
        self.max_rows, self.steps, self.batch_rows, self.lrs = max_rows, 0, [], []
        CpuTrainer.created.append(self)

    def step(self, x, t, loss_out=None):
        import torch
        assert x.shape[0] <= self.max_rows
        loss = torch.nn.MSELoss(reduction='sum')(self.model(x), t)
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
            loss_out[0] = torch.nn.MSELoss(reduction='sum')(self.model(x), t).item()

    def set_lr(self, lr):
        self.lrs.append(lr)
        for gr in self.opt.param_groups:
            gr['lr'] = lr

    def params(self):
        return [tuple(p.detach().numpy().copy() for p in L) for L in self.pars]

    def close(self):
        pass


def test_trainmod_host_logic(tmp_path, monkeypatch):
    from thepayne_amd import nnio, synth
    from thepayne_amd.train import trainspec as ts
    path, out = str(tmp_path / "grid.npz"), str(tmp_path / "net.npz")
    arrays, teacher = synth.spec_grid(path, 400, kind="SMLP", npix=60, H=(8, 8, 8), seed=5)
    # the grid reader
    spectra, labels, names, wave = ts.read_grid(path)
    assert spectra.dtype == np.float32 and spectra.shape == (400, 60) and labels.shape == (400, 4) and names == ['teff', 'logg', 'feh', 'afe']
    assert np.array_equal(wave, teacher["wavelength"])
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, spectra=arrays["spectra"], labels=arrays["labels"])
    with pytest.raises(ValueError):
        ts.read_grid(bad)
    # keyword defaults: the reference's (trainspec.py:67-158)
    class Stop(Exception):
        pass

    def stop(self):
        raise Stop()
    monkeypatch.setattr(ts.TrainMod, "_read_grid", stop)                # (the keywords are taken before the grid is read)
    D = object.__new__(ts.TrainMod)
    with pytest.raises(Stop):
        D.__init__(c3kpath=path)
    assert (D.numtrain, D.numtest, D.numsteps, D.numepochs, D.batchsize, D.H1, D.H2, D.H3) == (20000, 2000, 10000, 1, 20000, 256, 256, 256)
    assert D.label_i == ['teff', 'logg', 'feh', 'afe'] and D.waverange == [5150.0, 5300.0] and D.NNtype == 'SMLP' and D.lr == 1e-4
    assert D.restartfile is False and D.outfilename == 'TESTOUT.h5' and D.logplot is False
    assert D.resolution == 32000.0 * 2.0 * np.sqrt(2.0 * np.log(2.0)) and abs(D.resolution / 32000.0 - 2.355) < 1e-3
    monkeypatch.undo()
    with pytest.raises(IOError):
        ts.TrainMod(NNtype="ResNet", c3kpath=path)
    with pytest.raises(IOError):
        ts.TrainMod()                                                   # no grid file
    monkeypatch.setattr(ts, "Trainer", CpuTrainer)
    kw = dict(c3kpath=path, NNtype="LinNet", H1=8, H2=12, H3=6, numtrain=100, numtest=30, batchsize=40, numsteps=3, numepochs=2,
              output=out, device="cpu", seed=3, resolution=20000.0)
    T = ts.TrainMod(**kw)
    first = nnio.load_arrays(out)                                       # (the instances below write to the same path)
    # the sets: seeded, disjoint
    tr0, va0 = T.epoch_sets(0)
    tr1, va1 = T.epoch_sets(1)
    assert len(T.testind) == 30 and len(tr0) == len(va0) == 100
    for a, b in ((tr0, va0), (tr0, T.testind), (va0, T.testind), (tr1, va1), (tr1, T.testind), (va1, T.testind)):
        assert len(np.intersect1d(a, b)) == 0
    assert len(np.unique(tr0)) == 100 and not np.array_equal(tr0, tr1)
    T2 = ts.TrainMod(**kw)
    assert np.array_equal(T.testind, T2.testind) and np.array_equal(T2.epoch_sets(1)[0], tr1)
    assert not np.array_equal(T.testind, ts.TrainMod(**dict(kw, seed=4)).testind)
    with pytest.raises(ValueError):
        ts.TrainMod(**dict(kw, numtrain=200))                           # 30 + 400 > 400 models
    assert np.array_equal(T.xmin, arrays["labels"].min(axis=0)) and np.array_equal(T.xmax, arrays["labels"].max(axis=0))
    assert T.ymin.shape == (1,) and T.ymin[0] == arrays["spectra"].min() and T.ymax[0] == arrays["spectra"].max()
    enc = ((arrays["labels"] - T.xmin) / (T.xmax - T.xmin) - 0.5).astype(np.float32)
    assert np.array_equal(T._x32, enc) and enc.min() == -0.5 and enc.max() == 0.5
    p0 = T.pass_order(0, 0).numpy()
    assert np.array_equal(np.sort(p0), np.arange(100)) and np.array_equal(p0, T.pass_order(0, 0).numpy())
    assert not np.array_equal(p0, T.pass_order(0, 1).numpy()) and not np.array_equal(p0, T.pass_order(0, 0, 'valid').numpy())
    # the learning rate: StepLR(100, 0.9) stepped once an epoch
    assert T.lr_of_epoch(0) == T.lr_of_epoch(99) == 1e-4
    assert T.lr_of_epoch(100) == T.lr_of_epoch(199) == 1e-4 * 0.9 and T.lr_of_epoch(200) == 1e-4 * 0.9 ** 2
    # the file before training: the reference's keys (trainspec.py:214-232)
    assert set(first) == {"testpred", "testlabels", "label_i", "wavelengths", "resolution", "xmin", "xmax", "ymin", "ymax"}
    assert first["resolution"] == 20000.0 * 2.0 * np.sqrt(2.0 * np.log(2.0))
    assert np.array_equal(first["testpred"], arrays["spectra"][T.testind]) and np.array_equal(first["testlabels"], arrays["labels"][T.testind])
    # a run
    CpuTrainer.created.clear()
    arrs, trainer, elapsed = T.run()
    assert trainer is CpuTrainer.created[-1] and trainer.steps == 2 * 3 * 2 and set(trainer.batch_rows) == {40} and trainer.lrs == [1e-4, 1e-4]
    assert T.iter_arr == [(0, 0), (1, 0)] and len(T.validation_loss) == 2 and T.validation_loss[1] < T.validation_loss[0]
    got = nnio.load_arrays(out)
    assert set(got) == set(first) | {"model/lin%d.%s" % (i, k) for i in range(1, 7) for k in ("weight", "bias")}
    net = nnio.load_spec_net(out, "LinNet")
    assert [w.shape for w, b, a in net["layers"]] == [(8, 4), (8, 8), (12, 8), (12, 12), (6, 12), (60, 6)]
    assert all(np.array_equal(w, p[0]) and np.array_equal(b, p[1]) for (w, b, a), p in zip(net["layers"], trainer.params()))
    assert np.array_equal(net["wavelength"], wave) and net["resolution"] == float(first["resolution"])
    # restartfile: starts from the file's parameters; waverange cuts the pixels
    CpuTrainer.created.clear()
    T3 = ts.TrainMod(**dict(kw, restartfile=out, output=str(tmp_path / "net2.npz"), numepochs=0))
    T3.run()
    assert all(np.array_equal(a, b) for La, Lb in zip(CpuTrainer.created[-1].params(), trainer.params()) for a, b in zip(La, Lb))
    T4 = ts.TrainMod(**dict(kw, waverange=[wave[10], wave[29]], output=str(tmp_path / "net3.npz")))
    assert T4.D_out == 20 and np.array_equal(T4.wavelengths, wave[10:30])
    with pytest.raises(ValueError):
        ts.TrainMod(**dict(kw, waverange=[1000.0, 1100.0]))
