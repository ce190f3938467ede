"""Training the spectral networks on the MI355X: payne_specmlp_train_* (csrc/k_specmlp_train.hip) through the ABI and through
Payne.train.trainspec.TrainMod, against torch autograd / torch.optim.RAdam on the CPU in fp64 (for the fixture's networks stored
in tests/golden/g20_trainspec.npz, frozen from the reference's own modules).

The yardstick and the bound are those of tests/test_trainspec.py, whose helpers are shared: the pooled deviation
E(a) = max over tensors of max|a - a64| / max|a64|, and E(ours) <= 4 x E(torch CPU fp32) everywhere.  The loss is held to the
fp64 sum of squares of the fp32 residuals of payne_specmlp_train_predict's y on the same parameters, to N D_out 2^-52 relative.
Every measured ratio is printed (NOTES.md quotes them)."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import synth
from test_lnmlp import BOUND_FACTOR
from test_trainspec import (G20, ACT, LR, g20_net, layers_from, flat, pooled, torch_loss_grads, torch_predict, sum_of_squares,
                            radam_isolated, random_net, random_batch)

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
TILE_N = (1, 63, 64, 65, 130)                        # around the 64-row tile, and three workgroups with a two-row tail


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_trainspec")


@pytest.fixture(scope="module")
def lib():
    from thepayne_amd import _lib
    return _lib.load()


def f32_layers(layers):
    return [tuple(np.ascontiguousarray(a, dtype=np.float32) for a in L) for L in layers]


def make_desc(layers, nntype):
    """(SpecmlpDesc, the arrays it points into)."""
    from thepayne_amd import _lib
    keep = f32_layers(layers)
    d = _lib.SpecmlpDesc()
    d.n_layers, d.act = len(keep), ACT[nntype] if isinstance(nntype, str) else nntype
    for i, (w, b) in enumerate(keep):
        d.layers[i].n_out, d.layers[i].n_in = w.shape
        d.layers[i].w, d.layers[i].b = w.ctypes.data, b.ctypes.data
    return d, keep


def make_trainer(lib, layers, nntype, max_rows=130, lr=LR, beta1=0.9):
    from thepayne_amd import _lib
    d, keep = make_desc(layers, nntype)
    o = _lib.SpecmlpTrainOpts()
    o.lr, o.beta1, o.beta2, o.eps, o.max_rows = lr, beta1, 0.999, 1e-8, max_rows
    h = C.c_void_p()
    return lib.payne_specmlp_train_create(0, C.byref(d), C.byref(o), C.byref(h)), h


def batch(x, t, N, pad_x=3, pad_t=5):
    """The first N rows on the device with ld_x = D_in + pad_x, ld_t = D_out + pad_t and 1e30 in the padding."""
    import torch
    xp = np.full((max(N, 1), x.shape[1] + pad_x), 1e30, dtype=np.float32)
    tp = np.full((max(N, 1), t.shape[1] + pad_t), 1e30, dtype=np.float32)
    xp[:N, :x.shape[1]], tp[:N, :t.shape[1]] = x[:N], t[:N]
    return torch.as_tensor(xp).to("cuda:0"), torch.as_tensor(tp).to("cuda:0")


def call(fn, h, x_d, t_d, N):
    """fn = payne_specmlp_train_step / _loss on the batch -> (rc, the loss buffer [3]: sentinel, loss, sentinel)."""
    import torch
    loss_d = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda:0")
    rc = fn(h, x_d.data_ptr(), x_d.stride(0), t_d.data_ptr(), t_d.stride(0), N, loss_d[1:].data_ptr(), None)
    torch.cuda.synchronize()
    return rc, loss_d.cpu().numpy()


def predict(lib, h, x_d, N, d_out, pad_y=7):
    """payne_specmlp_train_predict into a buffer with ld_y = D_out + pad_y -> (y [N, D_out], the padding untouched?)."""
    import torch
    y_d = torch.full((N + 1, d_out + pad_y), SENTINEL, dtype=torch.float32, device="cuda:0")
    assert lib.payne_specmlp_train_predict(h, x_d.data_ptr(), x_d.stride(0), N, y_d.data_ptr(), y_d.stride(0), None) == 0
    torch.cuda.synchronize()
    y = y_d.cpu().numpy()
    assert np.all(y[:N, d_out:] == SENTINEL) and np.all(y[N] == SENTINEL)
    return np.ascontiguousarray(y[:N, :d_out])


def get(lib, h, what, layers, nntype):
    out = [tuple(np.full(np.shape(a), SENTINEL, dtype=np.float32) for a in L) for L in layers]
    d, keep = make_desc(out, nntype)                  # (points into `out` itself: contiguous fp32 arrays are not copied)
    assert lib.payne_specmlp_train_get(h, what, C.byref(d)) == 0
    return out


def one_step(lib, layers, nntype, x, t, N, max_rows=None):
    """A fresh handle: predict, then one step on the first N rows -> (y, loss buffer, gradients, parameters after the step)."""
    from thepayne_amd import _lib
    rc, h = make_trainer(lib, layers, nntype, max_rows=max_rows or max(N, 1))
    assert rc == 0 and h.value
    try:
        x_d, t_d = batch(x, t, N)
        y = predict(lib, h, x_d, N, t.shape[1])
        rc, loss = call(lib.payne_specmlp_train_step, h, x_d, t_d, N)
        assert rc == 0 and lib.payne_specmlp_train_steps(h) == 1
        return y, loss, get(lib, h, _lib.SPECMLP_GRADS, layers, nntype), get(lib, h, _lib.SPECMLP_PARAMS, layers, nntype)
    finally:
        lib.payne_specmlp_train_destroy(h)


def same_bytes(A, B):
    return all(a.tobytes() == b.tobytes() for La, Lb in zip(A, B) for a, b in zip(La, Lb))


def check_grads(what, grads, layers, nntype, x, t, N, g64=None):
    import torch
    if g64 is None:
        g64 = torch_loss_grads(layers, nntype, x[:N], t[:N], torch.float64)[1]
    g32 = torch_loss_grads(layers, nntype, x[:N], t[:N], torch.float32)[1]
    e, e32 = pooled(flat(grads), flat(g64)), pooled(flat(g32), flat(g64))
    print("%s: gradients E = %.3g = %.2f x torch fp32's %.3g" % (what, e, e / e32, e32))
    assert e <= BOUND_FACTOR * e32, (what, e / e32)


def check_y(what, y, layers, nntype, x, N):
    import torch
    y64, y32 = torch_predict(layers, nntype, x[:N], torch.float64), torch_predict(layers, nntype, x[:N], torch.float32)
    e, e32 = np.abs(y - y64).max() / np.abs(y64).max(), np.abs(y32 - y64).max() / np.abs(y64).max()
    print("%s: y E = %.3g = %.2f x torch fp32's %.3g" % (what, e, e / e32, e32))
    assert e <= BOUND_FACTOR * e32, (what, e / e32)


@pytest.mark.parametrize("name", sorted(G20))
def test_loss_and_gradients_through_the_abi(lib, g20, name):
    """Both fixture networks at N in {1, 63, 64, 65, 130}, ld_x > D_in, ld_t > D_out, 1e30 in the padding: the loss against the
    fp64 sum of squares of payne_specmlp_train_predict's fp32 residuals, the first step's gradients within the pooled bound (at
    N = 130 against the fixture's fp64 gradients); the sentinels around the loss word intact; a second handle returns the same
    bytes for loss, gradients and parameters."""
    nntype = G20[name]
    layers, x, t = g20_net(g20, name)
    layers = f32_layers(layers)
    for N in TILE_N:
        y, loss, grads, pars = one_step(lib, layers, nntype, x, t, N, max_rows=130 if N > 64 else N)
        assert loss[0] == SENTINEL and loss[2] == SENTINEL
        own = sum_of_squares(y, t[:N])
        print("g20 %s N=%d: loss %.17g, from payne_specmlp_train_predict's y %.17g" % (name, N, loss[1], own))
        assert abs(loss[1] - own) <= N * t.shape[1] * 2.0 ** -52 * own, (name, N)
        g64 = layers_from(g20, name + "/grad64/", nntype) if N == 130 else None
        check_grads("g20 %s N=%d" % (name, N), grads, layers, nntype, x, t, N, g64=g64)
        assert not same_bytes(pars, layers)                           # the update has moved the parameters
        y2, loss2, grads2, pars2 = one_step(lib, layers, nntype, x, t, N, max_rows=130 if N > 64 else N)
        assert loss2.tobytes() == loss.tobytes() and y2.tobytes() == y.tobytes() and same_bytes(grads, grads2) and same_bytes(pars, pars2), (name, N)


@pytest.mark.parametrize("name", sorted(G20))
def test_trajectory_and_consistency_through_the_abi(lib, g20, name):
    """12 full-batch steps at N = 130: the loss curve and the final parameters against the fixture's fp64 run, within 4 x torch
    fp32's deviations.  Then payne_specmlp_train_loss on 130 rows in chunks (max_rows = 50) equals the whole to N D_out 2^-52
    and changes neither parameters nor the step counter; a 13th step's gradients (dA through the transposed stored order) are
    those of the exported parameters; payne_specmlp_train_set_lr takes effect on the next step only."""
    from thepayne_amd import _lib
    nntype = G20[name]
    layers, x, t = g20_net(g20, name)
    layers = f32_layers(layers)
    rc, h = make_trainer(lib, layers, nntype, max_rows=130)
    assert rc == 0
    hs = None
    try:
        x_d, t_d = batch(x, t, 130)
        losses = []
        for s in range(12):
            rc, loss = call(lib.payne_specmlp_train_step, h, x_d, t_d, 130)
            assert rc == 0
            losses.append(loss[1])
        L64 = g20[name + "/traj_loss64"]
        e_loss, dev_loss = np.abs(np.array(losses) - L64).max() / L64.max(), float(g20[name + "/traj_loss_dev"])
        pars = get(lib, h, _lib.SPECMLP_PARAMS, layers, nntype)
        final64 = flat(layers_from(g20, name + "/traj_final64/", nntype, base=layers))
        e_par, dev_par = pooled(flat(pars), final64), float(g20[name + "/traj_par_dev"])
        print("g20 %s 12 steps: loss curve %.3g = %.2f x torch fp32's %.3g; parameters E = %.3g = %.2f x torch fp32's %.3g"
              % (name, e_loss, e_loss / dev_loss, dev_loss, e_par, e_par / dev_par, dev_par))
        assert e_loss <= BOUND_FACTOR * dev_loss and e_par <= BOUND_FACTOR * dev_par
        assert lib.payne_specmlp_train_steps(h) == 12
        # the loss whole and in chunks of max_rows = 50, on a second handle started from the exported parameters
        rc, whole = call(lib.payne_specmlp_train_loss, h, x_d, t_d, 130)
        assert rc == 0 and whole[0] == SENTINEL and whole[2] == SENTINEL
        own = sum_of_squares(predict(lib, h, x_d, 130, t.shape[1]), t)
        assert abs(whole[1] - own) <= 130 * t.shape[1] * 2.0 ** -52 * own, name
        rc, hs = make_trainer(lib, pars, nntype, max_rows=50)
        assert rc == 0
        rc, parts = call(lib.payne_specmlp_train_loss, hs, x_d, t_d, 130)
        assert rc == 0 and abs(parts[1] - whole[1]) <= 130 * t.shape[1] * 2.0 ** -52 * whole[1], name
        assert np.array_equal(predict(lib, hs, x_d, 130, t.shape[1]), predict(lib, h, x_d, 130, t.shape[1]))
        assert lib.payne_specmlp_train_steps(hs) == 0 and same_bytes(get(lib, hs, _lib.SPECMLP_PARAMS, layers, nntype), pars)
        assert lib.payne_specmlp_train_steps(h) == 12 and same_bytes(get(lib, h, _lib.SPECMLP_PARAMS, layers, nntype), pars)
        # the transposed copy: a 13th step's gradients are those of the exported parameters
        assert call(lib.payne_specmlp_train_step, h, x_d, t_d, 130)[0] == 0
        check_grads("g20 %s step 13" % name, get(lib, h, _lib.SPECMLP_GRADS, layers, nntype), pars, nntype, x, t, 130)
        # set_lr: two handles from the same parameters take one step at 1e-4; the second is then set to 1e-3 -- its parameters
        # are still the first's; after one more step each they differ, and the second's move is the larger
        ha = [make_trainer(lib, layers, nntype, max_rows=130)[1] for _ in range(2)]
        try:
            for hh in ha:
                assert call(lib.payne_specmlp_train_step, hh, x_d, t_d, 130)[0] == 0
            assert lib.payne_specmlp_train_set_lr(ha[1], 1e-3) == 0
            p1 = [get(lib, hh, _lib.SPECMLP_PARAMS, layers, nntype) for hh in ha]
            assert same_bytes(p1[0], p1[1])
            for hh in ha:
                assert call(lib.payne_specmlp_train_step, hh, x_d, t_d, 130)[0] == 0
            p2 = [get(lib, hh, _lib.SPECMLP_PARAMS, layers, nntype) for hh in ha]
            move = [np.abs(p2[i][-1][0] - p1[i][-1][0]).max() for i in range(2)]
            print("g20 %s set_lr: the second step moves W_out by %.3g at 1e-4 and %.3g at 1e-3" % (name, move[0], move[1]))
            assert 5.0 * move[0] < move[1] < 20.0 * move[0]
        finally:
            for hh in ha:
                lib.payne_specmlp_train_destroy(hh)
    finally:
        lib.payne_specmlp_train_destroy(h)
        lib.payne_specmlp_train_destroy(hs)


@pytest.mark.parametrize("nntype", sorted(ACT))
@pytest.mark.parametrize("d_out", (1, 31, 128, 129, 513, 1100))
def test_wide_and_ragged_outputs_through_the_abi(lib, nntype, d_out):
    """Hidden widths (33, 512, 40), N = 65, D_out from one column to 1100: a partial 32-column tile; exactly one and just over one
    128-column chunk of the output layer; just over one 512-column chunk of the dA_last stream; a ragged last chunk of both.
    Gradients and payne_specmlp_train_predict within the pooled bound against the in-test fp64 restatement."""
    rng = np.random.default_rng(7000 + d_out)
    layers = random_net(rng, [4, 33, 512, 40, d_out])
    x, t = random_batch(rng, 65, 4, d_out)
    y, loss, grads, pars = one_step(lib, layers, nntype, x, t, 65)
    what = "%s 4-33-512-40-%d N=65" % (nntype, d_out)
    own = sum_of_squares(y, t)
    assert abs(loss[1] - own) <= 65 * d_out * 2.0 ** -52 * own, what
    check_y(what, y, layers, nntype, x, 65)
    check_grads(what, grads, layers, nntype, x, t, 65)


@pytest.mark.parametrize("name", sorted(G20))
def test_update_isolated_through_the_abi(lib, g20, name):
    """8 steps at N = 65; after each the gradients are read and fed to torch RAdam on the CPU: the parameters against fp64 RAdam on
    those same gradients (steps 5 -> 6 cross the rectification switch)."""
    from thepayne_amd import _lib
    nntype = G20[name]
    layers, x, t = g20_net(g20, name)
    layers = f32_layers(layers)
    rc, h = make_trainer(lib, layers, nntype, max_rows=65)
    assert rc == 0
    try:
        x_d, t_d = batch(x, t, 65)
        G, P = [], []
        for s in range(8):
            assert call(lib.payne_specmlp_train_step, h, x_d, t_d, 65)[0] == 0
            G.append(get(lib, h, _lib.SPECMLP_GRADS, layers, nntype))
            P.append(get(lib, h, _lib.SPECMLP_PARAMS, layers, nntype))
        radam_isolated(layers, G, P, "g20 %s" % name)
    finally:
        lib.payne_specmlp_train_destroy(h)


def test_return_codes_without_a_launch(lib, g20):
    from thepayne_amd import _lib
    import torch
    layers, x, t = g20_net(g20, "smlp")
    layers = f32_layers(layers)
    rc, h = make_trainer(lib, layers, "SMLP", max_rows=64)
    assert rc == 0
    try:
        x_d, t_d = batch(x, t, 65, pad_x=0, pad_t=0)
        step, lossf, pred = lib.payne_specmlp_train_step, lib.payne_specmlp_train_loss, lib.payne_specmlp_train_predict
        rc, loss = call(step, h, x_d, t_d, 0)
        assert rc == 0 and np.all(loss == SENTINEL) and lib.payne_specmlp_train_steps(h) == 0      # N == 0 writes nothing
        assert call(lossf, h, x_d, t_d, 0)[0] == 0
        assert step(h, None, 5, None, 150, 0, None, None) == 0 and pred(h, None, 5, 0, None, 150, None) == 0
        loss_d = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda:0")
        y_d = torch.full((4, 150), SENTINEL, dtype=torch.float32, device="cuda:0")
        args = lambda ld_x=5, ld_t=150, N=4: (x_d.data_ptr(), ld_x, t_d.data_ptr(), ld_t, N, loss_d.data_ptr(), None)
        for fn in (step, lossf):
            assert fn(None, *args()) == _lib.E_INVALID                                            # NULL handle
            assert fn(h, *args(N=-1)) == _lib.E_INVALID
            assert fn(h, *args(ld_x=4)) == _lib.E_INVALID and fn(h, *args(ld_t=149)) == _lib.E_INVALID
            assert fn(h, None, 5, t_d.data_ptr(), 150, 4, loss_d.data_ptr(), None) == _lib.E_INVALID
            assert fn(h, x_d.data_ptr(), 5, None, 150, 4, loss_d.data_ptr(), None) == _lib.E_INVALID
        assert step(h, *args(N=65)) == _lib.E_INVALID                                             # N > max_rows
        assert lossf(h, x_d.data_ptr(), 5, t_d.data_ptr(), 150, 4, None, None) == _lib.E_INVALID
        assert pred(None, x_d.data_ptr(), 5, 4, y_d.data_ptr(), 150, None) == _lib.E_INVALID
        assert pred(h, x_d.data_ptr(), 5, -1, y_d.data_ptr(), 150, None) == _lib.E_INVALID
        assert pred(h, x_d.data_ptr(), 4, 4, y_d.data_ptr(), 150, None) == _lib.E_INVALID
        assert pred(h, x_d.data_ptr(), 5, 4, y_d.data_ptr(), 149, None) == _lib.E_INVALID
        assert pred(h, None, 5, 4, y_d.data_ptr(), 150, None) == _lib.E_INVALID and pred(h, x_d.data_ptr(), 5, 4, None, 150, None) == _lib.E_INVALID
        for bad in (0.0, -1e-4, float("nan"), float("inf")):
            assert lib.payne_specmlp_train_set_lr(h, bad) == _lib.E_INVALID
        assert lib.payne_specmlp_train_set_lr(None, 1e-4) == _lib.E_INVALID and lib.payne_specmlp_train_set_lr(h, 2e-4) == 0
        torch.cuda.synchronize()
        assert loss_d.item() == SENTINEL and torch.all(y_d == SENTINEL).item() and lib.payne_specmlp_train_steps(h) == 0
        assert same_bytes(get(lib, h, _lib.SPECMLP_PARAMS, layers, "SMLP"), layers)
        d, keep = make_desc(layers, "SMLP")
        assert lib.payne_specmlp_train_get(h, 2, C.byref(d)) == _lib.E_INVALID
        assert lib.payne_specmlp_train_get(None, 0, C.byref(d)) == _lib.E_INVALID and lib.payne_specmlp_train_get(h, 0, None) == _lib.E_INVALID
        d.layers[1].w = None
        assert lib.payne_specmlp_train_get(h, 0, C.byref(d)) == _lib.E_INVALID
        d, keep = make_desc(layers, "SMLP")
        d.n_layers = 5
        assert lib.payne_specmlp_train_get(h, 0, C.byref(d)) == _lib.E_INVALID
    finally:
        lib.payne_specmlp_train_destroy(h)
    lib.payne_specmlp_train_destroy(None)
    assert lib.payne_specmlp_train_steps(None) == -1
    # create
    assert make_trainer(lib, layers, "SMLP", max_rows=0)[0] == _lib.E_INVALID
    assert make_trainer(lib, layers, "SMLP", lr=0.0)[0] == _lib.E_INVALID
    assert make_trainer(lib, layers, "SMLP", beta1=1.0)[0] == _lib.E_INVALID
    assert make_trainer(lib, layers, 2)[0] == _lib.E_INVALID                                      # an activation kind that is neither
    rng = np.random.default_rng(0)
    for dims in ([6, 513, 8], [33, 16, 8], [6, 8], [6, 16, 65537]):                               # the limits
        rc, hh = make_trainer(lib, random_net(rng, dims), "SMLP", max_rows=8)
        assert rc == _lib.E_UNSUPPORTED and not hh.value, dims
        assert lib.payne_last_error(None).startswith(b"payne_specmlp_train_create: "), dims       # the message of a create that had no context
    rc, hh = make_trainer(lib, random_net(rng, [32, 512, 513]), "LinNet", max_rows=8)             # D_out alone may pass 512
    assert rc == 0
    lib.payne_specmlp_train_destroy(hh)
    d, keep = make_desc(random_net(rng, [6] + [8] * 8), "SMLP")
    o = _lib.SpecmlpTrainOpts()
    o.lr, o.beta1, o.beta2, o.eps, o.max_rows = 1e-4, 0.9, 0.999, 1e-8, 8
    d.n_layers = 9
    assert lib.payne_specmlp_train_create(0, C.byref(d), C.byref(o), C.byref(C.c_void_p())) == _lib.E_UNSUPPORTED
    assert lib.payne_specmlp_train_create(0, None, C.byref(o), C.byref(C.c_void_p())) == _lib.E_INVALID
    d.n_layers = 8
    assert lib.payne_specmlp_train_create(0, C.byref(d), None, C.byref(C.c_void_p())) == _lib.E_INVALID
    assert lib.payne_specmlp_train_create(0, C.byref(d), C.byref(o), None) == _lib.E_INVALID
    d.layers[3].b = None
    assert lib.payne_specmlp_train_create(0, C.byref(d), C.byref(o), C.byref(C.c_void_p())) == _lib.E_INVALID
    d, keep = make_desc(random_net(rng, [6, 8, 8]), "SMLP")
    d.layers[1].n_in = 7                                                                          # does not follow the layer before
    assert lib.payne_specmlp_train_create(0, C.byref(d), C.byref(o), C.byref(C.c_void_p())) == _lib.E_INVALID


@pytest.mark.parametrize("nntype", sorted(ACT))
def test_trainmod_end_to_end(tmp_path, nntype):
    """TrainMod on a synthetic grid of 1500 models of 300 pixels from an SMLP teacher, 2 epochs of 30 passes over 512 models in
    batches of 128: the validation loss of the last epoch is below the first's; PayneSpecPredict reads the file and its
    predictspec on the test labels agrees with the trainer's own forward to the tolerance tests/test_api_gpu.py holds a
    network's output to, 5e-6 x max|y|; TestSpec's medians are finite."""
    import torch
    from Payne.predict.predictspec import PayneSpecPredict
    from Payne.testing.testspec import TestSpec
    from Payne.train.trainspec import TrainMod
    from thepayne_amd.train import trainspec as ts
    path, out = str(tmp_path / "grid.npz"), str(tmp_path / "net.npz")
    synth.spec_grid(path, 1500, kind="SMLP", npix=300, seed=3)
    T = TrainMod(c3kpath=path, NNtype=nntype, H1=40, H2=24, H3=33, numtrain=512, batchsize=128, numsteps=30, numepochs=2, output=out, seed=11)
    arrs, trainer, elapsed = T.run()
    assert trainer.steps == 2 * 30 * 4 and T.iter_arr == [(0, 0), (1, 0)]
    print("TrainMod %s: validation loss %.6g -> %.6g, training loss %.6g -> %.6g" % (
        nntype, T.validation_loss[0], T.validation_loss[-1], T.training_loss[0], T.training_loss[-1]))
    assert T.validation_loss[-1] < T.validation_loss[0]
    P = PayneSpecPredict(nnpath=T.outpath, NNtype=nntype)
    labels = np.load(T.outpath)["testlabels"]
    assert labels.shape == (51, 4)
    pred = np.asarray(P.predictspec(labels))
    own = trainer.predict(torch.as_tensor(ts.encode(labels, T.xmin, T.xmax)).to("cuda:0")).cpu().numpy()
    err = np.abs(pred - own).max()
    print("TrainMod %s: max|predictspec - payne_specmlp_train_predict| = %.3g = %.3g x max|y|" % (nntype, err, err / np.abs(own).max()))
    assert pred.shape == own.shape == (51, 300) and err <= 5e-6 * np.abs(own).max()
    stats = TestSpec(T.outpath, NNtype=nntype).stats()
    assert stats["pixel_mad"].shape == (300,) and stats["spec_mad"].shape == (51,)
    assert np.all(np.isfinite(stats["pixel_mad"])) and np.all(np.isfinite(stats["spec_mad"]))
