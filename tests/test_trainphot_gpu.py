"""Training the photometric LayerNorm + SiLU networks on the MI355X: payne_lnmlp_train_* (csrc/k_lnmlp_train.hip) through the ABI
and through Payne.train.trainphot.TrainMod, against torch autograd / torch.optim.RAdam on the CPU in fp64 (for the fixture's
networks stored in tests/golden/g19_trainphot.npz, frozen from the reference's own modules).

The yardstick and the bound are those of tests/test_trainphot.py, whose helpers are shared: the pooled deviation
E(a) = max over tensors of max|a - a64| / max|a64|, and E(ours) <= 4 x E(torch CPU fp32) everywhere.  The loss is held to the
fp64 mean of squares of the fp32 residuals of payne_lnmlp_eval's y on the same parameters, to N D_out 2^-52 relative: which
also says that the trainer's forward returns payne_lnmlp_eval's bits.  Every measured ratio is printed (NOTES.md quotes them)."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import synth
from test_lnmlp import BOUND_FACTOR
from test_lnmlp_gpu import make_desc, create as create_eval
from test_trainphot import G19, g19_net, layers_from, flat, pooled, drop_scale, torch_loss_grads, loss_of_residuals, radam_isolated

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
TILE_N = (1, 63, 64, 65, 257)                        # around the 64-row tile, and several workgroups with a one-row tail


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_trainphot")


@pytest.fixture(scope="module")
def lib():
    from thepayne_amd import _lib
    return _lib.load()


def f32_layers(layers):
    return [tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in L) for L in layers]


def make_trainer(lib, layers, p=(), max_rows=257, seed=0, lr=1e-3, norm=None):
    from thepayne_amd import _lib
    d, keep = make_desc(layers, norm)
    o = _lib.LnmlpTrainOpts()
    o.lr, o.beta1, o.beta2, o.eps, o.seed, o.max_rows = lr, 0.9, 0.999, 1e-8, seed, max_rows
    for i, pp in enumerate(p):
        o.dropout_p[i] = pp
    h = C.c_void_p()
    return lib.payne_lnmlp_train_create(0, C.byref(d), C.byref(o), C.byref(h)), h


def batch(x, t, N, pad_x=3, pad_t=5):
    """The first N rows on the device with ld_x = D_in + pad_x, ld_t = D_out + pad_t and 1e30 in the padding."""
    import torch
    xp = np.full((max(N, 1), x.shape[1] + pad_x), 1e30, dtype=np.float32)
    tp = np.full((max(N, 1), t.shape[1] + pad_t), 1e30, dtype=np.float32)
    xp[:N, :x.shape[1]], tp[:N, :t.shape[1]] = x[:N], t[:N]
    return torch.as_tensor(xp).to("cuda:0"), torch.as_tensor(tp).to("cuda:0")


def call(fn, h, x_d, t_d, N):
    """fn = payne_lnmlp_train_step / _loss on the batch -> (rc, the loss buffer [3]: sentinel, loss, sentinel)."""
    import torch
    loss_d = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda:0")
    rc = fn(h, x_d.data_ptr(), x_d.stride(0), t_d.data_ptr(), t_d.stride(0), N, loss_d[1:].data_ptr(), None)
    torch.cuda.synchronize()
    return rc, loss_d.cpu().numpy()


def get(lib, h, what, layers):
    out = [tuple(None if a is None else np.full(np.shape(a), SENTINEL, dtype=np.float32) for a in L) for L in layers]
    d, keep = make_desc(out)                          # (points into `out` itself: contiguous fp32 arrays are not copied)
    assert lib.payne_lnmlp_train_get(h, what, C.byref(d)) == 0
    return out


def eval_y(lib, layers, x, N):
    """payne_lnmlp_eval's y [N, D_out] for the parameters `layers` on the fp32 rows x."""
    import torch
    rc, h = create_eval(lib, layers)
    assert rc == 0
    try:
        d_out = layers[-1][0].shape[0]
        x_d = torch.as_tensor(np.asarray(x[:N], dtype=np.float32).astype(np.float64)).to("cuda:0")
        y_d = torch.empty((N, d_out), dtype=torch.float32, device="cuda:0")
        assert lib.payne_lnmlp_eval(h, x_d.data_ptr(), x_d.stride(0), N, y_d.data_ptr(), y_d.stride(0), None) == 0
        torch.cuda.synchronize()
        return y_d.cpu().numpy()
    finally:
        lib.payne_lnmlp_destroy(h)


def one_step(lib, layers, x, t, N, p=(), seed=0, max_rows=None):
    """A fresh handle, one step on the first N rows -> (loss buffer, gradients, parameters after the step)."""
    from thepayne_amd import _lib
    rc, h = make_trainer(lib, layers, p=p, max_rows=max_rows or max(N, 1), seed=seed)
    assert rc == 0 and h.value
    try:
        x_d, t_d = batch(x, t, N)
        rc, loss = call(lib.payne_lnmlp_train_step, h, x_d, t_d, N)
        assert rc == 0 and lib.payne_lnmlp_train_steps(h) == 1
        return loss, get(lib, h, _lib.LNMLP_GRADS, layers), get(lib, h, _lib.LNMLP_PARAMS, layers)
    finally:
        lib.payne_lnmlp_train_destroy(h)


def same_bytes(A, B):
    return all(a.tobytes() == b.tobytes() for La, Lb in zip(A, B) for a, b in zip(La, Lb) if a is not None)


def check_grads(what, grads, layers, x, t, N, masks=None, g64=None):
    import torch
    if g64 is None:
        g64 = torch_loss_grads(layers, x[:N], t[:N], torch.float64, masks)[1]
    g32 = torch_loss_grads(layers, x[:N], t[:N], torch.float32, masks)[1]
    e, e32 = pooled(flat(grads), flat(g64)), pooled(flat(g32), flat(g64))
    print("%s: gradients E = %.3g = %.2f x torch fp32's %.3g" % (what, e, e / e32, e32))
    assert e <= BOUND_FACTOR * e32, (what, e / e32)
    return e / e32


@pytest.mark.parametrize("name", sorted(G19))
def test_loss_and_gradients_through_the_abi(lib, g19, name):
    """Both fixture networks at N in {1, 63, 64, 65, 257}, ld_x > D_in, ld_t > D_out, 1e30 in the padding, dropout off: the loss
    against payne_lnmlp_eval's y, the first step's gradients within the pooled bound (at N = 257 against the fixture's fp64
    gradients); a second handle returns the same bytes for loss, gradients and parameters."""
    layers, x, t = g19_net(g19, name)
    layers = f32_layers(layers)
    for N in TILE_N:
        loss, grads, pars = one_step(lib, layers, x, t, N, max_rows=257 if N > 64 else N)
        assert loss[0] == SENTINEL and loss[2] == SENTINEL
        own = loss_of_residuals(eval_y(lib, layers, x, N), t[:N])
        print("g19 %s N=%d: loss %.17g, from payne_lnmlp_eval's y %.17g" % (name, N, loss[1], own))
        assert abs(loss[1] - own) <= N * t.shape[1] * 2.0 ** -52 * own, (name, N)
        g64 = layers_from(g19, name + "/grad64/", G19[name]) if N == 257 else None
        check_grads("g19 %s N=%d" % (name, N), grads, layers, x, t, N, g64=g64)
        assert not same_bytes(pars, layers)                           # the update has moved the parameters
        loss2, grads2, pars2 = one_step(lib, layers, x, t, N, max_rows=257 if N > 64 else N)
        assert loss2.tobytes() == loss.tobytes() and same_bytes(grads, grads2) and same_bytes(pars, pars2), (name, N)


@pytest.mark.parametrize("name", sorted(G19))
def test_trajectory_and_consistency_through_the_abi(lib, g19, name):
    """12 full-batch steps at N = 257, dropout off: the loss curve and the final parameters against the fixture's fp64 run,
    within 4 x torch fp32's deviations.  Then the three weight copies agree: payne_lnmlp_train_loss (the trainer's own forward,
    on its stored order) equals the loss of a fresh payne_lnmlp_create from the exported row-major parameters, also when the
    rows come in chunks of max_rows, and changes neither parameters nor the step counter; the gradients of a 13th step (dA_in
    through the transposed stored order) are those of the exported parameters."""
    from thepayne_amd import _lib
    layers, x, t = g19_net(g19, name)
    layers = f32_layers(layers)
    rc, h = make_trainer(lib, layers, max_rows=257)
    rc2, hs = make_trainer(lib, layers, max_rows=100)
    assert rc == 0 and rc2 == 0
    try:
        x_d, t_d = batch(x, t, 257)
        losses = []
        for s in range(12):
            rc, loss = call(lib.payne_lnmlp_train_step, h, x_d, t_d, 257)
            assert rc == 0
            losses.append(loss[1])
        L64 = g19[name + "/traj_loss64"]
        e_loss, dev_loss = np.abs(np.array(losses) - L64).max() / L64.max(), float(g19[name + "/traj_loss_dev"])
        pars = get(lib, h, _lib.LNMLP_PARAMS, layers)
        e_par, dev_par = pooled(flat(pars), flat(layers_from(g19, name + "/traj_final64/", G19[name]))), float(g19[name + "/traj_par_dev"])
        print("g19 %s 12 steps: loss curve %.3g = %.2f x torch fp32's %.3g; parameters E = %.3g = %.2f x torch fp32's %.3g"
              % (name, e_loss, e_loss / dev_loss, dev_loss, e_par, e_par / dev_par, dev_par))
        assert e_loss <= BOUND_FACTOR * dev_loss and e_par <= BOUND_FACTOR * dev_par
        assert lib.payne_lnmlp_train_steps(h) == 12
        # consistency
        rc, loss = call(lib.payne_lnmlp_train_loss, h, x_d, t_d, 257)
        assert rc == 0 and loss[0] == SENTINEL and loss[2] == SENTINEL
        own = loss_of_residuals(eval_y(lib, pars, x, 257), t)
        assert abs(loss[1] - own) <= 257 * t.shape[1] * 2.0 ** -52 * own, name
        assert lib.payne_lnmlp_train_steps(h) == 12 and same_bytes(get(lib, h, _lib.LNMLP_PARAMS, layers), pars)
        # the transposed copy: a 13th step's gradients are those of the exported parameters
        assert call(lib.payne_lnmlp_train_step, h, x_d, t_d, 257)[0] == 0
        check_grads("g19 %s step 13" % name, get(lib, h, _lib.LNMLP_GRADS, layers), pars, x, t, 257)
        # one step on 100 rows, then the loss of 257 rows in chunks of max_rows = 100
        xs_d, ts_d = batch(x, t, 100)
        assert call(lib.payne_lnmlp_train_step, hs, xs_d, ts_d, 100)[0] == 0
        ps = get(lib, hs, _lib.LNMLP_PARAMS, layers)
        rc, loss = call(lib.payne_lnmlp_train_loss, hs, x_d, t_d, 257)
        own = loss_of_residuals(eval_y(lib, ps, x, 257), t)
        assert rc == 0 and abs(loss[1] - own) <= 257 * t.shape[1] * 2.0 ** -52 * own, name
    finally:
        lib.payne_lnmlp_train_destroy(h)
        lib.payne_lnmlp_train_destroy(hs)


@pytest.mark.parametrize("name", sorted(G19))
def test_update_isolated_through_the_abi(lib, g19, name):
    """8 steps at N = 65; after each the gradients are read and fed to torch RAdam on the CPU: the parameters against fp64 RAdam on
    those same gradients (steps 5 -> 6 cross the rectification switch)."""
    from thepayne_amd import _lib
    layers, x, t = g19_net(g19, name)
    layers = f32_layers(layers)
    rc, h = make_trainer(lib, layers, max_rows=65)
    assert rc == 0
    try:
        x_d, t_d = batch(x, t, 65)
        G, P = [], []
        for s in range(8):
            assert call(lib.payne_lnmlp_train_step, h, x_d, t_d, 65)[0] == 0
            G.append(get(lib, h, _lib.LNMLP_GRADS, layers))
            P.append(get(lib, h, _lib.LNMLP_PARAMS, layers))
        radam_isolated(layers, G, P, "g19 %s" % name)
    finally:
        lib.payne_lnmlp_train_destroy(h)


def test_dropout_through_the_abi(lib, g19):
    """MLP_v0 with p = 0.3 behind block 3, N = 65: gradients against the restatement multiplied by the exported mask."""
    from thepayne_amd.train import trainphot as tp
    layers, x, t = g19_net(g19, "v0")
    layers = f32_layers(layers)
    p = [0.0, 0.0, 0.3, 0.0, 0.0]
    loss, grads, pars = one_step(lib, layers, x, t, 65, p=p, seed=77)
    masks = {2: drop_scale(tp.dropout_mask(77, 0, 2, 65, layers[2][0].shape[0], 0.3), 0.3)}
    check_grads("g19 v0 p=0.3 N=65", grads, layers, x, t, 65, masks=masks)
    loss0, grads0, _ = one_step(lib, layers, x, t, 65)
    assert loss0[1] != loss[1] and not same_bytes(grads, grads0)      # the mask was applied
    loss2, grads2, pars2 = one_step(lib, layers, x, t, 65, p=p, seed=77)
    assert loss2.tobytes() == loss.tobytes() and same_bytes(grads, grads2) and same_bytes(pars, pars2)


def random_net(rng, dims):
    layers = []
    for i in range(len(dims) - 1):
        k = 1.0 / np.sqrt(dims[i])
        hidden = i < len(dims) - 2
        layers.append((rng.uniform(-k, k, (dims[i + 1], dims[i])).astype(np.float32), rng.uniform(-k, k, dims[i + 1]).astype(np.float32),
                       (1 + rng.normal(0, 0.3, dims[i + 1])).astype(np.float32) if hidden else None,
                       rng.normal(0, 0.3, dims[i + 1]).astype(np.float32) if hidden else None))
    return layers


@pytest.mark.parametrize("dims,N", [((6, 256, 256, 256, 256, 256, 8), 257), ((6, 256, 256, 256, 256, 256, 8), 2048), ((32, 512, 500, 300), 65)])
def test_shapes_through_the_abi(lib, dims, N):
    """The default shape at N = 257 and at the reference's batch of 2048, and the widest network (512, a padded 500, D_in = 32)
    at N = 65: one step, gradients within the pooled bound, torch fp32 computed at run time; the loss against payne_lnmlp_eval."""
    rng = np.random.default_rng(sum(dims) + N)
    layers = random_net(rng, dims)
    x = rng.normal(0, 1.5, (N, dims[0])).astype(np.float32)
    t = rng.normal(0, 1.0, (N, dims[-1])).astype(np.float32)
    loss, grads, pars = one_step(lib, layers, x, t, N)
    own = loss_of_residuals(eval_y(lib, layers, x, N), t)
    assert abs(loss[1] - own) <= N * dims[-1] * 2.0 ** -52 * own
    check_grads("widths %s N=%d" % ("-".join(map(str, dims)), N), grads, layers, x, t, N)


def test_return_codes_without_a_launch(lib, g19):
    from thepayne_amd import _lib
    import torch
    layers, x, t = g19_net(g19, "v0")
    layers = f32_layers(layers)
    rc, h = make_trainer(lib, layers, max_rows=64)
    assert rc == 0
    try:
        x_d, t_d = batch(x, t, 65, pad_x=0, pad_t=0)
        step, lossf = lib.payne_lnmlp_train_step, lib.payne_lnmlp_train_loss
        rc, loss = call(step, h, x_d, t_d, 0)
        assert rc == 0 and np.all(loss == SENTINEL) and lib.payne_lnmlp_train_steps(h) == 0        # N == 0 writes nothing
        assert call(lossf, h, x_d, t_d, 0)[0] == 0
        assert step(h, None, 5, None, 3, 0, None, None) == 0
        loss_d = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda:0")
        args = lambda ld_x=5, ld_t=3, N=4: (x_d.data_ptr(), ld_x, t_d.data_ptr(), ld_t, N, loss_d.data_ptr(), None)
        for fn in (step, lossf):
            assert fn(None, *args()) == _lib.E_INVALID                                            # NULL handle
            assert fn(h, *args(N=-1)) == _lib.E_INVALID
            assert fn(h, *args(ld_x=4)) == _lib.E_INVALID and fn(h, *args(ld_t=2)) == _lib.E_INVALID
            assert fn(h, None, 5, t_d.data_ptr(), 3, 4, loss_d.data_ptr(), None) == _lib.E_INVALID
            assert fn(h, x_d.data_ptr(), 5, None, 3, 4, loss_d.data_ptr(), None) == _lib.E_INVALID
        assert step(h, *args(N=65)) == _lib.E_INVALID                                             # N > max_rows
        assert lossf(h, x_d.data_ptr(), 5, t_d.data_ptr(), 3, 4, None, None) == _lib.E_INVALID
        torch.cuda.synchronize()
        assert loss_d.item() == SENTINEL and lib.payne_lnmlp_train_steps(h) == 0
        assert same_bytes(get(lib, h, _lib.LNMLP_PARAMS, layers), layers)
        d, keep = make_desc(layers)
        assert lib.payne_lnmlp_train_get(h, 2, C.byref(d)) == _lib.E_INVALID
        assert lib.payne_lnmlp_train_get(None, 0, C.byref(d)) == _lib.E_INVALID and lib.payne_lnmlp_train_get(h, 0, None) == _lib.E_INVALID
        d.n_layers = 5
        assert lib.payne_lnmlp_train_get(h, 0, C.byref(d)) == _lib.E_INVALID
    finally:
        lib.payne_lnmlp_train_destroy(h)
    lib.payne_lnmlp_train_destroy(None)
    assert lib.payne_lnmlp_train_steps(None) == -1
    # create
    ni = [np.array([0.0, 1.0])] * 5
    no = [np.array([0.0, 1.0])] * 3
    assert make_trainer(lib, layers, norm=(ni, no))[0] == _lib.E_INVALID                          # norms present in init
    for bad in (1.0, -0.01, 1.5, float("nan")):
        rc, hh = make_trainer(lib, layers, p=[0.0, bad])
        assert rc == _lib.E_INVALID and not hh.value, bad
    assert make_trainer(lib, layers, max_rows=0)[0] == _lib.E_INVALID
    assert make_trainer(lib, layers, lr=0.0)[0] == _lib.E_INVALID
    rng = np.random.default_rng(0)
    for dims in ([6, 513, 8], [6, 16, 513], [33, 16, 8], [6, 8]):                                 # the forward's limits
        rc, hh = make_trainer(lib, random_net(rng, dims))
        assert rc == _lib.E_UNSUPPORTED and not hh.value, dims
        assert lib.payne_last_error(None).startswith(b"payne_lnmlp_train_create: "), dims         # the message of a create that had no context
    d, keep = make_desc(random_net(rng, [6] + [8] * 8))
    d.n_layers = 9
    o = _lib.LnmlpTrainOpts()
    o.lr, o.beta1, o.beta2, o.eps, o.max_rows = 1e-3, 0.9, 0.999, 1e-8, 8
    assert lib.payne_lnmlp_train_create(0, C.byref(d), C.byref(o), C.byref(C.c_void_p())) == _lib.E_UNSUPPORTED
    assert lib.payne_lnmlp_train_create(0, None, C.byref(o), C.byref(C.c_void_p())) == _lib.E_INVALID
    d.n_layers = 8
    assert lib.payne_lnmlp_train_create(0, C.byref(d), None, C.byref(C.c_void_p())) == _lib.E_INVALID
    bad = random_net(rng, [6, 16, 8])
    bad[0] = (bad[0][0], bad[0][1], None, None)                                                   # a hidden layer without LayerNorm
    assert make_trainer(lib, bad)[0] == _lib.E_INVALID


def test_trainmod_end_to_end(tmp_path):
    """TrainMod on a synthetic grid of 4000 models from an MLP_v1 teacher: 3 epochs of batches of 256, dropout off.  The same
    batches (epoch_order) replayed by torch on the CPU in fp64 and fp32: the per-batch training losses within 4 x torch fp32's
    deviation, max|L - L64| / max L64; the validation loss falls; modpred reads the file, and its mean squared error on the
    file's test set, taken in normalised magnitudes, is payne_lnmlp_train_loss on those rows.  The last to 1e-4 relative:
    modpred's fp32 roundings of y std + mid (6e-8 of magnitudes near 10, over a std near 1) move a residual of order 0.3 by
    parts in 1e6."""
    import torch
    from Payne.predict.photANN_new import modpred
    from Payne.train.trainphot import TrainMod
    from test_trainphot import restatement
    path, out = str(tmp_path / "grid.npz"), str(tmp_path / "net.npz")
    arrays, label_o, teacher = synth.phot_grid(path, 4000, nntype="MLP_v1", H=(24, 24, 24), D_out=7, seed=2)
    T = TrainMod(modpath=path, label_o=label_o, NNtype="MLP_v1", H1=40, H2=24, H3=33, batchsize=256, numepochs=3, dropout=0,
                 output=out, logplot=False, seed=11)
    model0 = T.run(dryrun=True)[0]
    init = f32_layers(model0.layers)
    net = T.run()
    nb = len(T.trainind) // 256
    assert T.nbatches == nb and nb >= 8 and T.trainer.steps == 3 * nb and len(T.batchloss_arr) == 3
    ours = np.concatenate(T.running_loss)
    xt, yt = T.set_data("train")
    curves = {}
    for dtype in (torch.float64, torch.float32):
        model, pars = restatement(init, dtype)
        opt = torch.optim.RAdam(model.parameters(), lr=1e-3)
        L = []
        for epoch in range(3):
            order = T.epoch_order(epoch).cpu().numpy()
            for i in range(nb):
                idx = order[i * 256:(i + 1) * 256]
                loss = torch.nn.MSELoss(reduction='mean')(model(torch.as_tensor(xt[idx]).to(dtype)), torch.as_tensor(yt[idx]).to(dtype))
                opt.zero_grad()
                loss.backward()
                opt.step()
                L.append(loss.item())
        curves[dtype] = np.array(L)
    L64 = curves[torch.float64]
    e, e32 = np.abs(ours - L64).max() / L64.max(), np.abs(curves[torch.float32] - L64).max() / L64.max()
    print("TrainMod %d steps: loss curve %.3g = %.2f x torch fp32's %.3g; loss %.4f -> %.4f, validation %.4f -> %.4f"
          % (3 * nb, e, e / e32, e32, ours[0], ours[-1], T.validloss_arr[0], T.validloss_arr[-1]))
    assert e <= BOUND_FACTOR * e32, e / e32
    assert T.validloss_arr[-1] < T.validloss_arr[0]
    P = modpred(nnpath=T.outpath, nntype="MLP_v1", norm=True)
    assert list(P.modpararr) == label_o
    arrs = np.load(T.outpath)
    pred = P.pred(arrs["testlabels_in"].T.astype(np.float64))
    assert pred.shape == (len(T.testind), 7)
    no = np.array([T.normfactor[k] for k in label_o])
    x_n, t_n = T.set_data("test")
    mse = float(np.mean(((pred.astype(np.float64) - no[:, 0]) / no[:, 1] - t_n.astype(np.float64)) ** 2))
    loss_d = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    T.trainer.loss(torch.as_tensor(x_n).to("cuda:0"), torch.as_tensor(t_n).to("cuda:0"), loss_d)
    print("modpred's normalised MSE on the test set %.9g, payne_lnmlp_train_loss %.9g" % (mse, loss_d.item()))
    assert abs(mse - loss_d.item()) <= 1e-4 * loss_d.item()
    assert all(np.array_equal(a, b) for La, Lb in zip(net.layers, P.anns.model.layers) for a, b in zip(La, Lb) if a is not None)
