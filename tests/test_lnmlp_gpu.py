"""The photometric LayerNorm + SiLU networks on the MI355X: payne_lnmlp_kernel (csrc/k_lnmlp.hip) through the ABI and through
Payne.predict.photANN_new.modpred, against the reference's module in fp64 (tests/golden/g18_lnmlp.npz) and against the fp64
restatement of tests/test_lnmlp.py, where the same arithmetic runs on the host.

The bound everywhere: max|y_gpu - y64| <= 4 x max|y32 - y64|, y32 being torch's CPU fp32 evaluation of the same network on the
same rows (for g18 stored in the fixture): the kernel sums in another order than torch, the factor is the margin for that and
nothing else.  Measured ratios max|y_gpu - y64| / dev are printed by every test (NOTES.md quotes them)."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import synth
from test_lnmlp import G18, BOUND_FACTOR, g18_net, layers_of, forward64, norm_in, norm_out

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
TILE_N = (1, 63, 64, 65, 257)                        # around the kernel's 64-row tile, and more than one workgroup with a tail


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lnmlp")


@pytest.fixture(scope="module")
def lib():
    from thepayne_amd import _lib
    return _lib.load()


def make_desc(layers, norm=None):
    """(LnmlpDesc, the arrays it points into) for [(W, b, gain | None, beta | None)] and norm = (norm_i, norm_o) | None."""
    from thepayne_amd import _lib
    keep = []

    def ptr(a, dt=np.float32):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(a, dtype=dt))
        return keep[-1].ctypes.data
    d = _lib.LnmlpDesc()
    d.n_layers = len(layers)
    for i, (W, b, g, be) in enumerate(layers):
        L = d.layers[i]
        L.n_out, L.n_in = W.shape
        L.w, L.b, L.ln_gain, L.ln_bias = ptr(W), ptr(b), ptr(g), ptr(be)
    if norm is not None:
        ni, no = (np.asarray(n, dtype=np.float64) for n in norm)
        d.in_mid, d.in_std, d.out_mid, d.out_std = (ptr(a, np.float64) for a in (ni[:, 0], ni[:, 1], no[:, 0], no[:, 1]))
    return d, keep


def create(lib, layers, norm=None):
    d, keep = make_desc(layers, norm)
    h = C.c_void_p()
    rc = lib.payne_lnmlp_create(0, C.byref(d), C.byref(h))
    return rc, h


def evaluate(lib, h, x, N, d_out, pad_x=3, pad_y=5, extra_rows=2):
    """One payne_lnmlp_eval on the first N rows of x, with ld_x = D_in + pad_x (1e30 in the padding) and y [N + extra_rows][d_out
    + pad_y] pre-filled with SENTINEL -> (rc, the whole y buffer)."""
    import torch
    d_in = x.shape[1]
    xp = np.full((max(N, 1), d_in + pad_x), 1e30)
    xp[:N, :d_in] = x[:N]
    x_d = torch.as_tensor(xp).to("cuda:0")
    y_d = torch.full((N + extra_rows, d_out + pad_y), SENTINEL, dtype=torch.float32, device="cuda:0")
    rc = lib.payne_lnmlp_eval(h, x_d.data_ptr(), x_d.stride(0), N, y_d.data_ptr(), y_d.stride(0), None)
    torch.cuda.synchronize()
    return rc, y_d.cpu().numpy()


@pytest.mark.parametrize("name", sorted(G18))
def test_g18_through_the_abi(lib, g18, name):
    """Both fixture networks at N in {1, 63, 64, 65, 257}, ld_x > D_in, ld_y > D_out: within 4 dev of the reference in fp64; the
    columns from D_out on and the rows from N on keep the sentinel; a second call returns the same bits."""
    arrs, x, y64, dev = g18_net(g18, name)
    layers = layers_of(arrs, G18[name])
    d_out = y64.shape[1]
    rc, h = create(lib, layers)
    assert rc == 0 and h.value
    try:
        worst = 0.0
        for N in TILE_N:
            rc, y = evaluate(lib, h, x, N, d_out)
            assert rc == 0
            assert np.all(y[:, d_out:] == np.float32(SENTINEL)) and np.all(y[N:] == np.float32(SENTINEL)), (name, N)
            err = np.abs(y[:N, :d_out].astype(np.float64) - y64[:N]).max()
            worst = max(worst, err)
            print("g18 %s N=%d: max|y_gpu - y64| = %.3g = %.2f dev" % (name, N, err, err / dev))
            assert err <= BOUND_FACTOR * dev, (name, N, err / dev)
            rc2, y2 = evaluate(lib, h, x, N, d_out)
            assert rc2 == 0 and y2.tobytes() == y.tobytes(), (name, N)
        print("g18 %s: worst ratio %.2f" % (name, worst / dev))
    finally:
        lib.payne_lnmlp_destroy(h)


@pytest.fixture(scope="module")
def default_net():
    """The default shape (6, 256, 256, 256, 8) as MLP_v0 from synth.phot_mlp, 257 rows, the fp64 restatement and torch's CPU
    fp32 evaluation of the same layers (computed once)."""
    import torch
    arrs = synth.phot_mlp(nntype="MLP_v0", seed=5)
    layers = layers_of(arrs, "MLP_v0")
    x = np.random.default_rng(55).normal(0.0, 1.5, (257, 6))
    y64 = forward64(layers, x)
    mods = []
    for W, b, g, be in layers:
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = torch.as_tensor(W.copy()), torch.as_tensor(b.copy())
        mods.append(lin)
        if g is not None:
            ln = torch.nn.LayerNorm(W.shape[0])
            ln.weight.data, ln.bias.data = torch.as_tensor(g.copy()), torch.as_tensor(be.copy())
            mods += [ln, torch.nn.SiLU()]
    with torch.no_grad():
        y32 = torch.nn.Sequential(*mods).eval()(torch.as_tensor(x.astype(np.float32))).numpy()
    return arrs, layers, x, y64, float(np.abs(y32.astype(np.float64) - y64).max())


def test_default_shape_through_the_abi(lib, default_net):
    arrs, layers, x, y64, dev = default_net
    rc, h = create(lib, layers)
    assert rc == 0
    try:
        rc, y = evaluate(lib, h, x, 257, 8)
        assert rc == 0 and np.all(y[:, 8:] == np.float32(SENTINEL)) and np.all(y[257:] == np.float32(SENTINEL))
        err = np.abs(y[:257, :8].astype(np.float64) - y64).max()
        print("default MLP_v0 (6,256,256,256,8) N=257: max|y_gpu - y64| = %.3g = %.2f dev (dev = %.3g, max|y64| = %.3g)"
              % (err, err / dev, dev, np.abs(y64).max()))
        assert err <= BOUND_FACTOR * dev, err / dev
        rc2, y2 = evaluate(lib, h, x, 257, 8)
        assert rc2 == 0 and y2.tobytes() == y.tobytes()
    finally:
        lib.payne_lnmlp_destroy(h)


def test_widest_network_through_the_abi(lib):
    """Widths 512 (the limit: four column tiles a wave, the largest LDS image) and 500 (padded), D_in = 32, D_out = 300, against
    the fp64 restatement with torch's CPU fp32 deviation as the yardstick."""
    import torch
    rng = np.random.default_rng(512)
    dims = [32, 512, 500, 300]
    layers = []
    for i in range(3):
        k = 1.0 / np.sqrt(dims[i])
        W = rng.uniform(-k, k, (dims[i + 1], dims[i])).astype(np.float32)
        b = rng.uniform(-k, k, dims[i + 1]).astype(np.float32)
        hidden = i < 2
        layers.append((W, b, (1 + rng.normal(0, 0.3, dims[i + 1])).astype(np.float32) if hidden else None,
                       rng.normal(0, 0.3, dims[i + 1]).astype(np.float32) if hidden else None))
    x = rng.normal(0, 1.5, (65, 32))
    y64 = forward64(layers, x)
    a = torch.as_tensor(x.astype(np.float32))
    with torch.no_grad():
        for W, b, g, be in layers:
            a = torch.nn.functional.linear(a, torch.as_tensor(W), torch.as_tensor(b))
            if g is not None:
                a = torch.nn.functional.silu(torch.nn.functional.layer_norm(a, (W.shape[0],), torch.as_tensor(g), torch.as_tensor(be)))
    dev = float(np.abs(a.numpy().astype(np.float64) - y64).max())
    rc, h = create(lib, layers)
    assert rc == 0
    try:
        rc, y = evaluate(lib, h, x, 65, 300)
        assert rc == 0 and np.all(y[:, 300:] == np.float32(SENTINEL)) and np.all(y[65:] == np.float32(SENTINEL))
        err = np.abs(y[:65, :300].astype(np.float64) - y64).max()
        print("widths 32-512-500-300 N=65: max|y_gpu - y64| = %.3g = %.2f dev" % (err, err / dev))
        assert err <= BOUND_FACTOR * dev, err / dev
    finally:
        lib.payne_lnmlp_destroy(h)


def test_norm_is_the_plain_pass_in_the_references_fp64_wrapping(lib, g18):
    """norm=True equals norm=False on (x - mid) / std rounded once to fp32, its output times std plus mid in fp64 rounded once:
    the same bits."""
    for name in sorted(G18):
        arrs, x, y64, _ = g18_net(g18, name)
        layers = layers_of(arrs, G18[name])
        d_out = y64.shape[1]
        ni = [arrs["norm_i/" + k.decode()] for k in arrs["label_i"]]
        no = [arrs["norm_o/" + k.decode()] for k in arrs["label_o"]]
        rc, hn = create(lib, layers, norm=(ni, no))
        rc2, hp = create(lib, layers)
        assert rc == 0 and rc2 == 0
        try:
            rc, yn = evaluate(lib, hn, x, 65, d_out)
            rc2, yp = evaluate(lib, hp, norm_in(x[:65], ni).astype(np.float64), 65, d_out)
            assert rc == 0 and rc2 == 0
            want = norm_out(yp[:65, :d_out], no)
            assert np.array_equal(yn[:65, :d_out].view(np.uint32), want.view(np.uint32)), name
            assert np.all(yn[:, d_out:] == np.float32(SENTINEL)) and np.all(yn[65:] == np.float32(SENTINEL))
        finally:
            lib.payne_lnmlp_destroy(hn)
            lib.payne_lnmlp_destroy(hp)


def test_modpred_on_the_device(default_net, g18, tmp_path):
    """modpred from a file: pred on a list, a 1-D and a 2-D array (squeezed fp32 numpy, the argument unchanged) and on a device
    tensor (a device tensor back); getPhot's keys and shapes; norm=True equal to norm=False wrapped in the reference's fp64
    arithmetic, bit for bit."""
    import torch
    from Payne.predict.photANN_new import modpred
    arrs, layers, x, y64, dev = default_net
    path = str(tmp_path / "phot.npz")
    np.savez(path, **arrs)
    P = modpred(nnpath=path, nntype="MLP_v0")
    x2 = x.copy()
    y = P.pred(x2)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (257, 8) and np.array_equal(x2, x)
    assert np.abs(y.astype(np.float64) - y64).max() <= BOUND_FACTOR * dev
    y1 = P.pred(list(x[5]))
    assert y1.shape == (8,) and np.array_equal(y1, y[5])
    assert np.array_equal(P.pred(x[5]), y[5])
    x_d = torch.as_tensor(x).to("cuda:0")
    y_d = P.pred(x_d)
    assert isinstance(y_d, torch.Tensor) and y_d.is_cuda and y_d.dtype == torch.float32 and y_d.shape == (257, 8)
    assert np.array_equal(y_d.cpu().numpy(), y)
    assert P.pred(x_d[5]).shape == (8,)
    out = P.getPhot(x[5])
    assert list(out) == ['teff', 'logg', 'feh', 'afe', 'av', 'rv'] + synth.PHOT_FILTERS + ['band7']
    assert all(np.ndim(v) == 0 for v in out.values()) and out['av'] == x[5, 4] and out['band7'] == y[5, 7]
    out = P.getPhot(x[:9])
    assert all(v.shape == (9,) for v in out.values()) and np.array_equal(out['Bessell_B'], y[:9, 0])
    # norm=True
    Pn = modpred(nnpath=path, nntype="MLP_v0", norm=True)
    ni, no = Pn.anns.norm_i, Pn.anns.norm_o
    xn = norm_in(x, ni)
    yn = Pn.pred(x)
    assert np.array_equal(yn, norm_out(P.pred(xn.astype(np.float64)), no))
    # the other type, from the fixture's arrays
    a1, x1, y641, dev1 = g18_net(g18, "v1")
    y1 = modpred(nnpath=a1, nntype="MLP_v1").pred(x1)
    assert np.abs(y1.astype(np.float64) - y641).max() <= BOUND_FACTOR * dev1


def test_return_codes_without_a_launch(lib, g18):
    from thepayne_amd import _lib
    import torch
    arrs, x, y64, _ = g18_net(g18, "v0")
    layers = layers_of(arrs, "MLP_v0")
    rc, h = create(lib, layers)
    assert rc == 0
    try:
        rc, y = evaluate(lib, h, x, 0, 3)
        assert rc == 0 and np.all(y == np.float32(SENTINEL))                       # N == 0: nothing launched, nothing written
        assert lib.payne_lnmlp_eval(h, None, 5, 0, None, 3, None) == 0
        y_d = torch.full((4, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
        x_d = torch.zeros((4, 5), dtype=torch.float64, device="cuda:0")
        assert lib.payne_lnmlp_eval(None, x_d.data_ptr(), 5, 4, y_d.data_ptr(), 3, None) == _lib.E_INVALID    # NULL handle
        assert lib.payne_lnmlp_eval(h, x_d.data_ptr(), 4, 4, y_d.data_ptr(), 3, None) == _lib.E_INVALID       # ld_x < D_in
        assert lib.payne_lnmlp_eval(h, x_d.data_ptr(), 5, 4, y_d.data_ptr(), 2, None) == _lib.E_INVALID       # ld_y < D_out
        assert lib.payne_lnmlp_eval(h, x_d.data_ptr(), 5, -1, y_d.data_ptr(), 3, None) == _lib.E_INVALID
        assert lib.payne_lnmlp_eval(h, None, 5, 4, y_d.data_ptr(), 3, None) == _lib.E_INVALID
        torch.cuda.synchronize()
        assert np.all(y_d.cpu().numpy() == np.float32(SENTINEL))
    finally:
        lib.payne_lnmlp_destroy(h)
    lib.payne_lnmlp_destroy(None)
    rng = np.random.default_rng(0)

    def net(dims):
        out = []
        for i in range(len(dims) - 1):
            hidden = i < len(dims) - 2
            out.append((rng.normal(0, 0.1, (dims[i + 1], dims[i])), np.zeros(dims[i + 1]),
                        np.ones(dims[i + 1]) if hidden else None, np.zeros(dims[i + 1]) if hidden else None))
        return out
    for dims in ([6, 513, 8], [6, 16, 513], [33, 16, 8], [6, 8]):                   # a width of 513, 33 inputs, one layer
        rc, hh = create(lib, net(dims))
        assert rc == _lib.E_UNSUPPORTED and not hh.value, dims
        assert lib.payne_last_error(None).startswith(b"payne_lnmlp_create: "), dims    # the message of a create that had no context
    d, keep = make_desc(net([6] + [8] * 8))
    d.n_layers = 9                                                                 # nine layers
    assert lib.payne_lnmlp_create(0, C.byref(d), C.byref(C.c_void_p())) == _lib.E_UNSUPPORTED
    ok = net([6, 512, 512])
    rc, hh = create(lib, ok)
    assert rc == 0
    lib.payne_lnmlp_destroy(hh)
    bad = net([6, 16, 8])
    bad[1] = (bad[1][0][:, :15], bad[1][1], None, None)                            # 15 inputs after 16 outputs
    assert create(lib, bad)[0] == _lib.E_INVALID
    bad = net([6, 16, 8])
    bad[0] = (bad[0][0], bad[0][1], None, None)                                    # a hidden layer without LayerNorm
    assert create(lib, bad)[0] == _lib.E_INVALID
    assert lib.payne_lnmlp_create(0, None, C.byref(C.c_void_p())) == _lib.E_INVALID
