"""Label gradients of the spectral networks and Fisher forecasts on the MI355X: payne_specjac_* and payne_fisher_batch
(csrc/k_specjac.hip) through the ABI, PayneSpecPredict.predictgrad / getgrad and fitting.forecast.Forecast.

The yardstick, the kink rule and the references are those of tests/test_specjac.py, whose helpers are shared: torch's jvp on the
CPU in fp64 and fp32 on the restatement of tests/test_trainspec.py, E(ours) <= 4 x E(torch CPU fp32) for the Jacobian (physical and
PAYNE_JAC_ENCODED) and for y.  getgrad is held to the numpy oracle's own getspec applied to the fp64 Jacobian rows, within the
bound the payne_smooth_batch parity tests hold for fluxes of order one (tests/test_gpu_parity.py FLUX_TOL = 1e-6), relative to
max|row|.  payne_fisher_batch is held to numpy.einsum in fp64 on the same fp32 rows within n 2^-52 sum|a_i a_j w|, the bound of a
reordered fp64 sum.  Every measured ratio is printed (NOTES.md quotes them)."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import synth
from test_specjac import Reference, g20_reference, synth_layers, jac_numpy64, encode32, decode
from test_trainspec import G20, ACT, random_net

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
FLUX_TOL = 1e-6                                      # tests/test_gpu_parity.py
TORCH_FP32_FLUX_TOL = 2e-6                           # tests/test_gpu_parity.py
TILE_N = (1, 31, 32, 33, 64, 65, 130)


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_trainspec")


@pytest.fixture(scope="module")
def lib():
    from thepayne_amd import _lib
    return _lib.load()


def make_desc(layers, act):
    from thepayne_amd import _lib
    keep = [tuple(np.ascontiguousarray(a, dtype=np.float32) for a in L) for L in layers]
    d = _lib.SpecmlpDesc()
    d.n_layers, d.act = len(keep), act
    for i, (w, b) in enumerate(keep):
        d.layers[i].n_out, d.layers[i].n_in = w.shape
        d.layers[i].w, d.layers[i].b = w.ctypes.data, b.ctypes.data
    return d, keep


def create(lib, layers, nntype, xmin, xmax, max_rows):
    d, keep = make_desc(layers, ACT["LinNet" if nntype == "LinNet" else "SMLP"])
    xmin, xmax = np.ascontiguousarray(xmin, dtype=np.float64), np.ascontiguousarray(xmax, dtype=np.float64)
    h = C.c_void_p()
    rc = lib.payne_specjac_create(0, C.byref(d), xmin.ctypes.data, xmax.ctypes.data, max_rows, C.byref(h))
    assert rc == 0 and h.value, rc
    return h


def evaluate(lib, h, x, N, d_out, encoded, want_y=True, pads=(3, 7, 5)):
    """payne_specjac_eval on the first N stars into guarded buffers (ld_x = D + 3, ld_y = D_out + 7, ld_j = D_out + 5, one more
    star behind the last) -> (y or None, J [N, D, D_out]); asserts that nothing beyond D_out columns and N stars was written."""
    import torch
    D = x.shape[1]
    xp = np.full((max(N, 1), D + pads[0]), 1e30)
    xp[:N, :D] = x[:N]
    x_d = torch.as_tensor(xp).to("cuda:0")
    y_d = torch.full((N + 1, d_out + pads[1]), SENTINEL, dtype=torch.float32, device="cuda:0")
    j_d = torch.full((N + 1, D, d_out + pads[2]), SENTINEL, dtype=torch.float32, device="cuda:0")
    rc = lib.payne_specjac_eval(h, x_d.data_ptr(), x_d.stride(0), N, y_d.data_ptr() if want_y else None, y_d.stride(0), j_d.data_ptr(),
                                j_d.stride(1), 1 if encoded else 0, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    y, J = y_d.cpu().numpy(), j_d.cpu().numpy()
    assert np.all(y[:N, d_out:] == SENTINEL) and np.all(y[N] == SENTINEL) and np.all(J[:N, :, d_out:] == SENTINEL) and np.all(J[N] == SENTINEL)
    if not want_y:
        assert np.all(y == SENTINEL)
    return (np.ascontiguousarray(y[:N, :d_out]) if want_y else None), np.ascontiguousarray(J[:N, :, :d_out])


def one_call(lib, ref, N, encoded, max_rows=None, want_y=True):
    h = create(lib, ref.layers, ref.nntype, ref.xmin, ref.xmax, max_rows or max(N, 1))
    try:
        return evaluate(lib, h, ref.x, N, ref.layers[-1][0].shape[0], encoded, want_y=want_y)
    finally:
        lib.payne_specjac_destroy(h)


# ---- 1. the fixture's networks through the ABI -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G20))
def test_g20_networks_through_the_abi(lib, g20, name):
    """The fixture's rows exactly (xmin = -s / 2, xmax = s / 2 with s a power of two: raw = s e encodes back to e without rounding)
    and label scales 1 / s that differ per label."""
    base = g20_reference(g20, name)
    D = base.x.shape[1]
    s = np.array([4096.0, 4.0, 2.0, 0.5, 2.0])[:D]
    ref = Reference("g20 " + name, base.layers, base.nntype, base.x * s, -0.5 * s, 0.5 * s)
    assert np.array_equal(ref.e32, base.e32)
    worst = 0.0
    for N in TILE_N:
        for encoded in (False, True):
            y, J = one_call(lib, ref, N, encoded)
            rj, ry = ref.check("ABI", y, J, encoded, n=N)
            worst = max(worst, rj or 0.0, ry or 0.0)
    print("g20 %s: the largest ratio %.2f" % (name, worst))
    y, J = one_call(lib, ref, 65, False)
    y0, J0 = one_call(lib, ref, 65, False, want_y=False)               # y_dev = NULL
    assert y0 is None and J0.tobytes() == J.tobytes()


# ---- 2. ragged shapes ---------------------------------------------------------------------------------------------------
RAGGED = [(nntype, 4, d_out) for nntype in ("SMLP", "LinNet") for d_out in (1, 31, 128, 129, 513, 1100)] + [("SMLP", 5, 129), ("LinNet", 5, 129)]


@pytest.mark.parametrize("nntype,d_in,d_out", RAGGED)
def test_ragged_shapes(lib, nntype, d_in, d_out):
    """The project's set D-33-512-40-D_out, 65 stars: six workgroups of 12 stars at D_in = 4 (seven of 10 at D_in = 5), the last
    with five; the 512-wide layer takes the four-column-tiles-a-wave form of the hidden launch."""
    rng = np.random.default_rng(1000 * d_in + d_out)
    layers = random_net(rng, [d_in, 33, 512, 40, d_out])
    xmin, xmax = np.append(synth.SPEC_LABEL_MIN, 0.5)[:d_in], np.append(synth.SPEC_LABEL_MAX, 2.5)[:d_in]
    ref = Reference("%s %d-33-512-40-%d" % (nntype, d_in, d_out), layers, nntype, decode(rng.uniform(-0.5, 0.5, (65, d_in)), xmin, xmax), xmin, xmax)
    for encoded in (False, True):
        y, J = one_call(lib, ref, 65, encoded)
        ref.check("ABI", y, J, encoded)


@pytest.mark.parametrize("D", (4, 5))
def test_yst1_shape(lib, D):
    """D-300-300-1100, three layers, leaky: synth.make_yst_net."""
    net = synth.make_yst_net(npix=1100, H=300, seed=4, D=D)
    layers = synth_layers(net, "YST1")
    assert [W.shape for W, b in layers] == [(300, D), (300, 300), (1100, 300)]
    rng = np.random.default_rng(40 + D)
    ref = Reference("YST1 %d-300-300-1100" % D, layers, "YST1", decode(rng.uniform(-0.5, 0.5, (65, D)), net["x_min"], net["x_max"]), net["x_min"], net["x_max"])
    for encoded in (False, True):
        y, J = one_call(lib, ref, 65, encoded)
        ref.check("ABI", y, J, encoded)


# ---- 3. mechanics -------------------------------------------------------------------------------------------------------
def test_chunks_and_a_second_handle_return_the_same_bytes(lib, g20):
    ref = g20_reference(g20, "smlp")
    y, J = one_call(lib, ref, 130, False, max_rows=130)
    for max_rows in (16, 1, 130):                                       # (S = 10 stars a tile: 20-, 10- and 130-star passes)
        y2, J2 = one_call(lib, ref, 130, False, max_rows=max_rows)
        assert y2.tobytes() == y.tobytes() and J2.tobytes() == J.tobytes(), max_rows


def test_invalid_and_unsupported_arguments(lib, g20):
    import torch
    from thepayne_amd import _lib
    ref = g20_reference(g20, "linnet")
    layers, D, P = ref.layers, 4, 150
    xmin, xmax = np.full(8, -0.5), np.full(8, 0.5)
    h = C.c_void_p()

    def rc_create(layers=layers, act=1, xmin=xmin, xmax=xmax, max_rows=8, d=None, out=True, edit=None):
        desc, keep = make_desc(layers, act)
        if edit:
            edit(desc)
        return lib.payne_specjac_create(0, C.byref(desc) if d is None else d, None if xmin is None else xmin.ctypes.data,
                                        None if xmax is None else xmax.ctypes.data, max_rows, C.byref(h) if out else None)
    assert lib.payne_specjac_create(0, None, xmin.ctypes.data, xmax.ctypes.data, 8, C.byref(h)) == _lib.E_INVALID
    assert rc_create(xmin=None) == _lib.E_INVALID and rc_create(xmax=None) == _lib.E_INVALID and rc_create(out=False) == _lib.E_INVALID
    assert rc_create(edit=lambda d: setattr(d.layers[1], "n_out", 0)) == _lib.E_INVALID
    assert rc_create(edit=lambda d: setattr(d.layers[2], "n_in", 7)) == _lib.E_INVALID
    assert rc_create(edit=lambda d: setattr(d.layers[0], "w", None)) == _lib.E_INVALID
    assert rc_create(edit=lambda d: setattr(d.layers[5], "b", None)) == _lib.E_INVALID
    assert rc_create(act=2) == _lib.E_INVALID and rc_create(max_rows=0) == _lib.E_INVALID
    bad = xmin.copy()
    bad[2] = np.nan
    assert rc_create(xmin=bad) == _lib.E_INVALID and rc_create(xmax=xmin) == _lib.E_INVALID
    bad = xmax.copy()
    bad[0] = np.inf
    assert rc_create(xmax=bad) == _lib.E_INVALID
    rng = np.random.default_rng(0)
    assert rc_create(edit=lambda d: setattr(d, "n_layers", 1)) == _lib.E_UNSUPPORTED
    assert rc_create(edit=lambda d: setattr(d, "n_layers", 9)) == _lib.E_UNSUPPORTED
    assert rc_create(layers=random_net(rng, [9, 8, 10])) == _lib.E_UNSUPPORTED
    assert rc_create(layers=random_net(rng, [4, 513, 10])) == _lib.E_UNSUPPORTED
    assert lib.payne_last_error(None).startswith(b"payne_specjac_create: ")        # the message of a create that had no context
    assert rc_create(layers=random_net(rng, [4, 512, 10])) == 0 and h.value
    lib.payne_specjac_destroy(h)
    assert rc_create(layers=random_net(rng, [8, 2, 10])) == 0 and h.value
    lib.payne_specjac_destroy(h)
    assert rc_create(layers=random_net(rng, [4, 2, 65537])) == _lib.E_UNSUPPORTED
    lib.payne_specjac_destroy(None)
    # eval
    h = create(lib, layers, "LinNet", xmin[:D], xmax[:D], 8)
    try:
        x_d = torch.zeros((4, D), dtype=torch.float64, device="cuda:0")
        y_d = torch.full((4, P), SENTINEL, dtype=torch.float32, device="cuda:0")
        j_d = torch.full((4, D, P), SENTINEL, dtype=torch.float32, device="cuda:0")
        ev = lambda hh=h, x=x_d.data_ptr(), ld_x=D, N=4, y=y_d.data_ptr(), ld_y=P, j=j_d.data_ptr(), ld_j=P, flags=0: \
            lib.payne_specjac_eval(hh, x, ld_x, N, y, ld_y, j, ld_j, flags, None)
        for rc in (ev(hh=None), ev(N=-1), ev(flags=2), ev(flags=3), ev(ld_x=D - 1), ev(ld_j=P - 1), ev(ld_y=P - 1), ev(x=None), ev(j=None)):
            assert rc == _lib.E_INVALID
        assert ev(N=0, x=None, y=None, j=None) == 0 and ev(y=None, ld_y=0) == 0
        torch.cuda.synchronize()
        assert torch.all(y_d == SENTINEL).item() and not torch.any(j_d == SENTINEL).item()
    finally:
        lib.payne_specjac_destroy(h)
    # Fisher
    r_d = torch.zeros((2, 4, 10), dtype=torch.float32, device="cuda:0")
    w_d = torch.ones(10, dtype=torch.float64, device="cuda:0")
    F_d = torch.full((2, 4, 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    fi = lambda r=r_d.data_ptr(), ld=10, K=4, n=10, B=2, w=w_d.data_ptr(), F=F_d.data_ptr(): lib.payne_fisher_batch(0, r, ld, K, n, B, w, F, None)
    for rc in (fi(K=0), fi(n=0), fi(B=-1), fi(ld=9), fi(r=None), fi(w=None), fi(F=None)):
        assert rc == _lib.E_INVALID
    assert fi(K=17) == _lib.E_UNSUPPORTED and fi(B=0, r=None, w=None, F=None) == 0
    torch.cuda.synchronize()
    assert torch.all(F_d == SENTINEL).item()
    assert fi() == 0
    torch.cuda.synchronize()
    assert torch.all(F_d == 0.0).item()


# ---- 4. getgrad ---------------------------------------------------------------------------------------------------------
def smooth_linnet(npix=4096, seed=6):
    """A LinNet whose spectra and label derivatives are resolved by the model grid, as an emulator's are (the grid has three
    pixels per resolution element): synth.make_torch_net's output weights, white noise along the pixels, smoothed with a Gaussian
    of eight pixels.  The broadening then leaves a derivative row of the order of its own size, and max|row| is a fair scale."""
    net = synth.make_torch_net("LinNet", npix=npix, H=(16, 16, 16), seed=seed)
    k = np.exp(-0.5 * (np.arange(-32, 33) / 8.0) ** 2)
    W = net["lin6.weight"].astype(np.float64)
    W = np.stack([np.convolve(W[:, j], k / np.sqrt((k ** 2).sum()), mode="same") for j in range(W.shape[1])], axis=1)
    net["lin6.weight"] = np.ascontiguousarray(W, dtype=np.float32)
    return net


@pytest.mark.parametrize("stage", (1, 2))
def test_getgrad_against_the_oracle_chain(monkeypatch, stage):
    import oracle.payne_oracle as PO
    from Payne.predict.predictspec import PayneSpecPredict
    net = smooth_linnet()
    layers = synth_layers(net, "LinNet")
    wave = net["wavelength"]
    P = PayneSpecPredict(net, NNtype="LinNet", b_max=16)
    labels = np.array([5432.1, 4.3, -0.4, 0.15])
    kw = dict(Teff=labels[0], logg=labels[1], feh=labels[2], afe=labels[3], rot_vel=18.0, rad_vel=23.0)
    okw = dict(rot_vel=18.0, rad_vel=23.0)
    if stage == 2:
        outwave = synth.obs_grid(wave, 1100)
        outwave = np.concatenate([[wave[0] * 0.99995], outwave, [wave[-1] * 1.0003]])     # the ends leave the model's range
        kw.update(inst_R=21000.0, outwave=outwave)
        okw.update(inst_R=21000.0, outwave=outwave)
    w, flux, dflux = P.getgrad(**kw)
    w2, flux2 = P.getspec(**kw)
    assert np.array_equal(w, w2) and flux.tobytes() == flux2.tobytes()
    assert dflux.shape == (4, len(w)) and len(w) == (4096 if stage == 1 else 1102)
    e32 = encode32(labels[None, :], net["xmin"], net["xmax"])
    J64 = jac_numpy64(layers, "LinNet", e32)[1][0] / (net["xmax"] - net["xmin"])[:, None]
    given = {}
    monkeypatch.setattr(PO, "ann_forward", lambda net_, lab: given["spec"].copy())
    nan = np.isnan(flux)
    assert nan.sum() == (0 if stage == 1 else 2)
    for k in range(4):
        given["spec"] = J64[k]
        ow, row = PO.getspec(net, **okw)
        assert np.array_equal(np.isnan(row), nan) and np.array_equal(np.isnan(dflux[k]), nan)
        err = np.abs(dflux[k] - row)[~nan].max() / np.abs(row[~nan]).max()
        print("getgrad stage %d label %d: %.3g of max|row| (bound %.1g); max|row| %.3g of the network's row" % (stage, k, err, FLUX_TOL, np.abs(row[~nan]).max() / np.abs(J64[k]).max()))
        assert err <= FLUX_TOL, (stage, k, err)
    # predictgrad: one star and a batch, host and device
    import torch
    y1, j1 = P.predictgrad(labels)
    yb, jb = P.predictgrad(torch.as_tensor(np.stack([labels, labels + [100.0, 0.1, 0.1, 0.05]])).to("cuda:0"))
    assert y1.shape == (4096,) and j1.shape == (4, 4096) and yb.is_cuda and jb.shape == (2, 4, 4096)
    assert np.array_equal(yb[0].cpu().numpy(), y1) and np.array_equal(jb[0].cpu().numpy(), j1)
    # predictspec is the likelihood's forward pass (another kernel, operands split in fp16 parts): the two meet within the bound
    # tests/test_gpu_parity.py holds that pass to against torch's fp32 forward
    assert np.abs(y1 - P.predictspec(labels)).max() <= TORCH_FP32_FLUX_TOL


# ---- 5. Fisher matrices -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 4, 5, 16))
@pytest.mark.parametrize("n", (1, 63, 1100, 3600))
def test_fisher_against_einsum(lib, K, n):
    import torch
    rng = np.random.default_rng(100 * K + n)
    B, ld = 3, n + 5
    rows = np.full((B, K, ld), np.float32(1e30))
    rows[:, :, :n] = (rng.normal(0, 1, (B, K, n)) * 10.0 ** rng.uniform(-4, 0, (1, K, 1))).astype(np.float32)
    rows = rows.astype(np.float32)
    w = 1.0 / rng.uniform(0.005, 0.05, n) ** 2
    zero = rng.uniform(size=n) < 0.1
    if n > 1:
        w[zero] = 0.0
    rows[1, :, :n][:, w == 0.0] = np.nan                                # NaN where the weight is zero: skipped
    r_d, w_d = torch.as_tensor(rows).to("cuda:0"), torch.as_tensor(w).to("cuda:0")

    def run(r_d):
        F_d = torch.full((B + 1, K, K), SENTINEL, dtype=torch.float64, device="cuda:0")
        assert lib.payne_fisher_batch(0, r_d.data_ptr(), ld, K, n, B, w_d.data_ptr(), F_d.data_ptr(), None) == 0
        torch.cuda.synchronize()
        F = F_d.cpu().numpy()
        assert np.all(F[B] == SENTINEL)
        return F[:B]
    F = run(r_d)
    a = np.nan_to_num(rows[:, :, :n].astype(np.float64), nan=0.0)
    want = np.einsum("bip,bjp,p->bij", a, a, w)
    bound = n * 2.0 ** -52 * np.einsum("bip,bjp,p->bij", np.abs(a), np.abs(a), w)
    assert np.all(np.isfinite(F)) and np.all(np.abs(F - want) <= bound), float((np.abs(F - want) / np.maximum(bound, 1e-300)).max())
    print("Fisher K=%d n=%d: max |dF| / bound = %.3g" % (K, n, float((np.abs(F - want) / np.maximum(bound, 1e-300)).max())))
    assert np.array_equal(F, np.swapaxes(F, 1, 2)) and run(r_d).tobytes() == F.tobytes()
    if n > 1:                                                           # one NaN where w > 0: that star's row i and column i only
        i, p = K // 2, int(np.flatnonzero(w > 0)[0])
        rows2 = rows.copy()
        rows2[2, i, p] = np.nan
        F2 = run(torch.as_tensor(rows2).to("cuda:0"))
        hit = np.zeros((B, K, K), dtype=bool)
        hit[2, i, :] = hit[2, :, i] = True
        assert np.array_equal(np.isnan(F2), hit) and np.array_equal(F2[~hit], F[~hit])


# ---- 6. Forecast --------------------------------------------------------------------------------------------------------
def test_forecast_end_to_end():
    import torch
    from thepayne_amd.fitting.forecast import Forecast
    from thepayne_amd.predict._spec import fisher_batch
    net = synth.make_torch_net("SMLP", npix=1024, H=(24, 20, 16), seed=9)
    wave = net["wavelength"]
    obs_wave = synth.obs_grid(wave, 300)
    rng = np.random.default_rng(64)
    eflux = rng.uniform(0.005, 0.02, 300)
    eflux[[3, 77, 150]] = [0.0, np.nan, np.inf]
    N = 64
    pars = np.full((N, 8), np.nan)
    pars[:, :4] = decode(rng.uniform(-0.4, 0.4, (N, 4)), net["xmin"], net["xmax"])
    pars[:, 4], pars[:, 5], pars[:, 7] = rng.uniform(-30, 30, N), rng.uniform(3, 30, N), 21000.0
    fc = Forecast(net, "SMLP", obs_wave, eflux, b_max=64)               # (16 stars a call of the engine: four batches)
    rows = fc.jacobian(pars)
    assert rows.shape == (N, 4, 300) and rows.dtype == torch.float32 and rows.is_cuda and torch.all(torch.isfinite(rows)).item()
    F = fc.fisher(pars)
    assert F.shape == (N, 4, 4) and F.dtype == torch.float64
    assert F.cpu().numpy().tobytes() == fisher_batch(rows, torch.as_tensor(fc.weights).to("cuda:0")).cpu().numpy().tobytes()
    assert fc.weights[3] == fc.weights[77] == fc.weights[150] == 0.0 and (fc.weights > 0).sum() == 297
    # a batch boundary changes nothing: the same stars one at a time
    one = torch.cat([fc.jacobian(pars[i:i + 1]) for i in (0, 15, 16, 63)])
    assert one.cpu().numpy().tobytes() == rows[[0, 15, 16, 63]].cpu().numpy().tobytes()
    c = fc.crlb(pars)
    Fh = F.cpu().numpy()
    want = np.sqrt(np.stack([np.diag(np.linalg.inv(Fi)) for Fi in Fh]))
    assert c.shape == (N, 4) and np.all(np.isfinite(c)) and np.all(c > 0) and np.abs(c / want - 1.0).max() <= 1e-10
    half = Forecast(net, "SMLP", obs_wave, eflux / 2.0, b_max=64).crlb(pars)
    assert np.abs(half / (c / 2.0) - 1.0).max() <= 1e-12
    extra = rng.normal(0, 1, (N, 2, 300)).astype(np.float32)
    F6 = fc.fisher(pars, extra_rows=extra).cpu().numpy()
    assert F6.shape == (N, 6, 6) and F6[:, :4, :4].tobytes() == Fh.tobytes() and fc.crlb(pars, extra_rows=extra).shape == (N, 6)
    assert np.all(fc.crlb(pars, extra_rows=extra)[:, :4] >= c * (1 - 1e-9))   # marginalising over more parameters never tightens a bound
