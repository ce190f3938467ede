"""Label gradients of the spectral networks and Fisher forecasts -- what runs without a GPU: the fp64 statement of the forward-mode
pass against torch's jvp, the kernels' arithmetic (csrc/specjac_core.hpp) executed on the host under ASan / UBSan
(tests/emul/specjac_emul.cpp), the linearity of everything getspec does after the network (on the numpy oracle alone), and the
host logic of getgrad and Forecast.  The kernels themselves: tests/test_specjac_gpu.py, which shares the helpers defined here.

Yardstick: the project's (tests/test_trainspec.py).  For the Jacobian the named tensors are its D_in label planes J[:, k, :], for y
the one array; E(a) = max over tensors of max|a - a64| / max|a64|, a64 torch.autograd.functional.jvp (or the forward) on the CPU in
.double() on the restatement of tests/test_trainspec.py and the same fp32 encoded labels, and every bound is
    E(ours) <= BOUND_FACTOR x E(torch CPU fp32).
LeakyReLU kinks: a hidden pre-activation that rounding moves across zero changes a tangent by a factor of 100, which says nothing
about the arithmetic.  For leaky networks only stars whose fp64 hidden pre-activations all lie further than 1e-5 max|z| of their
layer from zero are compared, and at most 10 % of a test's stars may be left out that way (asserted).  Sigmoid networks leave
nothing out."""
import os
import subprocess

import numpy as np
import pytest

from thepayne_amd import nnio, synth
from test_lnmlp import BOUND_FACTOR
from test_trainspec import G20, ACT, g20_net, restatement, random_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINK_MARGIN = 1e-5
KINK_CAP = 0.10


# ---- references ---------------------------------------------------------------------------------------------------------
def encode32(x, xmin, xmax):
    return ((np.asarray(x, dtype=np.float64) - xmin) / (np.asarray(xmax, dtype=np.float64) - xmin) - 0.5).astype(np.float32)


def decode(e, xmin, xmax):
    """Raw fp64 labels whose encoding is close to e (the encoding of the result is what the references are given)."""
    return (np.asarray(e, dtype=np.float64) + 0.5) * (np.asarray(xmax, dtype=np.float64) - xmin) + xmin


def jac_numpy64(layers, nntype, e):
    """The forward-mode pass in numpy fp64 on encoded rows e [N, D]: (y [N, D_out], J [N, D, D_out] = dy / de, the hidden layers'
    pre-activations)."""
    a = np.asarray(e, dtype=np.float64)
    t, zs = None, []
    for l, (W, b) in enumerate(layers):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
        z = a @ W.T + b
        tz = np.broadcast_to(W.T, (a.shape[0],) + W.T.shape) if l == 0 else t @ W.T
        if l + 1 == len(layers):
            return z, np.ascontiguousarray(tz), zs
        zs.append(z)
        if nntype == "LinNet":
            a = 1.0 / (1.0 + np.exp(-z))
            slope = a * (1.0 - a)
        else:
            a, slope = np.where(z > 0, z, 0.01 * z), np.where(z > 0, 1.0, 0.01)
        t = tz * slope[:, None, :]


def torch_jac(layers, nntype, e32, dtype):
    """(y, J = dy / de) of the restatement by torch.autograd.functional.jvp on the CPU in `dtype`, one call a label."""
    import torch
    model = restatement(layers, "LinNet" if nntype == "LinNet" else "SMLP", dtype)[0]
    x = torch.as_tensor(np.array(e32)).to(dtype)
    J = np.empty((x.shape[0], x.shape[1], layers[-1][0].shape[0]), dtype=np.float64 if dtype == torch.float64 else np.float32)
    for k in range(x.shape[1]):
        v = torch.zeros_like(x)
        v[:, k] = 1.0
        y, jv = torch.autograd.functional.jvp(model, x, v)
        J[:, k, :] = jv.numpy()
    return y.detach().numpy(), J


def kept_stars(zs, nntype, what=""):
    """The stars the kink rule compares; asserts the cap."""
    keep = np.ones(zs[0].shape[0], dtype=bool)
    if nntype != "LinNet":
        for z in zs:
            keep &= np.all(np.abs(z) > KINK_MARGIN * np.abs(z).max(), axis=1)
    left = int((~keep).sum())
    print("%s: %d of %d stars left out by the kink rule" % (what, left, len(keep)))
    assert left <= KINK_CAP * len(keep), (what, left, len(keep))
    return keep


def pooled_planes(a, a64, keep):
    return max(float(np.abs(a[keep, k].astype(np.float64) - a64[keep, k]).max() / np.abs(a64[keep, k]).max()) for k in range(a64.shape[1]))


class Reference(object):
    """The references of one (network, stars) pair, computed once: fp64 and fp32 y and J (encoded and physical), the kept stars."""

    def __init__(self, what, layers, nntype, x, xmin, xmax):
        import torch
        self.what, self.layers, self.nntype = what, layers, nntype
        self.x, self.xmin, self.xmax = np.asarray(x, dtype=np.float64), np.asarray(xmin, dtype=np.float64), np.asarray(xmax, dtype=np.float64)
        self.e32 = encode32(self.x, self.xmin, self.xmax)
        self.y64, self.J64 = torch_jac(layers, nntype, self.e32, torch.float64)
        self.y32, self.J32 = torch_jac(layers, nntype, self.e32, torch.float32)
        self.keep = kept_stars(jac_numpy64(layers, nntype, self.e32)[2], nntype, what)
        s64 = 1.0 / (self.xmax - self.xmin)
        self.J64_phys = self.J64 * s64[None, :, None]
        self.J32_phys = self.J32 * s64.astype(np.float32)[None, :, None]

    def check(self, tag, y, J, encoded, n=None):
        """y (or None) and J of the first n stars inside the yardstick; returns the ratios (J, y)."""
        n = len(self.x) if n is None else n
        keep = self.keep[:n]
        if not keep.any():
            return None, None
        J64, J32 = (self.J64, self.J32) if encoded else (self.J64_phys, self.J32_phys)
        e, e32 = pooled_planes(J, J64[:n], keep), pooled_planes(J32[:n], J64[:n], keep)
        print("%s %s N=%d %s: J E = %.3g = %.2f x torch fp32's %.3g" % (self.what, tag, n, "encoded" if encoded else "physical", e, e / e32, e32))
        assert e <= BOUND_FACTOR * e32, (self.what, tag, n, e / e32)
        ry = None
        if y is not None:
            y64 = self.y64[:n]
            ey, ey32 = np.abs(y - y64).max() / np.abs(y64).max(), np.abs(self.y32[:n] - y64).max() / np.abs(y64).max()
            print("%s %s N=%d: y E = %.3g = %.2f x torch fp32's %.3g" % (self.what, tag, n, ey, ey / ey32, ey32))
            assert ey <= BOUND_FACTOR * ey32, (self.what, tag, n, ey / ey32)
            ry = ey / ey32
        return e / e32, ry


def g20_reference(g20, name):
    """The fixture's network on its 130 encoded rows; xmin = -0.5, xmax = 0.5 make the encoding the identity."""
    layers, x, t = g20_net(g20, name)
    D = x.shape[1]
    return Reference("g20 " + name, layers, G20[name], x.astype(np.float64), np.full(D, -0.5), np.full(D, 0.5))


def synth_layers(net, nntype):
    return [(W, b) for W, b, act in nnio.normalize_spec_net(net, nntype)["layers"]]


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_trainspec")


# ---- 1. the statement of the arithmetic -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G20))
def test_forward_mode_statement_equals_torch_jvp_in_fp64(g20, name):
    import torch
    layers, x, t = g20_net(g20, name)
    y, J, zs = jac_numpy64(layers, G20[name], x)
    y64, J64 = torch_jac(layers, G20[name], x, torch.float64)
    assert np.abs(J - J64).max() <= 1e-12 * np.abs(J64).max() and np.abs(y - y64).max() <= 1e-12 * np.abs(y64).max()
    if name == "smlp":                                                  # the fixture's rows keep clear of the kinks
        assert min(np.abs(z).min() / np.abs(z).max() for z in zs) > KINK_MARGIN


# ---- 2. the kernels' arithmetic on the host --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/specjac_emul.cpp built with the sanitizers; run(layers, nntype, x, xmin, xmax, encoded) -> (y, J)."""
    build = tmp_path_factory.mktemp("specjac_emul")
    exe = str(build / "specjac_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "specjac_emul.cpp")],
                   check=True)
    count = [0]

    def run(layers, nntype, x, xmin, xmax, encoded):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        with open(str(d / "net.txt"), "w") as f:
            f.write("%d %d\n" % (len(layers), ACT["LinNet" if nntype == "LinNet" else "SMLP"]) + "".join("%d %d\n" % (W.shape[1], W.shape[0]) for W, b in layers))
        for l, (W, b) in enumerate(layers):
            np.ascontiguousarray(W, dtype=np.float32).tofile(str(d / ("w%d.bin" % l)))
            np.ascontiguousarray(b, dtype=np.float32).tofile(str(d / ("b%d.bin" % l)))
        for nm, a in (("x", x), ("xmin", xmin), ("xmax", xmax)):
            np.ascontiguousarray(a, dtype=np.float64).tofile(str(d / (nm + ".bin")))
        res = subprocess.run([exe, str(d), str(x.shape[0]), "1" if encoded else "0"], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        N, D, P = x.shape[0], x.shape[1], layers[-1][0].shape[0]
        return np.fromfile(str(d / "y.bin"), dtype=np.float32).reshape(N, P), np.fromfile(str(d / "jac.bin"), dtype=np.float32).reshape(N, D, P)
    return run


@pytest.mark.parametrize("name", sorted(G20))
def test_jacobian_arithmetic_on_the_host(emul, g20, name):
    ref = g20_reference(g20, name)
    for N in (1, 65, 130):
        y, J = emul(ref.layers, ref.nntype, ref.x[:N], ref.xmin, ref.xmax, True)
        ref.check("emulator", y, J, True, n=N)


def test_chunked_output_layer_on_the_host(emul):
    """D_out = 1100: nine 128-column chunks, the last one ragged; physical labels and their scales."""
    rng = np.random.default_rng(1100)
    layers = random_net(rng, [4, 33, 40, 1100])
    xmin, xmax = synth.SPEC_LABEL_MIN[:4], synth.SPEC_LABEL_MAX[:4]
    ref = Reference("D_out=1100", layers, "SMLP", decode(rng.uniform(-0.5, 0.5, (65, 4)), xmin, xmax), xmin, xmax)
    y, J = emul(layers, "SMLP", ref.x, xmin, xmax, False)
    ref.check("emulator", y, J, False)
    yE, JE = emul(layers, "SMLP", ref.x, xmin, xmax, True)
    ref.check("emulator", yE, JE, True)
    assert yE.tobytes() == y.tobytes()


def test_kink_rule_on_the_issue_s_example():
    """synth.make_torch_net('SMLP', npix=1100, H=(300, 300, 300), seed=22) with 96 rows from default_rng(7): 5 of 96 left out."""
    layers = synth_layers(synth.make_torch_net("SMLP", npix=1100, H=(300, 300, 300), seed=22), "SMLP")
    e = np.random.default_rng(7).uniform(-0.5, 0.5, (96, 4)).astype(np.float32)
    keep = kept_stars(jac_numpy64(layers, "SMLP", e)[2], "SMLP", "SMLP 300")
    assert (~keep).sum() == 5


# ---- 3. everything after the network is linear ------------------------------------------------------------------------------
def test_getspec_is_linear_behind_the_network(monkeypatch):
    """Central differences of the oracle's getspec in one encoded label (h = 1e-4; truncation O(h^2) ~ 1e-8, rounding 1e-16 / h =
    1e-12, both relative) against the oracle's own broadening chain applied to the fp64 Jacobian row: within 1e-6 max|row|."""
    import oracle.payne_oracle as PO
    net = synth.make_torch_net("LinNet", npix=1000, H=(12, 10, 8), seed=3)
    layers = synth_layers(net, "LinNet")
    xmin, xmax = net["xmin"], net["xmax"]
    e0 = np.array([0.11, -0.2, 0.3, -0.05])
    wave = net["wavelength"]
    outwave = np.linspace(wave[0] - 0.3, wave[-1] + 0.3, 777)          # not 2^k pixels; both ends leave the model's range
    given = {}
    monkeypatch.setattr(PO, "ann_forward", lambda net_, labels: given["spec"].copy())

    def chain(spec):
        given["spec"] = np.asarray(spec, dtype=np.float64)
        return PO.getspec(net, rot_vel=35.0, rad_vel=-42.0, inst_R=21000.0, outwave=outwave)[1]
    y0, J, _ = jac_numpy64(layers, "LinNet", e0[None, :])
    base = chain(y0[0])
    nan = np.isnan(base)
    assert 0 < nan.sum() < 100
    h = 1e-4
    for k in range(4):
        ep, em = e0.copy(), e0.copy()
        ep[k] += h
        em[k] -= h
        fd = (chain(jac_numpy64(layers, "LinNet", ep[None, :])[0][0]) - chain(jac_numpy64(layers, "LinNet", em[None, :])[0][0])) / (2 * h)
        row = chain(J[0, k])
        assert np.array_equal(np.isnan(row), nan) and np.array_equal(np.isnan(fd), nan)
        err = np.abs(fd - row)[~nan].max() / np.abs(row[~nan]).max()
        print("label %d: central difference against the chain on the Jacobian row: %.3g of max|row|" % (k, err))
        assert err <= 1e-6, (k, err)
    # the physical derivative is the encoded one over (xmax - xmin)
    assert np.allclose(encode32(decode(e0, xmin, xmax), xmin, xmax), e0.astype(np.float32), atol=1e-7)


# ---- 4. host logic ------------------------------------------------------------------------------------------------------
def test_getgrad_refuses_what_is_not_linear():
    from thepayne_amd.predict._spec import PayneSpecPredict
    P = object.__new__(PayneSpecPredict)
    P.Canns = object()
    with pytest.raises(NotImplementedError):
        P.getgrad(Teff=5000.0)
    P.Canns = None
    with pytest.raises(NotImplementedError):
        P.getgrad(Teff=5000.0, inst_R=np.full(10, 0.1), outwave=np.linspace(5200.0, 5201.0, 10))


def test_forecast_weights_and_singular_fisher(monkeypatch):
    from thepayne_amd.fitting import forecast

    class Stub(object):
        def __init__(self, path, **kw):
            self.anns = type("A", (), {"n_labels": 4})()
    monkeypatch.setattr(forecast, "PayneSpecPredict", Stub)
    e = np.array([0.01, 0.0, np.nan, np.inf, -np.inf, 0.02])
    F = forecast.Forecast("net.npz", "SMLP", np.linspace(5200.0, 5201.0, 6), e)
    assert np.array_equal(F.weights, [1e4, 0.0, 0.0, 0.0, 0.0, 2500.0]) and F.n_labels == 4
    with pytest.raises(ValueError):
        forecast.Forecast("net.npz", "SMLP", np.linspace(5200.0, 5201.0, 5), e)
    good = np.array([[4e-10, 1e-6], [1e-6, 9.0]])
    c = forecast.crlb_from_fisher(np.array([good, np.ones((2, 2)), [[1.0, np.nan], [np.nan, 1.0]], np.zeros((2, 2))]))
    assert np.allclose(c[0], np.sqrt(np.diag(np.linalg.inv(good))), rtol=1e-10, atol=0) and np.all(np.isnan(c[1:]))


def test_reference_import_names_expose_the_new_methods():
    from Payne.predict.ystpred import PayneSpecPredict as Y
    from Payne.predict.predictspec import PayneSpecPredict as T
    for cls in (Y, T):
        assert callable(cls.predictgrad) and callable(cls.getgrad)
    from thepayne_amd import _lib
    assert _lib.JAC_ENCODED == 1 and all(s in _lib.SYMBOLS for s in ("payne_specjac_create", "payne_specjac_eval", "payne_specjac_destroy", "payne_fisher_batch"))
