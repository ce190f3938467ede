"""SED fits on the device: payne_sedfit_jac against the long-double reference and its bound, payne_sedfit_run against the numpy fp64
loop, and SEDFit's public interface.  References, bounds, rows and the fit's rule are tests/test_sedfit.py's."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import _lib
from thepayne_amd.fitting import SEDFit
from test_lmfit import CONVERGED, MAXITER, NAN
import test_sedfit as TS

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_FITTERS = {}


def fitter_of(phot, photscale, key):
    k = (key, bool(photscale))
    if k not in _FITTERS:
        _FITTERS[k] = SEDFit(usebands=phot["filters"], nnpath=phot, photscale=photscale)
    return _FITTERS[k]


# ---- payne_sedfit_jac ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("photscale", (False, True), ids=("dist", "scaled"))
@pytest.mark.parametrize("F,H", TS.JAC_SHAPES, ids=["F%d-H%d" % s for s in TS.JAC_SHAPES])
def test_jac_inside_the_bound_and_bit_stable(F, H, photscale):
    phot, th, ref = TS.jac_case(F, H, photscale)
    fit = fitter_of(phot, photscale, ("jac", F, H))
    full = fit.grad(th)
    for B in TS.JAC_B:
        m, J = fit.grad(th[:B])
        assert m.shape == (B, F) and J.shape == (B, F, th.shape[1])
        TS.check_jac("device F=%d H=%d B=%d" % (F, H, B), m, J, ref, rows=slice(0, B))     # the bound and the NaN pattern
        assert same_bytes(m, full[0][:B]) and same_bytes(J, full[1][:B])                   # the batch does not matter
    again = fit.grad(th)
    assert same_bytes(again[0], full[0]) and same_bytes(again[1], full[1])
    for s in (5, TS.JAC_S + 3, len(th) - 1):                                               # a star alone, from the middle of a tile
        m, J = fit.grad(th[s:s + 1])
        assert same_bytes(m, full[0][s:s + 1]) and same_bytes(J, full[1][s:s + 1])
    finite = np.isfinite(full[1])
    assert finite.any() and (F == 1 or not finite.all())


def test_jac_device_tensors_and_the_width_limit():
    import torch
    phot, th, ref = TS.jac_case(3, 32, False)
    fit = fitter_of(phot, False, ("jac", 3, 32))
    host = fit.grad(th)
    m, J = fit.grad(torch.as_tensor(th).cuda())
    assert isinstance(m, torch.Tensor) and m.is_cuda and J.is_cuda
    assert same_bytes(m.cpu().numpy(), host[0]) and same_bytes(J.cpu().numpy(), host[1])
    # H = 65: PAYNE_E_UNSUPPORTED from the library, NotImplementedError from SEDFit
    wide = TS.make_nets(2, 65)
    lib = _lib.load()
    arrs = [np.ascontiguousarray(wide[k], dtype=np.float32) for k in ("w1", "b1", "w2", "b2", "w3", "b3")] + [wide["xmin"], wide["xmax"], np.ascontiguousarray(wide["hiav"])]
    h = C.c_void_p()
    rc = lib.payne_sedfit_create(0, 2, 65, *[a.ctypes.data_as(C.c_void_p) for a in arrs], C.byref(h))
    assert rc == -2 and not h.value and b"H > 64" in lib.payne_last_error(None)
    with pytest.raises(NotImplementedError):
        SEDFit(usebands=wide["filters"], nnpath=wide)
    assert lib.payne_sedfit_jac(None, None, 1, 0, None, None, None) == -1
    assert lib.payne_sedfit_jac(fit._h, None, 1, 0, None, None, None) == -1 and lib.payne_sedfit_jac(fit._h, None, 0, 0, None, None, None) == 0
    assert lib.payne_sedfit_jac(fit._h, None, 0, 2, None, None, None) == -1


# ---- payne_sedfit_run ---------------------------------------------------------------------------------------------------------------
RUN_MODES = [("scaled", ("logA",)), ("dist", TS.FREE3[False]), ("scaled", TS.FREE3[True]), ("dist", TS.FREE_ALL[False]), ("scaled", TS.FREE_ALL[True])]
RUN_CASES = [(F, H, mode, free) for F, H in TS.FIT_SHAPES for mode, free in RUN_MODES]
_RUNS = {}


def run_inputs(F, H, photscale, free):
    """The CPU file's fixture (24 stars) with two more: star 24 is star 0 with every third filter at w = 0 and NaN magnitudes exactly
    there, star 25 is star 1 with fewer counting filters than parameters and no prior.  Returns (nets, case, references; None for 25)."""
    key = (F, H, photscale, tuple(free))
    if key not in _RUNS:
        phot, case, refs = TS.fit_inputs(F, H, photscale, free)
        c = {k: (np.concatenate([v, v[:2]]) if isinstance(v, np.ndarray) and v.ndim == 2 and len(v) == TS.FIT_N else v) for k, v in case.items()}
        K = len(c["cols"])
        c["w"][24, 1::3] = 0.0
        c["obs"][24, 1::3] = np.nan
        c["w"][25, K - 1:] = 0.0
        if c["sigma"] is not None:
            c["sigma"][25] = np.inf
        r24 = TS.reference_fit(phot, photscale, c, 24)
        _RUNS[key] = (phot, c, list(refs) + [r24, None])
    return _RUNS[key]


def run_raw(fit, c, rows=slice(None), **opts):
    """payne_sedfit_run on the stars `rows` with outputs of this test's own: every array pre-filled with a sentinel and one row longer
    than the batch.  Returns numpy arrays, the sentinel row included."""
    import torch
    fit._setup()
    dev = fit.device
    cols = c["cols"]
    K, P = len(cols), c["start"].shape[1]
    obs, w, start = (torch.as_tensor(np.ascontiguousarray(c[k][rows])).to(dev) for k in ("obs", "w", "start"))
    N = obs.shape[0]
    obs = torch.where(w != 0.0, obs, torch.full_like(obs, float("nan")))                   # NaN exactly where w = 0
    mu = sigma = None
    if c["sigma"] is not None:
        mu, sigma = (torch.as_tensor(np.ascontiguousarray(c[k][rows])).to(dev) for k in ("mu", "sigma"))
    out = dict(pars=torch.full((N + 1, P), SENTINEL, dtype=torch.float64, device=dev), chisq=torch.full((N + 1,), SENTINEL, dtype=torch.float64, device=dev),
               A=torch.full((N + 1, K, K), SENTINEL, dtype=torch.float64, device=dev), status=torch.full((N + 1,), -77, dtype=torch.int32, device=dev),
               niter=torch.full((N + 1,), -77, dtype=torch.int32, device=dev), at_bound=torch.full((N + 1,), -77, dtype=torch.int32, device=dev),
               nfilt=torch.full((N + 1,), -77, dtype=torch.int32, device=dev))
    o = _lib.LmfitOpts(**dict(TS.DEFAULTS, **opts))
    lo, hi = np.ascontiguousarray(c["lo"]), np.ascontiguousarray(c["hi"])
    rc = fit.lib.payne_sedfit_run(fit._h, int(fit.photscale), sum(1 << k for k in cols), start.data_ptr(), obs.data_ptr(), w.data_ptr(), N,
                                  lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), None if mu is None else mu.data_ptr(),
                                  None if sigma is None else sigma.data_ptr(), C.byref(o), *[out[k].data_ptr() for k in ("pars", "chisq", "A", "status", "niter", "at_bound", "nfilt")],
                                  None)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_sentinels(out, N):
    for k, v in out.items():
        tail = v[N]
        assert np.all(tail == (SENTINEL if v.dtype == np.float64 else -77)), k           # nothing behind the batch
    assert not np.any(out["pars"][:N] == SENTINEL) and not np.any(out["chisq"][:N] == SENTINEL) and not np.any(out["A"][:N] == SENTINEL)
    assert not np.any(out["status"][:N] == -77) and not np.any(out["niter"][:N] == -77) and not np.any(out["nfilt"][:N] == -77)


@pytest.mark.parametrize("F,H,mode,free", RUN_CASES, ids=["F%d-H%d-%s-K%d" % (F, H, m, len(f)) for F, H, m, f in RUN_CASES])
def test_run_against_the_fp64_loop(F, H, mode, free):
    photscale = mode == "scaled"
    phot, c, refs = run_inputs(F, H, photscale, free)
    fit = fitter_of(phot, photscale, ("fit", F, H))
    N, K = 26, len(c["cols"])
    out = run_raw(fit, c)
    check_sentinels(out, N)
    what = "device F=%d H=%d %s K=%d" % (F, H, mode, K)
    TS.check_fit(what, {k: v[:24] for k, v in out.items()}, c, refs[:24])
    # the star with filters at w = 0 (and NaN magnitudes there): counted, and compared like the others where the reference converged
    assert out["nfilt"][24] == F - len(range(1, F, 3)) and np.all(out["nfilt"][:24] == F) and out["status"][24] != NAN
    n_prior = 0 if c["sigma"] is None else int(np.isfinite(c["sigma"][24]).sum())
    if out["nfilt"][24] + n_prior < K:                                                    # (F = 7 with all seven free: it is too few itself)
        assert out["status"][24] == TS.TOO_FEW
    elif refs[24]["status"] == CONVERGED:
        TS.check_fit(what + " (w = 0)", {k: v[24:25] for k, v in out.items()}, {"cols": c["cols"]}, [refs[24]], max_left_out=0)
    # too few
    assert out["status"][25] == TS.TOO_FEW and out["niter"][25] == 0 and out["nfilt"][25] == K - 1 and np.isnan(out["chisq"][25]) and not out["A"][25].any()
    assert np.array_equal(out["pars"][25][c["cols"]], np.clip(c["start"][25][c["cols"]], c["lo"], c["hi"]))
    fixed = [p for p in range(c["start"].shape[1]) if p not in c["cols"]]
    assert np.array_equal(out["pars"][:N][:, fixed], c["start"][:, fixed])
    for s in range(24):
        if refs[s]["status"] == CONVERGED:
            d = np.sqrt(np.outer(np.diag(refs[s]["A"]), np.diag(refs[s]["A"])))
            assert np.all(np.abs(out["A"][s] - refs[s]["A"]) <= 1e-6 * d) and np.array_equal(out["A"][s], out["A"][s].T)
    # the same bytes on a second call, and for a star alone
    again = run_raw(fit, c)
    assert all(same_bytes(again[k], out[k]) for k in out)
    for s in (5, 24, 25):
        alone = run_raw(fit, c, rows=slice(s, s + 1))
        check_sentinels(alone, 1)
        assert all(same_bytes(alone[k][:1], out[k][s:s + 1]) for k in out), (what, s)
    # one evaluation
    one = run_raw(fit, c, maxiter=1)
    ran = out["status"][:N] != TS.TOO_FEW
    assert ran[:24].all() and np.all(one["status"][:N][ran] == MAXITER) and np.all(one["niter"][:N][ran] == 1) and np.all(one["status"][:N][~ran] == TS.TOO_FEW)


@pytest.mark.parametrize("photscale", (False, True), ids=("dist", "scaled"))
def test_noiseless_run_ends_at_the_truth(photscale):
    """The CPU file's noiseless case on the device: within 1e-6 marginal sigma of the truth with xtol = 1e-7."""
    F, H = TS.FIT_SHAPES[0]
    phot, case, refs = TS.fit_inputs(F, H, photscale, TS.free_of("three", photscale), noise=0.0, xtol=1e-7)
    out = run_raw(fitter_of(phot, photscale, ("fit", F, H)), case, xtol=1e-7)
    keep = [s for s, r in enumerate(refs) if r["status"] == CONVERGED]
    assert len(keep) >= TS.FIT_N - 2 and all(out["status"][s] == CONVERGED for s in keep)
    d = max(np.max(np.abs(out["pars"][s][case["cols"]] - case["truth"][s][case["cols"]]) / TS.marginal_sigma(refs[s]["A"])) for s in keep)
    print("noiseless on the device: %.3g sigma from the truth" % d)
    assert d <= 1e-6


def test_run_argument_checks():
    phot, c, refs = run_inputs(7, 48, False, TS.FREE3[False])
    fit = fitter_of(phot, False, ("fit", 7, 48))
    fit._setup()
    lib, h = fit.lib, fit._h
    lo, hi = np.ascontiguousarray(c["lo"]), np.ascontiguousarray(c["hi"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    mask = sum(1 << k for k in c["cols"])

    def call(handle=h, photscale=0, mask=mask, B=0, lo=lo, hi=hi, mu=None, sigma=None, opts=None):
        return lib.payne_sedfit_run(handle, photscale, mask, None, None, None, B, p(lo), p(hi), mu, sigma, opts, None, None, None, None, None, None, None, None)
    assert call() == 0                                                                    # B == 0 does nothing
    assert call(handle=None) == -1 and call(B=-1) == -1 and call(photscale=2) == -1 and call(mask=0) == -1 and call(mask=1 << 7) == -1
    assert call(B=3) == -1                                                                # null arrays with B > 0
    assert call(lo=hi, hi=lo) == -1 and call(hi=np.array([hi[0], hi[1], 5.0])) == -1 and call(lo=np.array([np.nan, lo[1], lo[2]])) == -1
    assert call(mu=C.c_void_p(16)) == -1 and call(opts=C.byref(_lib.LmfitOpts(**dict(TS.DEFAULTS, maxiter=0)))) == -1
    assert lib.payne_sedfit_run(h, 0, mask, None, None, None, 0, None, p(hi), None, None, None, None, None, None, None, None, None, None, None) == -1


# ---- SEDFit ---------------------------------------------------------------------------------------------------------------------------
def test_sedfit_public_interface():
    import torch
    F, H = 12, 16
    free = ("Teff", "logR", "Dist", "Av")
    phot, case, refs = TS.fit_inputs(F, H, False, free)
    fit = SEDFit(usebands=phot["filters"], nnpath=phot)
    emags = np.full(case["obs"].shape, TS.SIGMA_MAG)
    mags = case["obs"].copy()
    mags[3, 2], emags[3, 5], emags[3, 6], emags[3, 7] = np.nan, np.inf, 0.0, -1.0
    bounds = {TS.NAMES[False][k]: (l, h) for k, l, h in zip(case["cols"], case["lo"], case["hi"])}
    prior = (case["mu"], case["sigma"])
    res = fit.fit(mags, emags, case["start"], free=free, bounds=bounds, prior=prior)
    assert res["free"] == ("Teff", "logR", "Dist", "Av") and isinstance(res["pars"], np.ndarray)
    assert res["pars"].shape == (TS.FIT_N, 7) and res["err"].shape == (TS.FIT_N, 4) and res["fisher"].shape == (TS.FIT_N, 4, 4)
    assert res["nfilt"][3] == F - 4 and np.all(np.delete(res["nfilt"], 3) == F)
    keep = [s for s in range(TS.FIT_N) if s != 3]
    TS.check_fit("SEDFit.fit", {k: res[k][keep] for k in ("pars", "status", "niter")}, case, [refs[s] for s in keep], max_left_out=2)
    for s in keep:
        if refs[s]["status"] == CONVERGED:                                                # the marginalised errors
            assert np.allclose(res["err"][s], TS.marginal_sigma(refs[s]["A"]), rtol=1e-5)
    dev = fit.fit(torch.as_tensor(mags).cuda(), torch.as_tensor(emags).cuda(), torch.as_tensor(case["start"]).cuda(), free=free, bounds=bounds, prior=prior)
    assert all(isinstance(dev[k], torch.Tensor) and dev[k].is_cuda for k in ("pars", "err", "fisher", "chisq", "nfilt", "status", "niter", "at_bound"))
    assert all(same_bytes(dev[k].cpu().numpy(), res[k]) for k in ("pars", "fisher", "chisq", "status", "niter", "nfilt"))
    m, J = fit.grad(res["pars"])
    m64, J64 = TS.jac_numpy64(phot, res["pars"], False)
    assert np.allclose(m, m64, rtol=0, atol=1e-9) and np.allclose(J, J64, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError):
        fit.fit(mags, emags, case["start"], free=free, bounds=dict(bounds, Av=(0.0, 5.0)), prior=prior)
    with pytest.raises(ValueError):
        fit.fit(mags, emags, case["start"], free=free, bounds=bounds)                     # logR and Dist free without a prior
    fit.close()
