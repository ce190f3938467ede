"""Labels and continuum polynomial in one Levenberg-Marquardt fit on the device: payne_lmfit_update_poly through the C ABI and
OptFit.fit_joint end to end.  The inputs, the references and the bounds are tests/test_lmfit_poly.py's, which checks on the CPU that the
fp64 joint reference loop converges on the inputs fitted here.

Yardstick of fit_joint: d = max_k |x - x*| sqrt(A*_kk) over all K parameters, x* and A* the fp64 joint reference loop's, stays within
1e-2 (10 xtol, the project's bound for device fits); the same numpy loop fed with torch's CPU fp32 model and Jacobian is printed next
to it."""
import numpy as np
import pytest
from numpy.polynomial.chebyshev import chebvander

from thepayne_amd import _lib
from test_lmfit import DEFAULTS, RUNNING, CONVERGED, STEP_TOL, RECOVERY_BMAX, RECOVERY_MAX_EVALS, g20, sigma_distance                         # noqa: F401
from test_contfit import EPS, ALT_STARS, oracle_star
from test_lmfit_poly import (SHAPES, BIG, LINEAR, JOINT_CASES, poly_case, check_poly_tiles, poly_emul, start_of, linear_case, joint_inputs,   # noqa: F401
                             joint_fit, joint_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


def handle(K, max_stars, **opts):
    import torch
    from thepayne_amd.fitting.optfit import LMHandle
    return LMHandle(K, max_stars, torch.device("cuda", 0), **dict(DEFAULTS, **opts))


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def state_of(h):
    """The handle's state as tests/test_lmfit.py's parse_state returns the emulator's."""
    r = {k: v.cpu().numpy() for k, v in h.result().items()}
    return dict(x_best=r["x_best"], x_trial=h.trial().cpu().numpy(), A=r["A"], g=r["g"], chisq=r["chisq"], lam=r["lambda"], status=r["status"].astype(int),
                niter=r["niter"].astype(int), at_bound=r["at_bound"].astype(np.int64))


def tile_of(st, K):
    """[B, 16, 16] from the stored A, g and chi^2 of a first (always accepted) evaluation."""
    G = np.zeros((len(st["chisq"]), 16, 16))
    G[:, :K, :K], G[:, :K, K], G[:, K, :K], G[:, K, K] = st["A"], st["g"], st["g"], st["chisq"]
    return G


def relaid(a, ld, n, fill):
    """The same values in an array of another leading dimension."""
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :n] = a[..., :n]
    return out


def x_on_device(x, offset):
    """x on the device, `offset` doubles behind a 16-byte boundary."""
    buf = dev(np.concatenate([np.zeros(offset), x]))
    return buf[offset:]


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Km,P", SHAPES)
@pytest.mark.parametrize("n", (5, 37, 1000, 3600))
def test_sums_through_the_abi(lib, Km, P, n):
    """The first evaluation is always accepted, so A, g and chi^2 are the tile.  Three stars against the einsum; 70 stars for the
    bytes: a second call, a star alone, the other load path."""
    import torch
    K, B = Km + P, 70
    case = poly_case(np.random.default_rng(10000 * Km + 100 * P + n), B, Km, P, n, n + 3, n + 6)
    x0, lo, hi = start_of(case)
    first = None
    for ld, ld_f, xoff in ((n + 3, n + 6, 1), ((n + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8, 0)):          # element by element; 16 bytes a lane
        rows_d, flux_d, w_d = dev(relaid(case["rows"], ld, n, np.float32(1e30))), dev(relaid(case["flux"], ld_f, n, np.float32(1e30))), dev(relaid(case["w"], ld_f, n, 1e30))
        x_d = x_on_device(case["x"], xoff)
        h = handle(K, B)

        def run(b0=0, nb=B):
            h.begin(x0[b0:b0 + nb], lo, hi)
            assert lib.payne_lmfit_update_poly(h._h, P, rows_d[b0:].data_ptr(), ld, flux_d[b0:].data_ptr(), w_d[b0:].data_ptr(), ld_f, x_d.data_ptr(), n, None) == 0
            torch.cuda.synchronize()
            return state_of(h)
        st = run()
        G = tile_of(st, K)
        check_poly_tiles(G[:3], case, "ABI ld=%d" % ld, stars=range(3))
        assert np.array_equal(st["A"], np.swapaxes(st["A"], 1, 2)) and np.all(st["niter"] == 1)
        assert np.all(np.isfinite(G)) and np.all(G[:, K, K] > 0)                                     # (star 1 holds NaN under w == 0 only)
        again = run()
        assert all(again[k].tobytes() == st[k].tobytes() for k in st)                                # a second call: the same bytes
        for b in (0, 1, B // 2, B - 1):                                                              # a star alone: the same bytes as in the batch
            one = run(b, 1)
            assert all(one[k][0].tobytes() == st[k][b].tobytes() for k in st), (b,)
        if first is None:
            first = st
        else:
            assert all(first[k].tobytes() == st[k].tobytes() for k in st)                            # both load paths: the same bits
        h.close()


# ---- 2. against the emulator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Km,P,n", [(4, 4, 37), (5, 9, 1000), (0, 4, 37)])
def test_state_after_each_step_is_the_emulator_s(lib, poly_emul, Km, P, n):
    """Three updates on fresh random rows each: after every one the device's state is the emulator's -- status, evaluations, lambda and
    at_bound exactly, x_trial (whose last P entries are the next update's coefficients) within STEP_TOL."""
    import torch
    K, B, T = Km + P, 3, 3
    rng = np.random.default_rng(31 * Km + P + n)
    case = poly_case(rng, B, Km, P, n, n + 3, n + 6)
    updates = [case["rows"]] + [poly_case(rng, B, Km, P, n, n + 3, n + 6)["rows"] for _ in range(T - 1)]
    x0, lo, hi = start_of(case)
    begin_e, Gs_e, states_e = poly_emul(x0, lo, hi, case["flux"], case["w"], case["x"], updates, n, P)
    h = handle(K, B)
    h.begin(x0, lo, hi)
    flux_d, w_d, x_d = dev(case["flux"]), dev(case["w"]), dev(case["x"])
    for t, rows in enumerate(updates):
        rows_d = dev(rows)
        assert lib.payne_lmfit_update_poly(h._h, P, rows_d.data_ptr(), n + 3, flux_d.data_ptr(), w_d.data_ptr(), n + 6, x_d.data_ptr(), n, None) == 0
        torch.cuda.synchronize()
        st, se = state_of(h), states_e[t]
        for key in ("status", "niter", "at_bound", "lam"):
            assert np.array_equal(st[key], se[key]), (t, key, st[key], se[key])
        for b in range(B):
            assert np.all(np.isfinite(se["A"][b])) and np.all(np.diag(se["A"][b]) > 0)
            sig = 1.0 / np.sqrt(np.diag(se["A"][b]))
            err = np.abs(st["x_trial"][b] - se["x_trial"][b]) / sig
            errb = np.abs(st["x_best"][b] - se["x_best"][b]) / sig
            print("Km=%d P=%d n=%d update %d star %d: status %d, |x_trial - emulator's| = %.3g sigma at most" % (Km, P, n, t, b, st["status"][b], err.max()))
            assert err.max() <= STEP_TOL and errb.max() <= STEP_TOL, (t, b, err.max(), errb.max())
    assert np.all(states_e[-1]["niter"] >= 1)
    h.close()


# ---- 3. a linear model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", LINEAR)
def test_one_gauss_newton_step_is_continuumfit_s_polynomial(lib, n, P):
    """K_m = 0, lambda0 = lambda_min = 0: one update from an arbitrary c lands on ContinuumFit.fit's coefficients within bound (b)."""
    import torch
    from thepayne_amd.fitting.contfit import ContinuumFit
    case, rows, start = linear_case(n, P)
    N = case["N"]
    flux, w, model = np.ascontiguousarray(case["flux"][:, :n]), np.ascontiguousarray(case["w"][:, :n]), np.ascontiguousarray(case["model"][:, :n])
    h = handle(P, N, lambda0=0.0, lambda_min=0.0, xtol=0.0)
    h.begin(start, np.full(P, -BIG), np.full(P, BIG))
    x_d = dev(case["x"])
    h.update_poly(dev(model[:, None, :]), dev(flux), dev(w), x_d, P)
    torch.cuda.synchronize()
    st = state_of(h)
    h.close()
    assert np.all(st["status"] == RUNNING) and np.all(st["lam"] == 0.0) and np.all(st["at_bound"] == 0)
    wave = 5000.0 + np.cumsum(np.random.default_rng(n).uniform(0.5, 1.5, n))                         # (abscissa_of's grid)
    cf = ContinuumFit(wave, npoly=P)
    assert np.array_equal(cf.x, case["x"])
    ref = cf.run(dev(flux), dev(w), dev(model), normalise=False)
    coef = ref["coef"].cpu().numpy()
    V = chebvander(case["x"], P - 1)
    worst = 0.0
    for s in range(N):
        o = oracle_star(flux[s], w[s], model[s], case["x"], P)
        p_c, p_g = V @ coef[s], V @ st["x_trial"][s]
        bound = max(n, 16) * EPS * o["cond"] * np.abs(V @ o["coef"]).max()
        worst = max(worst, float(np.abs(p_g - p_c).max() / bound))
        assert np.abs(p_g - p_c).max() <= bound, (n, P, s, np.abs(p_g - p_c).max(), bound)
    print("n=%d P=%d: |p - ContinuumFit's| / bound (b) = %.3g" % (n, P, worst))


# ---- 4. OptFit.fit_joint --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nobs,P,fit_vrad", JOINT_CASES)
def test_fit_joint_against_the_joint_reference_loop(g20, nobs, P, fit_vrad):
    import torch
    from thepayne_amd.fitting.optfit import OptFit
    net, nntype, case, coef, flux, x = joint_inputs(g20, nobs)
    refs = joint_reference(g20, nobs, P, fit_vrad)
    S = ALT_STARS
    cols = case["cols"] + ([4] if fit_vrad else [])
    Km = len(cols)
    fit = OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX)
    f32 = flux.astype(np.float32)
    res = fit.fit_joint(f32, case["eflux"][:S], case["start"][:S], npoly=P, fit_vrad=fit_vrad)
    assert res["coef"].shape == (S, P) and res["fisher"].shape == (S, Km + P, Km + P) and res["err"].shape == (S, Km + P) and res["pars"].shape == (S, 8)
    assert res["labels"] == fit.labels(fit_vrad) + ["pc_%d" % j for j in range(P)] and np.all(res["cont_status"] == 0) and np.all(res["npix"] == nobs)
    other = [c for c in range(8) if c not in cols]
    assert np.array_equal(res["pars"][:, other], case["start"][:S][:, other], equal_nan=True)
    for i in range(S):
        r64 = refs[i]
        r32 = joint_fit(g20, i, nobs, P, fit_vrad, dtype=torch.float32)
        z = np.concatenate([res["pars"][i, cols], res["coef"][i]])
        d, d32 = sigma_distance(z, r64["x"], r64["A"]), sigma_distance(r32["x"], r64["x"], r64["A"])
        print("nobs=%d P=%d fit_vrad=%s star %d: status %d after %d evaluations (reference: %d), d = %.3g sigma (bound 1e-2; the fp32-fed loop's %.3g)"
              % (nobs, P, fit_vrad, i, res["status"][i], res["niter"][i], r64["niter"], d, d32))
        assert res["status"][i] == CONVERGED and res["niter"][i] <= RECOVERY_MAX_EVALS, (i, res["status"][i], res["niter"][i])
        assert d <= 1e-2, (i, d, d32)
        assert np.all(np.isfinite(res["err"][i])) and np.all(res["err"][i] >= 1.0 / np.sqrt(np.diag(res["fisher"][i])) * (1.0 - 1e-12))   # marginal >= conditional
    # three stars are two chunks here (b_max 16 holds 2 stars' rows): each star's bytes are those of the star alone
    for i in range(S):
        one = fit.fit_joint(f32[i:i + 1], case["eflux"][i:i + 1], case["start"][i:i + 1], npoly=P, fit_vrad=fit_vrad)
        for key in ("pars", "coef", "chisq", "fisher", "status", "niter", "at_bound", "err"):
            assert np.asarray(one[key][0]).tobytes() == np.asarray(res[key][i]).tobytes(), (i, key)
    if (nobs, P, fit_vrad) == JOINT_CASES[0]:
        # given coefficients: the same fit; a spectrum that is NaN at a counting pixel: status NAN and NaN results, the neighbours as before
        from thepayne_amd.fitting.contfit import ContinuumFit
        c0 = ContinuumFit(case["obs_wave"], npoly=P).fit(f32, case["eflux"][:S], fit.model_spectra(case["start"][:S]), normalise=False)["coef"]
        given = fit.fit_joint(f32, case["eflux"][:S], case["start"][:S], npoly=P, coef=c0)
        assert all(np.asarray(given[k]).tobytes() == np.asarray(res[k]).tobytes() for k in ("pars", "coef", "chisq", "fisher", "status", "niter"))
        bad = f32.copy()
        bad[1, 10] = np.nan
        res2 = fit.fit_joint(bad, case["eflux"][:S], case["start"][:S], npoly=P)
        assert res2["cont_status"][1] == _lib.CONTFIT_NAN and res2["status"][1] == _lib.LMFIT_NAN and np.all(np.isnan(res2["pars"][1, cols]))
        assert np.all(np.isnan(res2["coef"][1])) and np.all(np.isnan(res2["fisher"][1])) and np.all(np.isnan(res2["err"][1])) and np.isnan(res2["chisq"][1])
        assert all(np.asarray(res2[k])[[0, 2]].tobytes() == np.asarray(res[k])[[0, 2]].tobytes() for k in ("pars", "coef", "chisq", "fisher", "status"))
        # clipping: a cosmic ray on star 0 (500 sigma; 10 x the reduced chi of the starting fit, which it dominates, is far below it and
        # far above every other pixel) is dropped by the starting fit's one clip and does not count in the joint fit
        hit = f32.copy()
        hit[0, 500] += 5.0
        res3 = fit.fit_joint(hit, case["eflux"][:S], case["start"][:S], npoly=P, clip=dict(nclip=1, kappa=10.0, rescale=True))
        assert res3["npix"][0] == nobs - 1 and np.all(res3["npix"][1:] == nobs) and np.all(res3["status"] == CONVERGED)
        assert sigma_distance(np.concatenate([res3["pars"][0, cols], res3["coef"][0]]), refs[0]["x"], refs[0]["A"]) <= 1e-2
        with pytest.raises(ValueError):
            fit.fit_joint(f32, case["eflux"][:S], case["start"][:S], npoly=11)                       # 5 + 11 parameters


# ---- 5. arguments ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_state_untouched(lib):
    import torch
    Km, P, B, n = 2, 3, 2, 8
    K = Km + P
    inv = _lib.E_INVALID
    h = handle(K, 4)
    x0, lo, hi = dev(np.ones((B, K))), np.full(K, -10.0), np.full(K, 10.0)
    rows, flux, w, x = dev(np.ones((B, 1 + Km, n), dtype=np.float32)), dev(np.ones((B, n), dtype=np.float32)), dev(np.ones((B, n))), dev(np.linspace(-1, 1, n))

    def update(h_=h._h, P=P, rows=rows, ld=n, flux=flux, w=w, ld_f=n, x=x, n=n):
        return lib.payne_lmfit_update_poly(h_, P, None if rows is None else rows.data_ptr(), ld, None if flux is None else flux.data_ptr(),
                                           None if w is None else w.data_ptr(), ld_f, None if x is None else x.data_ptr(), n, None)
    h.begin(x0, lo, hi)
    torch.cuda.synchronize()
    before = state_of(h)
    assert update(h_=None) == inv                                                            # null handle
    assert update(n=0) == inv and update(ld=n - 1) == inv and update(ld_f=n - 1) == inv      # n < 1, ld < n, ld_f < n
    assert update(P=0) == inv and update(P=-1) == inv and update(P=K + 1) == inv             # P < 1, P > K
    assert update(rows=None) == inv and update(flux=None) == inv and update(w=None) == inv   # null pointers with B > 0
    assert update(x=None) == inv                                                             # null x_dev with B > 0
    torch.cuda.synchronize()
    after = state_of(h)
    assert all(np.array_equal(after[k], before[k]) for k in before) and np.all(after["niter"] == 0)   # none of the refused calls ran
    with pytest.raises(ValueError):
        h.update_poly(rows, flux, w, x, K + 1)
    with pytest.raises(ValueError):
        h.update_poly(rows, flux, w, x[:-1], P)
    with pytest.raises(ValueError):
        h.update_poly(rows[:, :2], flux, w, x, P)
    # B == 0 succeeds and does nothing; P == K (no model parameter) is allowed
    assert lib.payne_lmfit_begin(h._h, None, lo.ctypes.data, hi.ctypes.data, 0, None) == 0 and update(rows=None, flux=None, w=None, x=None) == 0
    h.begin(x0, lo, hi)
    assert update(P=K, rows=dev(np.ones((B, 1, n), dtype=np.float32))) == 0
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 1)
    h.close()
