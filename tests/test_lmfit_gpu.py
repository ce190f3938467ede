"""Batched Levenberg-Marquardt on the device: payne_lmfit_* through the C ABI and thepayne_amd/fitting/optfit.py end to end.  The
references, the scripted inputs and the bounds are tests/test_lmfit.py's, which checks on the CPU that the fp64 reference loop
converges on the inputs recovered here.

Yardstick of the noisy fits: the distance d = max_k |x - x*| sqrt(F*_kk) of the device's solution from the fp64 reference loop's
x* stays within max(10 xtol, 4 x the distance of the same numpy loop fed with torch's CPU fp32 model and Jacobian, started at x*)."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import (DEFAULTS, RUNNING, CONVERGED, STALLED, MAXITER, STEP_TOL, SUM_K, RECOVERY_BMAX, RECOVERY_N, SNR, sums_case, check_tiles,
                        scripts, check_script, emul, g20, recovery_inputs, reference_fit, sigma_distance)                      # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
XTOL = DEFAULTS["xtol"]


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


def update_raw(lib, h, rows_d, ld, flux_d, w_d, ld_f, n):
    assert lib.payne_lmfit_update(h._h, rows_d.data_ptr(), ld, flux_d.data_ptr(), w_d.data_ptr(), ld_f, n, None) == 0


def tile_of(st, K):
    """[B, 16, 16] from the stored A, g and chi^2 of a first (always accepted) evaluation."""
    B = len(st["chisq"])
    G = np.zeros((B, 16, 16))
    G[:, :K, :K], G[:, :K, K], G[:, K, :K], G[:, K, K] = st["A"], st["g"], st["g"], st["chisq"]
    return G


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SUM_K)
@pytest.mark.parametrize("n", (5, 37, 1000, 3600))
def test_sums_through_the_abi(lib, K, n):
    import torch
    for B in (1, 3, 70):
        rng = np.random.default_rng(1000 * B + 100 * K + n)
        big = 1e6
        x0, lo, hi = np.zeros((B, K)), np.full(K, -big), np.full(K, big)
        first = None
        for ld, ld_f in ((n + 3, n + 6), ((n + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8)):      # element by element; 16 bytes a lane
            rng2 = np.random.default_rng(1000 * B + 100 * K + n)
            rows, flux, w = sums_case(rng2, B, K, n, ld, ld_f)
            rows_d, flux_d, w_d = dev(rows), dev(flux), dev(w)
            h = handle(K, B + 2)

            def run(b0=0, nb=B):
                h.begin(x0[b0:b0 + nb], lo, hi)
                update_raw(lib, h, rows_d[b0:], ld, flux_d[b0:], w_d[b0:], ld_f, n)
                torch.cuda.synchronize()
                return state_of(h)
            st = run()
            G = tile_of(st, K)
            check_tiles(G, rows, flux, w, n, K, "ABI B=%d ld=%d" % (B, ld))
            assert np.array_equal(st["A"], np.swapaxes(st["A"], 1, 2)) and np.all(st["niter"] == 1)
            again = run()
            assert all(again[k].tobytes() == st[k].tobytes() for k in st)                    # a second call: the same bytes
            for b in sorted({0, B // 2, B - 1}):                                             # a star alone: the same bytes as in the batch
                one = run(b, 1)
                assert all(one[k][0].tobytes() == st[k][b].tobytes() for k in st), (B, b)
            if first is None:
                first = G
            else:
                assert G.tobytes() == first.tobytes()                                        # both load paths: the same bits
            h.close()


# ---- 2. against the emulator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", scripts(), ids=lambda s: s.name.replace(" ", "_"))
def test_state_machine_against_the_emulator(lib, emul, sc):
    import torch
    begin_e, Gs_e, states_e = sc.run(emul)
    h = handle(sc.K, 4, **sc.opts)
    h.begin(sc.x0, sc.lo, sc.hi)
    torch.cuda.synchronize()
    begin = state_of(h)
    flux_d, w_d = dev(sc.flux), dev(sc.w)
    states = []
    for rows in sc.rows:
        update_raw(lib, h, dev(rows), sc.ld, flux_d, w_d, sc.ld_f, sc.n)
        torch.cuda.synchronize()
        states.append(state_of(h))
    h.close()
    check_script(sc, begin, states, "device")
    for t, (st, se) in enumerate(zip([begin] + states, [begin_e] + states_e)):
        for key in ("status", "niter", "at_bound", "lam"):
            assert np.array_equal(st[key], se[key]), (sc.name, t, key, st[key], se[key])
        if t > 0 and np.all(np.isfinite(se["A"])) and np.all(np.diag(se["A"][0]) > 0):
            sig = 1.0 / np.sqrt(np.diag(se["A"][0]))
            err = np.abs(st["x_trial"][0] - se["x_trial"][0]) / sig
            print("%s update %d: |x_trial - emulator's| = %.3g sigma at most" % (sc.name, t - 1, err.max()))
            assert err.max() <= STEP_TOL, (sc.name, t, err.max())
        else:
            assert np.array_equal(st["x_trial"], se["x_trial"], equal_nan=True)


# ---- 3. arguments ---------------------------------------------------------------------------------------------------------------
def test_invalid_and_unsupported_arguments(lib):
    import torch
    K, B, n = 3, 2, 8
    out = C.c_void_p()
    inv, uns = _lib.E_INVALID, _lib.E_UNSUPPORTED

    def create(K=K, max_stars=4, opts=None, out=out, **kw):
        o = _lib.LmfitOpts(**kw) if opts is None else opts
        rc = lib.payne_lmfit_create(0, K, max_stars, C.byref(o) if o is not False else None, C.byref(out) if out is not None else None)
        if rc == 0:
            lib.payne_lmfit_destroy(out)
        return rc
    assert create() == 0 and create(opts=False) == 0 and create(K=15) == 0 and create(lambda0=0.0, lambda_min=0.0) == 0
    assert create(out=None) == inv                                       # null out
    assert create(K=0) == inv                                            # K < 1
    assert create(max_stars=0) == inv                                    # max_stars < 1
    assert create(xtol=float("nan")) == inv and create(lambda_max=float("inf")) == inv     # an option that is not finite
    assert create(lambda0=-1.0, lambda_min=-1.0) == inv                  # lambda0 < 0, lambda_min < 0
    assert create(lambda_min=1.0, lambda_max=0.5, lambda0=1.0) == inv    # lambda_max < lambda_min
    assert create(lambda0=1e9) == inv and create(lambda0=1e-13) == inv   # lambda0 outside [lambda_min, lambda_max]
    assert create(down=0.5) == inv and create(up=0.5) == inv             # down < 1, up < 1
    assert create(xtol=-1.0) == inv and create(maxiter=0) == inv         # xtol < 0, maxiter < 1
    assert create(K=16) == uns                                           # K > 15

    h = handle(K, 4)
    x0, lo, hi = dev(np.zeros((B, K))), np.full(K, -1.0), np.full(K, 1.0)

    def begin(h_=h._h, x0=x0, lo=lo, hi=hi, B=B):
        return lib.payne_lmfit_begin(h_, None if x0 is None else x0.data_ptr(), None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data, B, None)
    assert begin() == 0
    assert begin(h_=None) == inv and begin(lo=None) == inv and begin(hi=None) == inv      # null handle / lo / hi
    assert begin(B=-1) == inv and begin(B=5) == inv                                          # B outside 0 .. max_stars
    assert begin(x0=None) == inv                                                             # null x0_dev with B > 0
    assert begin(lo=hi) == inv and begin(lo=np.array([-1.0, 2.0, -1.0])) == inv              # lo >= hi
    assert begin(hi=np.array([1.0, np.inf, 1.0])) == inv and begin(lo=np.array([np.nan, -1.0, -1.0])) == inv   # not finite
    assert lib.payne_lmfit_trial(None) is None and lib.payne_lmfit_trial(h._h) is not None
    rows, flux, w = dev(np.zeros((B, 1 + K, n), dtype=np.float32)), dev(np.zeros((B, n), dtype=np.float32)), dev(np.ones((B, n)))

    def update(h_=h._h, rows=rows, ld=n, flux=flux, w=w, ld_f=n, n=n):
        return lib.payne_lmfit_update(h_, None if rows is None else rows.data_ptr(), ld, None if flux is None else flux.data_ptr(),
                                      None if w is None else w.data_ptr(), ld_f, n, None)
    assert begin() == 0
    assert update(h_=None) == inv                                                            # null handle
    assert update(n=0) == inv and update(ld=n - 1) == inv and update(ld_f=n - 1) == inv      # n < 1, ld < n, ld_f < n
    assert update(rows=None) == inv and update(flux=None) == inv and update(w=None) == inv   # null pointers with B > 0
    assert lib.payne_lmfit_result(None, *([None] * 9)) == inv                                # null handle
    assert lib.payne_lmfit_result(h._h, *([None] * 9)) == 0                                  # every pointer may be NULL
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 0)                                                 # none of the refused calls ran
    # B == 0 succeeds and does nothing
    assert begin(B=0, x0=None) == 0 and update(rows=None, flux=None, w=None) == 0 and lib.payne_lmfit_result(h._h, *([None] * 9)) == 0
    lib.payne_lmfit_destroy(None)
    h.close()


# ---- 4. OptFit ------------------------------------------------------------------------------------------------------------------
def make_fit(net, nntype, case):
    from thepayne_amd.fitting.optfit import OptFit
    return OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX)


def device_spectra(fit, pars):
    """The model OptFit minimises at `pars` [N, 8]: payne_specjac_eval's y through payne_smooth_batch (fp32 [N, nobs])."""
    P = fit.predictor
    eng = P.anns.engine
    P._bind(fit.obs_wave)
    from thepayne_amd.fitting.optfit import fitted_columns
    y, _ = P._jacobian().eval(pars[:, fitted_columns(fit.n_labels, False)])
    th = np.full((len(pars), eng.ncols), np.nan)
    th[:, :8] = pars
    return eng.smooth_batch(y, th, stage=2).cpu().numpy()


@pytest.mark.parametrize("nobs", (37, 1000))
@pytest.mark.parametrize("which", ("smlp", "linnet", "synth5"))
def test_noiseless_recovery(g20, which, nobs):
    for fit_vrad in (False, True):
        net, nntype, case, ref = recovery_inputs(g20, which, nobs, fit_vrad)
        fit = make_fit(net, nntype, case)
        cols = case["cols"] + ([4] if fit_vrad else [])
        flux = device_spectra(fit, case["truth"])
        assert np.all(np.isfinite(flux))
        whole = None
        for N in (RECOVERY_N, 3, 1):
            res = fit.fit(flux[:N], case["eflux"][:N], case["start"][:N], fit_vrad=fit_vrad)
            d = [sigma_distance(res["pars"][i, cols], case["truth"][i, cols], res["fisher"][i]) for i in range(N)]
            print("%s nobs=%d fit_vrad=%s N=%d: evaluations %s, worst distance from the truth %.3g sigma (bound %.3g)"
                  % (which, nobs, fit_vrad, N, list(res["niter"]), max(d), 10.0 * XTOL))
            assert np.all(res["status"] == CONVERGED) and np.all(res["niter"] <= DEFAULTS["maxiter"]), (which, nobs, fit_vrad, N, res["status"], res["niter"])
            assert max(d) <= 10.0 * XTOL, (which, nobs, fit_vrad, N, d)
            assert res["labels"] == fit.labels(fit_vrad) and np.all(res["npix"] == nobs) and res["pars"].shape == (N, 8)
            other = [c for c in range(8) if c not in cols]
            assert np.array_equal(res["pars"][:, other], case["start"][:N][:, other], equal_nan=True)
            if whole is None:
                whole = res
            else:                                                       # a star's result does not depend on the block it was in
                for key in ("pars", "chisq", "fisher", "status", "niter", "at_bound", "err"):
                    assert np.asarray(res[key]).tobytes() == np.asarray(whole[key][:N]).tobytes(), (which, nobs, fit_vrad, N, key)


@pytest.mark.parametrize("which,nobs", [("smlp", 1000), ("synth5", 1000)])
def test_noisy_spectra_against_the_reference_loop(g20, which, nobs):
    """Seeded noise at S/N 100 on the recovery stars.  Compared are the stars on which the fp64 reference loop ends CONVERGED inside
    the box within 25 evaluations (at least three of them, at most six): where noise moves the optimum onto a bound, or the loop runs
    into maxiter, the end point depends on the path and is no yardstick.  Measured on an MI355X: see NOTES.md."""
    import torch
    net, nntype, case, _ = recovery_inputs(g20, which, nobs, False)
    fit = make_fit(net, nntype, case)
    cols = case["cols"]
    N = RECOVERY_N
    rng = np.random.default_rng(77)
    flux = (device_spectra(fit, case["truth"]).astype(np.float64) + rng.normal(0, 1.0 / SNR, (N, nobs))).astype(np.float32)
    res = fit.fit(flux, case["eflux"], case["start"])
    compared = 0
    for i in range(N):
        r64, _ = reference_fit(net, nntype, case, flux[i].astype(np.float64), i)
        if r64["status"] != CONVERGED or r64["at_bound"] != 0 or r64["niter"] > 25:
            continue
        compared += 1
        r32, _ = reference_fit(net, nntype, case, flux[i].astype(np.float64), i, start=r64["x"], dtype=torch.float32)
        d = sigma_distance(res["pars"][i, cols], r64["x"], r64["A"])
        d32 = sigma_distance(r32["x"], r64["x"], r64["A"])
        print("%s nobs=%d star %d: d = %.3g sigma, the fp32-fed loop's %.3g (bound %.3g); status %d after %d evaluations (reference: %d)"
              % (which, nobs, i, d, d32, max(10.0 * XTOL, 4.0 * d32), res["status"][i], res["niter"][i], r64["niter"]))
        assert d <= max(10.0 * XTOL, 4.0 * d32), (which, nobs, i, d, d32)
        if compared == 6:
            break
    assert compared >= 3, compared


def test_truth_outside_the_box(g20):
    """[Fe/H]'s upper bound below the truth: the fit ends on the bound with the bit set, as the reference loop does."""
    net, nntype, case, _ = recovery_inputs(g20, "synth5", 1000, False)
    fit = make_fit(net, nntype, case)
    N = 3
    flux = device_spectra(fit, case["truth"][:N])
    span = net["xmax"][2] - net["xmin"][2]
    for i in range(N):
        edge = case["truth"][i, 2] - 0.05 * span
        start = case["start"][i:i + 1].copy()
        start[0, 2] = edge - 0.05 * span
        res = fit.fit(flux[i:i + 1], case["eflux"][i:i + 1], start, bounds={"[Fe/H]": (net["xmin"][2], edge)})
        import test_lmfit as T
        model = T.OracleModel(net, nntype, case["obs_wave"], start[0])
        lo, hi = net["xmin"].copy(), net["xmax"].copy()
        hi[2] = edge
        ref = T.lm_reference(model, start[0, case["cols"]], lo, hi, flux[i].astype(np.float64), 1.0 / case["eflux"][i] ** 2)
        print("star %d: status %d after %d evaluations (reference %d after %d); at_bound %s (reference %s); distance %.3g sigma"
              % (i, res["status"][0], res["niter"][0], ref["status"], ref["niter"], bin(res["at_bound"][0]), bin(ref["at_bound"]),
                 sigma_distance(res["pars"][0, case["cols"]], ref["x"], ref["A"])))
        assert ref["x"][2] == edge and ref["at_bound"] & 0b100
        assert res["pars"][0, 2] == edge and res["at_bound"][0] & 0b100 and res["status"][0] != RUNNING


def test_error_bars_are_the_forecast_s(g20):
    from thepayne_amd.fitting.forecast import Forecast, crlb_from_fisher
    net, nntype, case, _ = recovery_inputs(g20, "synth5", 1000, False)
    fit = make_fit(net, nntype, case)
    N, nobs = 5, 1000
    eflux = case["eflux"][:N].copy()
    eflux[:, [3, 500]] = [0.0, np.inf]
    res = fit.fit(device_spectra(fit, case["truth"][:N]), eflux, case["start"][:N])
    assert np.all(res["npix"] == nobs - 2) and np.all(res["status"] == CONVERGED)
    fc = Forecast(net, nntype, case["obs_wave"], eflux[0], b_max=RECOVERY_BMAX)
    F = fc.fisher(res["pars"]).cpu().numpy()
    a = np.nan_to_num(fc.jacobian(res["pars"]).cpu().numpy().astype(np.float64), nan=0.0)
    bound = nobs * 2.0 ** -52 * np.einsum("bip,bjp,p->bij", np.abs(a), np.abs(a), fc.weights)
    ratio = float((np.abs(res["fisher"] - F) / np.maximum(bound, 1e-300)).max())
    print("fisher against Forecast.fisher: max |dF| / bound = %.3g" % ratio)
    assert np.all(np.abs(res["fisher"] - F) <= bound), ratio
    assert np.array_equal(res["err"], crlb_from_fisher(res["fisher"])) and np.all(np.isfinite(res["err"])) and res["err"].shape == (N, 5)
