"""Spectrum and photometry in one Levenberg-Marquardt fit on the device: payne_lmfit_update_phot through the C ABI and
OptFit.fit_specphot end to end.  The inputs, the references and the bounds are tests/test_lmfit_phot.py's, which checks on the CPU that
the fp64 joint reference loop converges on the inputs fitted here.

Yardstick of fit_specphot: d = max_k |x - x*| sqrt(A*_kk) over all K parameters, x* and A* the fp64 joint reference loop's, stays within
1e-2 (10 xtol, the project's bound for device fits)."""
import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import DEFAULTS, CONVERGED, STALLED, STEP_TOL, RECOVERY_BMAX, g20, sigma_distance                                          # noqa: F401
from test_lmfit_poly_gpu import lib, handle, dev, state_of, tile_of, relaid, x_on_device                                          # noqa: F401
from test_lmfit_phot import SHAPES, SP_CASES, REAL_CASES, MAX_EVALS, KEEP, phot_case, check_phot_tiles, phot_emul, specphot_inputs           # noqa: F401
import test_sedfit as TS

pytestmark = pytest.mark.gpu


def ptr(t):
    return None if t is None else t.data_ptr()


def update_phot(lib, hd, case, rows_d, flux_d, w_d, x_d, ld, ld_f, ph, b0=0, **over):
    """payne_lmfit_update_phot on the stars from b0 on; ph: dict of device tensors mags, dmags, obs, pw, mu, sigma (or None)."""
    a = dict(h=hd._h, Km=case["Km"], Kp=case["Kp"], P=case["P"], rows=rows_d[b0:], ld=ld, flux=flux_d[b0:], w=w_d[b0:], ld_f=ld_f, x=x_d, n=case["n"], F=case["F"],
             ncol=case["ncol"], sed_col=np.ascontiguousarray(case["sed_col"], dtype=np.int32), mags=ph["mags"][b0:], dmags=ph["dmags"][b0:], obs=ph["obs"][b0:],
             pw=ph["pw"][b0:], mu=None if ph["mu"] is None else ph["mu"][b0:], sigma=None if ph["sigma"] is None else ph["sigma"][b0:])
    a.update(over)
    sc = a["sed_col"]
    return lib.payne_lmfit_update_phot(a["h"], a["Km"], a["Kp"], a["P"], ptr(a["rows"]), a["ld"], ptr(a["flux"]), ptr(a["w"]), a["ld_f"], ptr(a["x"]), a["n"], a["F"], a["ncol"],
                                       None if sc is None else sc.ctypes.data, ptr(a["mags"]), ptr(a["dmags"]), ptr(a["obs"]), ptr(a["pw"]), ptr(a["mu"]), ptr(a["sigma"]), None)


def phot_on_device(case, mags=None, dmags=None):
    return dict(mags=dev(case["mags"] if mags is None else mags), dmags=dev(case["dmags"] if dmags is None else dmags), obs=dev(case["obs"]), pw=dev(case["pw"]),
                mu=None if case["mu"] is None else dev(case["mu"]), sigma=None if case["sigma"] is None else dev(case["sigma"]))


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Km,Kp,P", SHAPES)
@pytest.mark.parametrize("n", (5, 37, 1000))
def test_sums_through_the_abi(lib, Km, Kp, P, n):
    """The first evaluation is always accepted, so A, g and chi^2 are the tile.  Three stars against the long-double reference; 70
    stars for the bytes: a second call, a star alone, the other load path.  F = 7 carries priors."""
    import torch
    B = 70
    for F in (1, 7, 64):
        case = phot_case(np.random.default_rng(100000 * Km + 10000 * Kp + 1000 * P + 10 * n + F), B, Km, Kp, P, n, F, n + 3, n + 6, prior=F == 7)
        K = case["K"]
        ph = phot_on_device(case)
        first = None
        for ld, ld_f, xoff in ((n + 3, n + 6, 1), ((n + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8, 0)):      # element by element; 16 bytes a lane
            rows_d, flux_d, w_d = dev(relaid(case["rows"], ld, n, np.float32(1e30))), dev(relaid(case["flux"], ld_f, n, np.float32(1e30))), dev(relaid(case["w"], ld_f, n, 1e30))
            x_d = x_on_device(case["x"], xoff)
            h = handle(K, B)

            def run(b0=0, nb=B):
                h.begin(case["x0"][b0:b0 + nb], case["lo"], case["hi"])
                assert update_phot(lib, h, case, rows_d, flux_d, w_d, x_d, ld, ld_f, ph, b0=b0) == 0
                torch.cuda.synchronize()
                return state_of(h)
            st = run()
            G = tile_of(st, K)
            check_phot_tiles(G[:3], case, "ABI ld=%d" % ld, stars=range(3))
            assert np.array_equal(st["A"], np.swapaxes(st["A"], 1, 2)) and np.all(st["niter"] == 1)
            assert np.all(np.isfinite(G)) and np.all(G[:, K, K] > 0)                                 # (NaN sits under w == 0 and pw == 0 only)
            again = run()
            assert all(again[k].tobytes() == st[k].tobytes() for k in st)                            # a second call: the same bytes
            for b in (0, 1, B // 2, B - 1):                                                          # a star alone: the same bytes as in the batch
                one = run(b, 1)
                assert all(one[k][0].tobytes() == st[k][b].tobytes() for k in st), (b,)
            if first is None:
                first = st
            else:
                assert all(first[k].tobytes() == st[k].tobytes() for k in st)                        # both load paths: the same bits
            h.close()


# ---- 2. against the emulator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Km,Kp,P,n,F", [(4, 2, 4, 37, 7), (6, 3, 6, 1000, 33)])
def test_state_after_each_step_is_the_emulator_s(lib, phot_emul, Km, Kp, P, n, F):
    """Three updates on fresh random rows and magnitudes each, priors included: after every one the device's state is the emulator's --
    status, evaluations, lambda and at_bound exactly, x_trial (which the next update's coefficients and priors are read from) within
    STEP_TOL."""
    import torch
    B, T = 3, 3
    rng = np.random.default_rng(31 * Km + 7 * Kp + P + n + F)
    case = phot_case(rng, B, Km, Kp, P, n, F, n + 3, n + 6, prior=True)
    K = case["K"]
    more = [phot_case(rng, B, Km, Kp, P, n, F, n + 3, n + 6) for _ in range(T - 1)]
    keep = case["pw"] != 0.0                                          # (the later updates' NaN pattern is their own: keep numbers wherever this pw counts)
    updates = [(case["rows"], case["mags"], case["dmags"])] + [(c["rows"], np.where(keep, np.nan_to_num(c["mags"], nan=15.0), np.nan),
                                                                np.where(keep[:, :, None], np.nan_to_num(c["dmags"], nan=0.5), np.nan)) for c in more]
    begin_e, Gs_e, states_e = phot_emul(case, updates)
    h = handle(K, B)
    h.begin(case["x0"], case["lo"], case["hi"])
    flux_d, w_d, x_d = dev(case["flux"]), dev(case["w"]), dev(case["x"])
    for t, (rows, mags, dmags) in enumerate(updates):
        rows_d, ph = dev(rows), phot_on_device(case, mags, dmags)
        assert update_phot(lib, h, case, rows_d, flux_d, w_d, x_d, n + 3, n + 6, ph) == 0
        torch.cuda.synchronize()
        st, se = state_of(h), states_e[t]
        for key in ("status", "niter", "at_bound", "lam"):
            assert np.array_equal(st[key], se[key]), (t, key, st[key], se[key])
        for b in range(B):
            assert np.all(np.isfinite(se["A"][b])) and np.all(np.diag(se["A"][b]) > 0)
            sig = 1.0 / np.sqrt(np.diag(se["A"][b]))
            err = np.abs(st["x_trial"][b] - se["x_trial"][b]) / sig
            errb = np.abs(st["x_best"][b] - se["x_best"][b]) / sig
            print("Km=%d Kp=%d P=%d n=%d F=%d update %d star %d: status %d, |x_trial - emulator's| = %.3g sigma at most" % (Km, Kp, P, n, F, t, b, st["status"][b], err.max()))
            assert err.max() <= STEP_TOL and errb.max() <= STEP_TOL, (t, b, err.max(), errb.max())
    assert np.all(states_e[-1]["niter"] >= 1)
    h.close()


# ---- 3. OptFit.fit_specphot -----------------------------------------------------------------------------------------------------
_FITS = {}


def fitters(inp, name):
    from thepayne_amd.fitting import SEDFit
    from thepayne_amd.fitting.optfit import OptFit
    if name not in _FITS:
        _FITS[name] = (OptFit(inp["net"], inp["nntype"], inp["obs_wave"], b_max=RECOVERY_BMAX),
                       SEDFit(usebands=inp["phot"]["filters"], nnpath=inp["phot"], photscale=inp["cfg"]["photscale"]))
    return _FITS[name]


def run_specphot(inp, name):
    fit, sed = fitters(inp, name)
    cfg = inp["cfg"]
    return fit.fit_specphot(inp["flux"], inp["eflux"], inp["mags"], inp["emags"], inp["start"], inp["phot_start"], sed, free_phot=cfg["free"], npoly=cfg["P"],
                            fit_vrad=cfg["fit_vrad"], bounds=inp["bounds"], prior=inp["prior"])


@pytest.mark.parametrize("name", sorted(SP_CASES))
def test_fit_specphot_against_the_joint_reference_loop(g20, name):
    inp = specphot_inputs(g20, name)
    fit, sed = fitters(inp, name)
    res = run_specphot(inp, name)
    Km, Kp, P, K, cols, pcols = inp["Km"], inp["Kp"], inp["P"], inp["K"], inp["cols"], inp["pcols"]
    ncol = 6 if inp["cfg"]["photscale"] else 7
    assert res["fisher"].shape == (KEEP, K, K) and res["err"].shape == (KEEP, K) and res["pars"].shape == (KEEP, 8) and res["coef"].shape == (KEEP, P)
    assert res["phot_pars"].shape == (KEEP, ncol) and res["mags_model"].shape == inp["mags"].shape and np.all(res["nfilt"] == inp["mags"].shape[1]) and np.all(res["npix"] == len(inp["obs_wave"]))
    assert res["labels"] == fit.labels(inp["cfg"]["fit_vrad"]) + [TS.NAMES[inp["cfg"]["photscale"]][c] for c in pcols] + ["pc_%d" % j for j in range(P)]
    other = [c for c in range(8) if c not in cols]
    assert np.array_equal(res["pars"][:, other], inp["start"][:, other], equal_nan=True) and np.all(res["cont_status"] == 0)
    fixed = [c for c in range(4, ncol) if c not in pcols]
    assert np.array_equal(res["phot_pars"][:, fixed], inp["phot_start"][:, [c - 4 for c in fixed]]) and np.array_equal(res["phot_pars"][:, :4], res["pars"][:, :4])
    m_at, _ = sed.grad(res["phot_pars"])
    assert np.array_equal(res["mags_model"], m_at)                                                   # the model magnitudes are sed.grad's at the solution
    worst = 0.0
    for i, ref in enumerate(inp["refs"]):
        z = np.concatenate([res["pars"][i, cols], res["phot_pars"][i, pcols], res["coef"][i]])
        d = sigma_distance(z, ref["x"], ref["A"])
        worst = max(worst, d)
        print("case %s star %d: status %d after %d evaluations (reference: %d), chi^2 %.6g (reference %.6g), d = %.3g sigma (bound 1e-2)"
              % (name, i, res["status"][i], res["niter"][i], ref["niter"], res["chisq"][i], ref["chisq"], d))
        F = res["fisher"][i]
        s = 1.0 / np.sqrt(np.diag(F))
        want = np.sqrt(np.diag(np.linalg.inv(F * np.outer(s, s)))) * s                               # sqrt(diag(inv(F))), through the unit-diagonal scaling
        assert np.all(np.isfinite(res["err"][i])) and np.allclose(res["err"][i], want, rtol=1e-9, atol=0.0), (name, i)
        assert np.all(res["err"][i] >= s * (1.0 - 1e-12))                                            # marginal >= conditional
    print("case %s: the largest distance %.3g sigma" % (name, worst))
    for i in range(KEEP):
        assert res["status"][i] == CONVERGED, (name, i, res["status"][i], res["niter"][i])
    assert worst <= 1e-2, (name, worst)


@pytest.mark.parametrize("name", REAL_CASES)
def test_fit_specphot_with_noise_at_the_error_bar(g20, name):
    """What a user's data look like: the magnitudes scatter by their 0.02 mag errors.  The shared labels are then pulled off the
    spectrum's own minimum, the fp32 spectral model's rounding reaches chi^2 at 2e-6 .. 5e-6 (tests/test_lmfit_phot.py: MAG_NOISE), more
    than the last decisive step gains, and update_star's acceptance rule may reject trial after trial at the solution: a star ends
    CONVERGED after more evaluations than the reference, or STALLED.  Either way it lies within the bound, 1e-2 sigma of the fp64 loop."""
    inp = specphot_inputs(g20, name, TS.SIGMA_MAG)
    res = run_specphot(inp, name)
    worst = 0.0
    for i, ref in enumerate(inp["refs"]):
        z = np.concatenate([res["pars"][i, inp["cols"]], res["phot_pars"][i, inp["pcols"]], res["coef"][i]])
        d = sigma_distance(z, ref["x"], ref["A"])
        worst = max(worst, d)
        print("case %s, 0.02 mag of noise, star %d: status %d after %d evaluations (reference: %d), chi^2 %.7g (reference %.7g), d = %.3g sigma (bound 1e-2)"
              % (name, i, res["status"][i], res["niter"][i], ref["niter"], res["chisq"][i], ref["chisq"], d))
    for i in range(KEEP):
        assert res["status"][i] in (CONVERGED, STALLED), (name, i, res["status"][i], res["niter"][i])
        assert np.all(np.isfinite(res["err"][i]))
    assert worst <= 1e-2, (name, worst)


def test_the_magnitudes_tighten_the_spectrum_and_the_spectrum_the_magnitudes(g20):
    """The feature's point, on case a, in the two forms that the addition of Fisher matrices implies, both on the public results.
    Teff: its marginal error from spectrum and magnitudes together is below fit_joint's on the spectrum alone -- the same ten
    parameters with and without the magnitudes' block.  Av: its marginal ``err`` from fit_specphot (over all ten parameters) is below
    the marginal error from the magnitudes alone with all six parameters they see free (Teff, log g, [Fe/H], [a/Fe], logR, Av), taken
    at the joint solution through ``sed.grad``: marginalising the joint matrix over the polynomial leaves the magnitudes' 6 x 6 matrix
    plus a Schur complement of the spectrum's, which is positive semi-definite.  The form with SEDFit.fit's (Teff, logR, Av) free does not
    follow and does not hold: that fit keeps log g, [Fe/H], [a/Fe] fixed, so its error is conditional on them, and a conditional and a
    marginal error are not ordered (NOTES.md has the figures).  SEDFit.fit's own figures, three and six parameters free, are printed."""
    inp = specphot_inputs(g20, "a")
    fit, sed = fitters(inp, "a")
    res = run_specphot(inp, "a")
    spec = fit.fit_joint(inp["flux"], inp["eflux"], inp["start"], npoly=inp["P"])
    prow = np.concatenate([inp["start"][:, :4], inp["phot_start"]], axis=1)
    three = sed.fit(inp["mags"], inp["emags"], prow, free=("Teff", "logR", "Av"), bounds=inp["bounds"])
    six = sed.fit(inp["mags"], inp["emags"], res["phot_pars"], free=("Teff", "logg", "FeH", "aFe", "logR", "Av"), bounds=inp["bounds"])
    k_av = res["labels"].index("Av")
    _, J = sed.grad(res["phot_pars"])
    J = J[:, :, [0, 1, 2, 3, 4, 6]]
    for i in range(KEEP):
        A = np.einsum("fi,fj,f->ij", J[i], J[i], 1.0 / inp["emags"][i] ** 2)
        s = 1.0 / np.sqrt(np.diag(A))
        alone = np.sqrt(np.diag(np.linalg.inv(A * np.outer(s, s)))) * s
        print("star %d: sigma(Teff) %.4g K together, %.4g K from the spectrum alone; sigma(Av) %.5g together, %.5g from the magnitudes alone with six parameters free at the "
              "same point (SEDFit.fit: %.5g with six free, status %d; %.5g with three)" % (i, res["err"][i, 0], spec["err"][i, 0], res["err"][i, k_av], alone[5], six["err"][i, 5],
                                                                                         six["status"][i], three["err"][i, 2]))
        assert res["err"][i, 0] < spec["err"][i, 0] and res["err"][i, k_av] < alone[5], i


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_state_untouched(lib):
    import torch
    B, n = 2, 8
    case = phot_case(np.random.default_rng(1), B, 2, 2, 3, n, 5, n, n, prior=True)
    K, inv = case["K"], _lib.E_INVALID
    h = handle(K, 4)
    rows, flux, w, x, ph = dev(case["rows"]), dev(case["flux"]), dev(case["w"]), dev(case["x"]), phot_on_device(case)

    def update(**over):
        return update_phot(lib, h, case, rows, flux, w, x, over.pop("ld", n), over.pop("ld_f", n), ph, **over)
    h.begin(case["x0"], case["lo"], case["hi"])
    torch.cuda.synchronize()
    before = state_of(h)
    sc = case["sed_col"]                                              # [0, 1, 5, 6, -1, -1, -1]

    def with_col(k, v):
        out = sc.copy()
        out[k] = v
        return out
    assert update(h=None) == inv                                                             # null handle
    assert update(n=0) == inv and update(ld=n - 1) == inv and update(ld_f=n - 1) == inv      # n < 1, ld < n, ld_f < n
    assert update(P=-1, Km=6) == inv and update(Kp=-1, Km=5) == inv and update(Km=3) == inv and update(P=2) == inv   # P < 0, Kp < 0, Km + Kp + P != K
    assert update(F=-1) == inv and update(ncol=5) == inv and update(ncol=8) == inv
    assert update(mags=None) == inv and update(dmags=None) == inv and update(obs=None) == inv and update(pw=None) == inv   # null photometric arrays with F > 0
    assert update(rows=None) == inv and update(flux=None) == inv and update(w=None) == inv and update(x=None) == inv
    assert update(sed_col=None) == inv and update(sed_col=with_col(0, -2)) == inv and update(sed_col=with_col(0, 7)) == inv
    assert update(sed_col=with_col(2, -1)) == inv and update(sed_col=with_col(4, 0)) == inv  # a photometric parameter without a column, a coefficient with one
    assert update(mu=None) == inv and update(sigma=None) == inv                              # only one of mu / sigma
    torch.cuda.synchronize()
    after = state_of(h)
    assert all(np.array_equal(after[k], before[k]) for k in before) and np.all(after["niter"] == 0)   # none of the refused calls ran
    h.begin(case["x0"], case["lo"], np.where(np.arange(K) == 3, 5.0, case["hi"]))            # Av's box reaches 5
    assert update() == inv
    big = phot_case(np.random.default_rng(2), B, 2, 2, 3, n, 65, n, n)
    h.begin(case["x0"], case["lo"], case["hi"])
    assert update_phot(lib, h, big, rows, flux, w, x, n, n, phot_on_device(big)) == _lib.E_UNSUPPORTED and b"F > 64" in lib.payne_last_error(None)
    # B == 0 succeeds and does nothing; F == 0 with null arrays and no priors, P == 0 with a null x are allowed
    assert lib.payne_lmfit_begin(h._h, None, case["lo"].ctypes.data, case["hi"].ctypes.data, 0, None) == 0
    assert update(rows=None, flux=None, w=None, x=None, mags=None, dmags=None, obs=None, pw=None, mu=None, sigma=None) == 0
    h.begin(case["x0"], case["lo"], case["hi"])
    assert update(F=0, mags=None, dmags=None, obs=None, pw=None) == 0
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 1)
    h.close()
    plain = phot_case(np.random.default_rng(3), B, 4, 2, 0, n, 5, n, n)
    h = handle(plain["K"], 4)
    h.begin(plain["x0"], plain["lo"], plain["hi"])
    assert update_phot(lib, h, plain, dev(plain["rows"]), dev(plain["flux"]), dev(plain["w"]), None, n, n, phot_on_device(plain)) == 0
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 1)
    with pytest.raises(ValueError):
        h.update_phot(dev(plain["rows"]), dev(plain["flux"]), dev(plain["w"]), None, 0, 7, plain["sed_col"], *[phot_on_device(plain)[k] for k in ("mags", "dmags", "obs", "pw")])
    h.close()
