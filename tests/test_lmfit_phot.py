"""Spectrum and photometry in one Levenberg-Marquardt fit (payne_lmfit_update_phot, OptFit.fit_specphot) -- what runs without a GPU:
the kernel's arithmetic (csrc/lmfit_core.hpp: tile_sums_gap_host; csrc/lmfit_phot_core.hpp) executed on the host under ASan / UBSan
(tests/emul/lmfit_phot_emul.cpp, a program of its own) against a long-double reference, the degenerate cases against the two older
emulators, the fp64 joint reference loop the GPU tests compare with (and that it converges on the inputs those tests use), and the
argument checks.  The kernel itself: tests/test_lmfit_phot_gpu.py, which shares the helpers defined here.

Bounds, derived (u = 2^-53 a rounding, first order in u):
  sums   The rows of both blocks are rebuilt here operation by operation as the core forms them -- the spectral ones as
         tests/test_lmfit_poly.py's poly_rows does (P = 0: one subtraction), with K_p zero rows in the gap; the photometric ones are the
         derivatives as given and obs - mag, one subtraction -- so the reference's rows are the core's, bit for bit, and what is left is
         the rounding of the sums, which the reference (numpy.longdouble, 2^-64) does not share.  Per term, rounded operations it passes
         through, the final tile + g included:
           spectral     R_i fl(R_j w): 1, at most n accumulations, the final sum: n + 2
           photometric  fl(R_i pw) R_j: 1, at most F accumulations (fma), at most K more where the priors' terms follow on chi^2, the
                        final sum: F + K + 2
           priors       iv = 1 / (sigma sigma): 2; d = mu - x: 1; on A_kk one addition and the final sum: 4; on g_k one fma and the
                        final sum: 5; on chi^2 fl(d d): 3 with d's, iv's 2, its own fma and those of the priors behind it, at most K, the
                        final sum: K + 6
         The issue's constant n + F + K + 4 covers all of these as soon as n + F >= 2 and is kept as it is stated; no group's count is
         smaller than its own share of it by more than the other groups' sizes, so nothing smaller is claimed.  At n = 1, F = 0 the
         count for chi^2 with a prior on every parameter is K + 6 against K + 5: a worst case in which every rounding has the same sign.
         |dG| <= (n + F + K + 4) 2^-53 (sum_p |R_i R_j| w + sum_f |R_i R_j| pw + |prior terms|) on the upper triangle, column K
         included: the block is added there, which is all update_star reads; below the diagonal the tile is the spectral one alone.
  step   tests/test_lmfit.py's STEP_TOL, 1e-10 of a parameter's conditional sigma."""
import os
import subprocess

import numpy as np
import pytest
from numpy.polynomial.chebyshev import chebvander

from thepayne_amd import _lib, synth
from test_lmfit import (DEFAULTS, RUNNING, CONVERGED, SINGULAR, NAN, STEP_TOL, g20, emul as plain_emul, sums_case, parse_state, lm_reference, OracleModel,   # noqa: F401
                        recovery_net, recovery_case, sigma_distance)
from test_contfit import abscissa_of, oracle_star
from test_lmfit_poly import BIG, poly_case, poly_rows, poly_emul                                    # noqa: F401
import test_sedfit as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = 2.0 ** -53
SHAPES = ((4, 2, 4), (4, 3, 0), (6, 3, 6), (1, 1, 0), (4, 0, 4))      # (K_m, K_p, P)
SUM_N = (1, 5, 37, 1000)
SUM_F = (0, 1, 7, 33, 64)
AV_HI = 4.5


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def sed_cols_of(Km, Kp, P, ncol=7):
    """sed_col [K]: the first four model parameters are the shared labels, the others of the model see no magnitude; the K_p
    photometric ones are the last K_p columns of the row (so that Av is among them); the coefficients none."""
    return np.array(list(range(min(Km, 4))) + [-1] * max(Km - 4, 0) + list(range(ncol - Kp, ncol)) + [-1] * P, dtype=np.int32)


def phot_case(rng, B, Km, Kp, P, n, F, ld, ld_f, prior=False, ncol=7):
    """tests/test_lmfit_poly.py's poly_case (P = 0: tests/test_lmfit.py's sums_case) with a photometric block: mags, obs, pw fp64
    [B, F], dmags fp64 [B, F, ncol] of order one; a tenth of the filters has pw = 0 (F > 1) and all four arrays hold NaN there.
    prior: mu, sigma [B, K], a third of the sigmas infinite.  x0 [B, K] is zero but for the trial coefficients; the box is wide but
    for the parameter on the row's last column, Av, whose upper bound must stay below 5."""
    if P:
        case = poly_case(rng, B, Km, P, n, ld, ld_f)
    else:
        rows, flux, w = sums_case(rng, B, Km, n, ld, ld_f)
        case = dict(rows=rows, flux=flux, w=w, x=abscissa_of(n), coef=np.zeros((B, 0)), n=n, Km=Km, P=0, B=B, ld=ld, ld_f=ld_f)
    K = Km + Kp + P
    sed_col = sed_cols_of(Km, Kp, P, ncol)
    mags = rng.normal(15.0, 2.0, (B, F))
    dmags = rng.normal(0.0, 1.0, (B, F, ncol)) * 10.0 ** rng.uniform(-3, 0, (1, 1, ncol))
    obs = mags + 0.05 * rng.normal(0, 1, (B, F))
    pw = 1.0 / rng.uniform(0.01, 0.1, (B, F)) ** 2
    if F > 1:
        zero = rng.uniform(size=(B, F)) < 0.1
        zero[:, 0] = False
        pw[zero], mags[zero], obs[zero], dmags[zero] = 0.0, np.nan, np.nan, np.nan
    x0 = np.concatenate([np.zeros((B, Km + Kp)), case["coef"]], axis=1)
    lo, hi = np.full(K, -1e6), np.full(K, 1e6)
    hi[sed_col == ncol - 1] = AV_HI
    mu = sigma = None
    if prior:
        mu, sigma = rng.normal(0, 1, (B, K)), 10.0 ** rng.uniform(-2, 1, (B, K))
        sigma[rng.uniform(size=(B, K)) < 1.0 / 3.0] = np.inf
    case.update(Kp=Kp, K=K, F=F, ncol=ncol, sed_col=sed_col, mags=mags, dmags=dmags, obs=obs, pw=pw, x0=x0, lo=lo, hi=hi, mu=mu, sigma=sigma)
    return case


def spectral_rows(case, stars=None):
    """R [stars, K + 1, n] of the spectral tile as lmfit_core.hpp forms it: zero rows in the gap, zero where w == 0."""
    n, Km, Kp, P = case["n"], case["Km"], case["Kp"], case["P"]
    stars = list(range(case["B"]) if stars is None else stars)
    if P:
        R = poly_rows(case, stars=stars)
    else:
        rows, flux = case["rows"][stars], case["flux"][stars]
        with np.errstate(invalid="ignore", over="ignore"):
            R = np.concatenate([rows[:, 1:, :n].astype(np.float64), (flux[:, :n].astype(np.float64) - rows[:, 0, :n].astype(np.float64))[:, None, :]], axis=1)
        R = np.where(case["w"][stars, :n][:, None, :] == 0.0, 0.0, R)
    return np.concatenate([R[:, :Km], np.zeros((len(stars), Kp, n)), R[:, Km:]], axis=1)


def phot_rows(case, mags=None, dmags=None, stars=None):
    """R [stars, K + 1, F] of the photometric block as lmfit_phot_core.hpp forms it, zero where pw == 0."""
    stars = list(range(case["B"]) if stars is None else stars)
    mags, dmags = (case["mags"] if mags is None else mags)[stars], (case["dmags"] if dmags is None else dmags)[stars]
    K, sc = case["K"], case["sed_col"]
    R = np.zeros((len(stars), K + 1, case["F"]))
    for k in range(K):
        if sc[k] >= 0:
            R[:, k] = dmags[:, :, sc[k]]
    R[:, K] = case["obs"][stars] - mags
    return np.where(case["pw"][stars][:, None, :] == 0.0, 0.0, R)


def reference_tiles(case, x=None, stars=None):
    """(G, the bound) [stars, K + 1, K + 1] in long double / fp64: both blocks' sums and the priors' terms at x (default x0)."""
    stars = list(range(case["B"]) if stars is None else stars)
    n, F, K = case["n"], case["F"], case["K"]
    Rs, Rp = spectral_rows(case, stars).astype(LD), phot_rows(case, stars=stars).astype(LD)
    w, pw = case["w"][stars, :n].astype(LD), case["pw"][stars].astype(LD)
    G = (Rs[:, :, None, :] * Rs[:, None, :, :] * w[:, None, None, :]).sum(-1) + (Rp[:, :, None, :] * Rp[:, None, :, :] * pw[:, None, None, :]).sum(-1)
    mag = (np.abs(Rs)[:, :, None, :] * np.abs(Rs)[:, None, :, :] * w[:, None, None, :]).sum(-1) \
        + (np.abs(Rp)[:, :, None, :] * np.abs(Rp)[:, None, :, :] * pw[:, None, None, :]).sum(-1)
    if case["sigma"] is not None:
        x = (case["x0"] if x is None else x)[stars]
        sig = case["sigma"][stars]
        has = np.isfinite(sig)
        iv = np.where(has, 1.0 / np.where(has, sig, 1.0).astype(LD) ** 2, LD(0.0))
        d = np.where(has, case["mu"][stars].astype(LD) - x.astype(LD), LD(0.0))
        k = np.arange(K)
        for T, sgn in ((G, 1), (mag, 0)):
            T[:, k, k] += iv
            T[:, k, K] += d * iv if sgn else np.abs(d) * iv
            T[:, K, k] += d * iv if sgn else np.abs(d) * iv
            T[:, K, K] += (d * d * iv).sum(axis=1)
    return G, ((n + F + K + 4) * U * mag).astype(np.float64)


def check_phot_tiles(G, case, what, stars=None):
    """The upper triangle of G [len(stars), 16, 16] inside the sums' bound; zero outside the (K + 1) x (K + 1) block.  Returns the
    largest ratio met."""
    K = case["K"]
    want, bound = reference_tiles(case, stars=stars)
    iu = np.triu_indices(K + 1)
    got = G[:, :K + 1, :K + 1][:, iu[0], iu[1]]
    err = np.abs(got.astype(LD) - want[:, iu[0], iu[1]]).astype(np.float64)
    bnd = bound[:, iu[0], iu[1]]
    ratio = float((err / np.maximum(bnd, 1e-300)).max())
    print("%s Km=%d Kp=%d P=%d n=%d F=%d priors=%s: max |dG| / bound = %.3g" % (what, case["Km"], case["Kp"], case["P"], case["n"], case["F"], case["sigma"] is not None, ratio))
    assert np.all(np.isfinite(got)) and np.all(err <= bnd), (what, case["Km"], case["Kp"], case["P"], case["n"], case["F"], ratio)
    outside = G.copy()
    outside[:, :K + 1, :K + 1] = 0.0
    assert not outside.any()
    return ratio


# ---- the emulator -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def phot_emul(tmp_path_factory):
    """tests/emul/lmfit_phot_emul.cpp built with the sanitizers as a program of its own; run(case, updates = [(rows, mags, dmags)],
    expect=0, cfg overrides and options) -> (state after begin, [G [B, 16, 16] per update], [state per update])."""
    build = tmp_path_factory.mktemp("lmfit_phot_emul")
    exe = str(build / "lmfit_phot_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "lmfit_phot_emul.cpp")],
                   check=True)
    count = [0]

    def run(case, updates=None, expect=0, K=None, Km=None, Kp=None, P=None, n=None, F=None, ncol=None, prior=None, sed_col=None, lo=None, hi=None, **opts):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        o = dict(DEFAULTS, **opts)
        updates = [(case["rows"], case["mags"], case["dmags"])] if updates is None else updates
        B, K_ = case["B"], case["K"]
        cfg = [B, K_ if K is None else K, case["Km"] if Km is None else Km, case["Kp"] if Kp is None else Kp, case["P"] if P is None else P,
               case["n"] if n is None else n, case["ld"], case["ld_f"], len(updates), case["F"] if F is None else F, case["ncol"] if ncol is None else ncol,
               (int(case["sigma"] is not None) if prior is None else prior)]
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%s\n%s %d\n" % (" ".join(str(int(v)) for v in cfg), " ".join(repr(float(o[k])) for k in ("lambda0", "down", "up", "lambda_min", "lambda_max", "xtol")),
                                     o["maxiter"]))
        K_ = cfg[1]
        none = np.zeros((B, max(K_, 0)))
        for nm, a, dt in (("x0", case["x0"], np.float64), ("lo", case["lo"] if lo is None else lo, np.float64), ("hi", case["hi"] if hi is None else hi, np.float64),
                          ("flux", case["flux"], np.float32), ("w", case["w"], np.float64), ("x", case["x"], np.float64),
                          ("sed_col", case["sed_col"] if sed_col is None else sed_col, np.int32), ("obs", case["obs"], np.float64), ("pw", case["pw"], np.float64),
                          ("mu", none if case["mu"] is None else case["mu"], np.float64), ("sigma", none if case["sigma"] is None else case["sigma"], np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        for t, (r, m, dm) in enumerate(updates):
            np.ascontiguousarray(r, dtype=np.float32).tofile(str(d / ("rows%d.bin" % t)))
            np.ascontiguousarray(m, dtype=np.float64).tofile(str(d / ("mags%d.bin" % t)))
            np.ascontiguousarray(dm, dtype=np.float64).tofile(str(d / ("dmags%d.bin" % t)))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        if expect:
            return None
        begin = parse_state(np.fromfile(str(d / "state_begin.bin")), B, K_)
        Gs = [np.fromfile(str(d / ("G%d.bin" % t))).reshape(B, 16, 16) for t in range(len(updates))]
        states = [parse_state(np.fromfile(str(d / ("state%d.bin" % t))), B, K_) for t in range(len(updates))]
        return begin, Gs, states
    return run


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Km,Kp,P", SHAPES)
@pytest.mark.parametrize("n", SUM_N)
def test_sums_against_long_double_on_the_host(phot_emul, Km, Kp, P, n):
    worst = 0.0
    for F in SUM_F:
        for prior in (False, True):
            rng = np.random.default_rng(100000 * Km + 10000 * Kp + 1000 * P + 10 * n + F)     # (the spectral part is the same for every F)
            case = phot_case(rng, 3, Km, Kp, P, n, F, n + 3, n + 6, prior=prior)
            K = case["K"]
            begin, Gs, states = phot_emul(case)
            worst = max(worst, check_phot_tiles(Gs[0], case, "emulator"))
            st = states[0]                                            # the stored matrix, gradient and chi^2 are the tile's upper triangle
            up = np.triu(Gs[0][:, :K, :K])
            assert np.array_equal(st["A"], up + np.swapaxes(np.triu(Gs[0][:, :K, :K], 1), 1, 2))
            assert np.array_equal(st["g"], Gs[0][:, :K, K]) and np.array_equal(st["chisq"], Gs[0][:, K, K]) and np.all(st["niter"] == 1)
    print("Km=%d Kp=%d P=%d n=%d: the largest ratio over F and priors %.3g" % (Km, Kp, P, n, worst))
    # a NaN magnitude at a counting filter reaches chi^2
    case = phot_case(np.random.default_rng(5), 3, Km, Kp, P, n, 7, n + 3, n + 6)
    f = int(np.flatnonzero(case["pw"][2] > 0)[0])
    mags2 = case["mags"].copy()
    mags2[2, f] = np.nan
    ok = phot_emul(case)
    begin, G2, st2 = phot_emul(case, [(case["rows"], mags2, case["dmags"])])
    assert np.isnan(G2[0][2, K, K]) and st2[0]["status"][2] == NAN and np.array_equal(G2[0][:2], ok[1][0][:2]) and np.all(st2[0]["status"][:2] != NAN)


# ---- 2. the degenerate cases ----------------------------------------------------------------------------------------------------
def same_states(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("Km,P,n,F", [(4, 4, 37, 0), (4, 4, 37, 7), (5, 9, 1000, 33), (4, 0, 37, 0), (5, 0, 1000, 7), (1, 0, 5, 1)])
def test_without_photometry_the_state_is_the_older_emulators(phot_emul, poly_emul, plain_emul, Km, P, n, F):
    """K_p = 0, no priors, F = 0 or every pw = 0: after each of three updates the state is lmfit_poly_emul's (P >= 1) or lmfit_emul's
    (P = 0) as numbers, status / niter / at_bound included."""
    rng = np.random.default_rng(77 * Km + 7 * P + n + F)
    case = phot_case(rng, 3, Km, 0, P, n, F, n + 3, n + 6)
    case["pw"][:] = 0.0
    case["lo"][:], case["hi"][:] = -1e6, 1e6                          # (the older emulators have no Av)
    more = [phot_case(rng, 3, Km, 0, P, n, F, n + 3, n + 6) for _ in range(2)]
    updates = [(c["rows"], c["mags"], c["dmags"]) for c in [case] + more]
    begin, Gs, states = phot_emul(case, updates, hi=case["hi"])
    if P:
        b0, G0, s0 = poly_emul(case["x0"], case["lo"], case["hi"], case["flux"], case["w"], case["x"], [u[0] for u in updates], n, P)
    else:
        b0, G0, s0 = plain_emul(case["x0"], case["lo"], case["hi"], case["flux"], case["w"], [u[0] for u in updates], n)
    assert same_states(begin, b0)
    for t in range(3):
        assert same_states(states[t], s0[t]), t
        assert np.array_equal(states[t]["status"], s0[t]["status"]) and np.array_equal(states[t]["niter"], s0[t]["niter"]) and np.array_equal(states[t]["at_bound"], s0[t]["at_bound"])
        assert np.array_equal(Gs[t], G0[t], equal_nan=True)
    assert np.all(states[-1]["niter"] >= 1)


def test_a_photometric_parameter_nothing_constrains_is_singular(phot_emul):
    case = phot_case(np.random.default_rng(3), 3, 4, 2, 4, 37, 7, 40, 44)
    case["pw"][1] = 0.0                                               # star 1: no filter counts and no prior: A_kk = 0 for logR and Av
    begin, Gs, states = phot_emul(case)
    assert states[0]["status"][1] == SINGULAR and states[0]["niter"][1] == 1 and np.all(states[0]["status"][[0, 2]] == RUNNING)
    assert not Gs[0][1, 4:6, :].any() and not Gs[0][1, :, 4:6].any()
    # ... and a prior on both makes up for the filters
    case["mu"], case["sigma"] = np.zeros((3, 10)), np.full((3, 10), np.inf)
    case["sigma"][1, 4:6] = 0.5
    begin, Gs, states = phot_emul(case)
    assert states[0]["status"][1] == RUNNING and np.all(np.diag(states[0]["A"][1])[4:6] == 4.0)


# ---- 3. the joint reference loop ------------------------------------------------------------------------------------------------
NOBS, POOL, KEEP, MAX_EVALS = 37, 18, 6, 15
# The noise drawn on the magnitudes (their errors stay TS.SIGMA_MAG = 0.02 mag).  The device's spectral model is fp32, so its chi^2 at
# a point carries a rounding term of about 2 w sqrt(n) |r| eps that changes from trial to trial, r the spectral residual at the joint
# solution, which is what the magnitudes' noise pulls the shared labels off the (noiseless) spectrum's own minimum by.  update_star
# accepts a trial on chi^2 <= the best so far, and the last decisive step, xtol = 1e-3 conditional sigma, lowers chi^2 by 1e-6: the
# status is the reference's only where that term is well below 1e-6.  With w = 1e4, n = 37, eps = 6e-8 that asks for |r| of a few 1e-5,
# which a draw of 0.02 mag exceeds thirty-fold (measured on an MI355X: chi^2 scatters by 2e-6 .. 5e-6 along a line through the solution,
# and a star then ends STALLED or after a dozen rejections, at the right place and a lower chi^2 than the reference's); a twentieth of
# the error bar, 0.001 mag, keeps the term at 1e-7 .. 2.5e-7.  tests/test_lmfit.py's recovery inputs are noiseless for the same reason.
MAG_NOISE = 0.001
SP_CASES = {"a": dict(which="smlp", fit_vrad=False, photscale=False, free=("logR", "Av"), P=4),
            "b": dict(which="synth5", fit_vrad=True, photscale=False, free=("logR", "Dist", "Av"), P=4),
            "c": dict(which="smlp", fit_vrad=False, photscale=True, free=("logA", "Av"), P=0),
            "d": dict(which="synth5", fit_vrad=True, photscale=False, free=("logR", "Dist", "Av"), P=6)}
SP_NETS = (7, 16)
_SP = {}


def specphot_fun(net, nntype, phot, obs_wave, fixed, phot_row, cfg, x_abs, pk):
    """fun(z) -> (model, J) of the joint model [m p ; mags ; the parameters that carry a prior], z = [the fitted columns, the free
    photometric parameters, the coefficients]."""
    names = TS.NAMES[cfg["photscale"]]
    om = OracleModel(net, nntype, obs_wave, fixed, fit_vrad=cfg["fit_vrad"])
    Km = len(net["xmin"]) + int(cfg["fit_vrad"])
    pcols = sorted(names.index(f) for f in cfg["free"])
    Kp, P = len(pcols), cfg["P"]
    K = Km + Kp + P
    V = chebvander(x_abs, P - 1) if P else None
    nobs = len(obs_wave)

    def fun(z):
        m, J = om(z[:Km])
        if P:
            p = V @ z[Km + Kp:]
            spec, Js = m * p, np.concatenate([J * p[None, :], np.zeros((Kp, nobs)), m[None, :] * V.T], axis=0)
        else:
            spec, Js = m, np.concatenate([J, np.zeros((Kp, nobs))], axis=0)
        row = phot_row.copy()
        row[:4] = z[:4]
        row[pcols] = z[Km:Km + Kp]
        mg, Jm = TS.jac_numpy64(phot, row[None, :], cfg["photscale"])
        Jp = np.zeros((K, mg.shape[1]))
        Jp[:4] = Jm[0][:, :4].T
        Jp[Km:Km + Kp] = Jm[0][:, pcols].T
        return np.concatenate([spec, mg[0], z[pk]]), np.concatenate([Js, Jp, np.eye(K)[:, pk]], axis=1)
    return fun, Km, pcols


def specphot_inputs(g20, name, noise=None):
    """The inputs of case `name` and the fp64 joint loop's result on them, computed once: the first KEEP stars of a pool of POOL on
    which the loop ends CONVERGED within MAX_EVALS evaluations (the reference alone decides who is left out).  The spectra are the
    oracle's at the truth times a Chebyshev series (P > 0), rounded to fp32 as the device is given them, S/N 100; the magnitudes
    numpy's fp64 model at the truth plus `noise` (MAG_NOISE unless given) of noise, errors 0.02 mag; every fitted label and photometric parameter starts 10 % of its box
    off the truth, the coefficients at oracle_star's polynomial against the start's model; Dist, where it is free, has a 5 % prior."""
    noise = MAG_NOISE if noise is None else noise
    key = (name, noise)
    if key in _SP:
        return _SP[key]
    from thepayne_amd.fitting.contfit import abscissa
    cfg = SP_CASES[name]
    net, nntype = recovery_net(g20, cfg["which"])
    pool = recovery_case(net, NOBS, seed=11, N=POOL)
    phot = TS.fit_nets(*SP_NETS)
    names = TS.NAMES[cfg["photscale"]]
    rng = np.random.default_rng(4242 + ord(name))
    fit_vrad, P = cfg["fit_vrad"], cfg["P"]
    cols = pool["cols"] + ([4] if fit_vrad else [])
    D, Km = len(net["xmin"]), len(cols)
    x_abs = abscissa(pool["obs_wave"])
    ptruth = np.column_stack([rng.uniform(*TS.TRUTH[nm], POOL) for nm in names[4:]])
    pbox = np.array([TS.FIT_BOX[nm] for nm in names[4:]])
    free_i = [names.index(f) - 4 for f in cfg["free"]]
    pstart = ptruth.copy()
    pstart[:, free_i] = np.clip(ptruth[:, free_i] + 0.1 * (pbox[free_i, 1] - pbox[free_i, 0]) * rng.choice([-1.0, 1.0], (POOL, len(free_i))), pbox[free_i, 0], pbox[free_i, 1])
    ctruth = np.concatenate([rng.uniform(0.5, 2.0, (POOL, 1)), rng.uniform(-0.1, 0.1, (POOL, max(P - 1, 0)))], axis=1)[:, :P]
    mags = TS.jac_numpy64(phot, np.concatenate([pool["truth"][:, :4], ptruth], axis=1), cfg["photscale"])[0] + noise * rng.normal(0, 1, (POOL, SP_NETS[0]))
    emags = np.full(mags.shape, TS.SIGMA_MAG)
    plo, phi = np.array([TS.FIT_BOX[f][0] for f in cfg["free"]]), np.array([TS.FIT_BOX[f][1] for f in cfg["free"]])
    order = np.argsort([names.index(f) for f in cfg["free"]])
    plo, phi = plo[order], phi[order]
    pnames = [cfg["free"][i] for i in order]
    lo = np.concatenate([net["xmin"], [-500.0] if fit_vrad else [], plo, np.full(P, -BIG)])
    hi = np.concatenate([net["xmax"], [500.0] if fit_vrad else [], phi, np.full(P, BIG)])
    K = len(lo)
    keep, refs, flux, coef0 = [], [], [], []
    for s in range(POOL):
        truth = pool["truth"][s]
        f = OracleModel(net, nntype, pool["obs_wave"], truth, fit_vrad=fit_vrad)(truth[cols])[0]
        if P:
            f = f * (chebvander(x_abs, P - 1) @ ctruth[s])
        f32 = f.astype(np.float32)
        w = 1.0 / pool["eflux"][s] ** 2
        pk, pmu, psig = [], [], []
        if "Dist" in cfg["free"]:
            pk, pmu, psig = [Km + pnames.index("Dist")], [ptruth[s, names.index("Dist") - 4]], [0.05 * ptruth[s, names.index("Dist") - 4]]
        prow = np.concatenate([pool["start"][s, :4], pstart[s]])
        fun, _, pcols = specphot_fun(net, nntype, phot, pool["obs_wave"], pool["start"][s], prow, cfg, x_abs, pk)
        z0 = [pool["start"][s][cols], prow[pcols]]
        if P:
            m0 = OracleModel(net, nntype, pool["obs_wave"], pool["start"][s], fit_vrad=fit_vrad)(pool["start"][s][cols])[0]
            o = oracle_star(f32, w, m0.astype(np.float32), x_abs, P)
            assert o["status"] == 0
            z0.append(o["coef"])
            coef0.append(o["coef"])
        obs_all = np.concatenate([f32.astype(np.float64), mags[s], pmu])
        w_all = np.concatenate([w, 1.0 / emags[s] ** 2, 1.0 / np.asarray(psig) ** 2 if pk else []])
        res = lm_reference(fun, np.concatenate(z0), lo, hi, obs_all, w_all)
        print("case %s pool star %d: status %d after %d evaluations, chi^2 %.4g" % (name, s, res["status"], res["niter"], res["chisq"]))
        if res["status"] == CONVERGED and res["niter"] <= MAX_EVALS:
            keep.append(s)
            refs.append(res)
            flux.append(f32)
        if len(keep) == KEEP:
            break
    assert len(keep) == KEEP, (name, len(keep))
    prior = None
    if "Dist" in cfg["free"]:
        prior = {"Dist": (ptruth[keep, names.index("Dist") - 4], 0.05 * ptruth[keep, names.index("Dist") - 4])}
    bounds = {f: TS.FIT_BOX[f] for f in cfg["free"]}
    _SP[key] = dict(cfg=cfg, net=net, nntype=nntype, phot=phot, obs_wave=pool["obs_wave"], flux=np.array(flux), eflux=pool["eflux"][keep], start=pool["start"][keep],
                     truth=pool["truth"][keep], mags=mags[keep], emags=emags[keep], phot_start=pstart[keep], phot_truth=ptruth[keep], prior=prior, bounds=bounds, cols=cols,
                     Km=Km, Kp=len(pcols), P=P, K=K, pcols=pcols, lo=lo, hi=hi, refs=refs, keep=keep)
    return _SP[key]


REAL_CASES = ("a", "c")                                              # fitted once more with noise at the error bar (tests/test_lmfit_phot_gpu.py)


@pytest.mark.parametrize("name,noise", [(nm, None) for nm in sorted(SP_CASES)] + [(nm, TS.SIGMA_MAG) for nm in REAL_CASES])
def test_joint_reference_loop_converges(g20, name, noise):
    """The inputs tests/test_lmfit_phot_gpu.py fits on the device: the pool yields KEEP stars on which the fp64 loop on
    [m p ; mags ; priors] ends CONVERGED within MAX_EVALS evaluations, inside the box; the marginal errors say what the magnitudes add."""
    inp = specphot_inputs(g20, name, noise)
    assert len(inp["refs"]) == KEEP and inp["K"] == inp["Km"] + inp["Kp"] + inp["P"] <= 15 and (name != "d" or inp["K"] == 15) and (name != "b" or inp["K"] == 13)
    for i, res in enumerate(inp["refs"]):
        assert res["status"] == CONVERGED and res["niter"] <= MAX_EVALS and res["x"].shape == (inp["K"],)
        zt = np.concatenate([inp["truth"][i][inp["cols"]], inp["phot_truth"][i][[c - 4 for c in inp["pcols"]]]])
        sig = np.sqrt(np.diag(np.linalg.inv(res["A"])))
        print("case %s star %d (pool %d): %d evaluations, at_bound %d, |x - truth| <= %.3g marginal sigma over labels and photometric parameters"
              % (name, i, inp["keep"][i], res["niter"], res["at_bound"], np.max(np.abs(res["x"][:len(zt)] - zt) / sig[:len(zt)])))
        assert np.all(np.isfinite(sig))


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------
def test_the_emulator_refuses_what_the_library_refuses(phot_emul):
    case = phot_case(np.random.default_rng(1), 2, 4, 2, 3, 37, 7, 40, 44, prior=True)
    K = case["K"]
    assert phot_emul(case) is not None
    sc = case["sed_col"]

    def with_col(k, v):
        out = sc.copy()
        out[k] = v
        return out
    swapped = phot_case(np.random.default_rng(1), 2, 4, 2, 3, 37, 7, 44, 40, prior=True)
    assert phot_emul(swapped) is not None and phot_emul(swapped, expect=3, n=41) is None    # ld_f < n <= ld
    for bad in (dict(n=0), dict(n=41), dict(n=45),                                           # n < 1, ld < n <= ld_f, both
                dict(P=-1, Km=8), dict(Kp=-1, Km=7), dict(Km=-1, Kp=7), dict(Km=5), dict(P=2), dict(Kp=1),   # a negative count; Km + Kp + P != K
                dict(F=-1), dict(ncol=5), dict(ncol=8),
                dict(sed_col=with_col(0, -2)), dict(sed_col=with_col(0, 7)), dict(sed_col=with_col(1, 6), ncol=6),   # outside [-1, ncol)
                dict(sed_col=with_col(4, -1)), dict(sed_col=with_col(5, -1)),                                  # a photometric parameter nothing sees
                dict(sed_col=with_col(6, 0)), dict(sed_col=with_col(8, 3)),                                    # a coefficient with a column
                dict(prior=2),                                                                                 # only one of mu / sigma
                dict(hi=np.where(np.arange(K) == 5, 5.0, case["hi"])), dict(hi=np.where(np.arange(K) == 5, 1e6, case["hi"])),   # Av's box reaches 5
                dict(K=16), dict(K=0), dict(lambda0=-1.0), dict(lo=np.where(np.arange(K) == 2, np.nan, case["lo"]))):
        assert phot_emul(case, expect=3, **bad) is None, bad
    # Av on a shared label's place is held to the same rule; any other column may reach 5
    assert phot_emul(case, expect=3, sed_col=with_col(0, 6), hi=np.where(np.arange(K) == 0, 5.0, case["hi"])) is None
    assert phot_emul(case, hi=np.where(np.arange(K) == 4, 5.0, case["hi"])) is not None
    # F beyond the cap: unsupported, not invalid
    big = phot_case(np.random.default_rng(2), 2, 4, 2, 3, 37, 65, 40, 44)
    assert phot_emul(big, expect=4) is None
    assert _lib.LMFIT_PHOT_MAX_F == 64 and "payne_lmfit_update_phot" in _lib.SYMBOLS


def test_fit_specphot_argument_checks():
    from thepayne_amd.fitting import optfit, sedfit
    xmin, xmax = synth.SPEC_LABEL_MIN, synth.SPEC_LABEL_MAX
    smin, smax = synth.PHOT_LABEL_MIN, synth.PHOT_LABEL_MAX
    N, nobs, F = 3, 10, 5
    flux, eflux = np.ones((N, nobs)), np.full((N, nobs), 0.01)
    start = np.tile([5000.0, 4.0, 0.0, 0.1, 10.0, 5.0, np.nan, 20000.0], (N, 1))
    mags, emags = np.full((N, F), 12.0), np.full((N, F), 0.02)
    pstart = np.tile([0.0, 100.0, 0.3], (N, 1))

    def check(n_labels=4, photscale=False, phot_start=pstart, mags=mags, emags=emags, smin=smin, smax=smax, F=F, **kw):
        st = np.where(np.arange(8) == 6, 1.0, start) if n_labels == 5 and not kw.pop("nan_vmic", False) else start
        lo5, hi5 = (np.append(xmin, 0.5), np.append(xmax, 2.5)) if n_labels == 5 else (xmin, xmax)
        return optfit.check_specphot_args(flux, eflux, mags, emags, st, phot_start, nobs, n_labels, lo5, hi5, F, smin, smax, photscale=photscale, **kw)
    c = check()
    assert c["names"] == ["Teff", "log(g)", "[Fe/H]", "[a/Fe]", "logR", "Av"] and (c["Km"], c["Kp"], c["P"]) == (4, 2, 0) and c["coef"] is None
    assert list(c["sed_col"]) == [0, 1, 2, 3, 4, 6] and c["phot_cols"] == [4, 6] and c["mu"] is None and c["opts"] == optfit.LM_DEFAULTS
    assert np.array_equal(c["lo"][:4], np.maximum(xmin, smin[:4])) and np.array_equal(c["hi"][:4], np.minimum(xmax, smax[:4])) and c["hi"][5] < 5.0
    assert (c["lo"][4], c["hi"][4]) == sedfit.WIDE["logR"] and c["flux"].dtype == np.float32
    # the filters that do not count, as SEDFit.fit has them
    e2, m2 = emags.copy(), mags.copy()
    e2[0, :4], m2[1, 2] = [np.nan, np.inf, 0.0, -1.0], np.nan
    c = check(mags=m2, emags=e2)
    assert not c["pw"][0, :4].any() and c["pw"][1, 2] == 0.0 and c["obs"][1, 2] == 0.0 and np.count_nonzero(c["pw"]) == N * F - 5
    # every block: Vrad, all three photometric parameters with a prior, a polynomial, names and boxes by name
    pr = {"Dist": (np.full(N, 100.0), np.full(N, 5.0)), "Teff": (5000.0, np.inf)}
    c = check(fit_vrad=True, free_phot=("Av", "Dist", "logR"), npoly=3, prior=pr, bounds={"Vrad": (-50.0, 60.0), "Av": (0.0, 3.0), "pc_1": (-1.0, 1.0)},
              coef_bounds=[(0.0, 3.0), (-2.0, 2.0), (-2.0, 2.0)], xtol=1e-4)
    assert c["names"] == ["Teff", "log(g)", "[Fe/H]", "[a/Fe]", "Vrad", "logR", "Dist", "Av", "pc_0", "pc_1", "pc_2"] and list(c["sed_col"]) == [0, 1, 2, 3, -1, 4, 5, 6, -1, -1, -1]
    assert (c["lo"][4], c["hi"][4], c["hi"][7], c["lo"][8], c["lo"][9], c["hi"][9], c["lo"][10]) == (-50.0, 60.0, 3.0, 0.0, -1.0, 1.0, -2.0) and c["opts"]["xtol"] == 1e-4
    assert c["sigma"].shape == (N, 11) and np.all(c["sigma"][:, 6] == 5.0) and np.all(np.isinf(np.delete(c["sigma"], 6, axis=1))) and np.all(c["mu"][:, 6] == 100.0) and np.all(c["mu"][:, 0] == 0.0)
    c = check(n_labels=5, photscale=True, phot_start=pstart[:, :2], free_phot=("logA", "Av"))
    assert c["names"][4:] == ["Vmic", "logA", "Av"] and list(c["sed_col"]) == [0, 1, 2, 3, -1, 4, 5]
    assert check(free_phot=())["Kp"] == 0
    assert check(n_labels=5, fit_vrad=True, free_phot=("logR", "Dist", "Av"), npoly=6, prior=pr)["lo"].shape == (15,)          # a full tile
    with pytest.raises(ValueError, match="6 fitted columns of the spectrum, 3 photometric parameters and npoly = 7"):
        check(n_labels=5, fit_vrad=True, free_phot=("logR", "Dist", "Av"), npoly=7, prior=pr)
    with pytest.raises(ValueError, match="do not overlap"):
        check(smin=np.where(np.arange(6) == 0, 9000.0, smin))
    inf_s = {"Dist": (np.full(N, 100.0), np.where(np.arange(N) == 1, np.inf, 5.0))}
    for bad in (dict(free_phot=("logA",)), dict(free_phot=("Teff",)), dict(free_phot=("Av", "Av")), dict(photscale=True),      # (phot_start has three columns)
                dict(free_phot=("logR", "Dist", "Av")), dict(free_phot=("logR", "Dist"), prior=inf_s), dict(free_phot=("logR", "Dist"), prior={"Teff": (5000.0, 10.0)}),
                dict(npoly=-1), dict(npoly=2.5), dict(npoly=True), dict(coef=np.ones((N, 2))), dict(clip=dict(nclip=2)), dict(coef_bounds=[(0.0, 1.0)]),
                dict(npoly=2, coef=np.ones((N, 3))), dict(npoly=2, clip=dict(drop_clipped=False)),
                dict(bounds={"Av": (0.0, 5.0)}), dict(bounds={"Dist": (1.0, 2.0)}), dict(bounds={"Teff": (6000.0, 4000.0)}), dict(bounds=np.zeros((6, 2))),
                dict(prior={"Dist": (1.0, 1.0)}), dict(prior={"Av": (0.1, 0.0)}), dict(prior={"Av": (np.nan, 1.0)}), dict(prior={"Av": (0.1, np.nan)}),
                dict(mags=mags[:, :4]), dict(emags=emags[:2]), dict(phot_start=pstart[:, :2]), dict(phot_start=np.where(np.arange(3) == 1, np.nan, pstart)),
                dict(F=65, mags=np.ones((N, 65)), emags=np.ones((N, 65))), dict(vrad_step=0.0), dict(maxiter=0), dict(n_labels=5, nan_vmic=True)):
        with pytest.raises(ValueError):
            check(**bad)
    with pytest.raises(TypeError):
        check(ftol=1e-3)
    with pytest.raises(TypeError):
        object.__new__(optfit.OptFit).fit_specphot(flux, eflux, mags, emags, start, pstart, sed=None)
    assert hasattr(optfit.LMHandle, "update_phot") and "payne_lmfit_update_phot" in optfit.OptFit.fit_specphot.__doc__
