"""Labels and continuum polynomial in one Levenberg-Marquardt fit (payne_lmfit_update_poly, OptFit.fit_joint) -- what runs without a
GPU: the kernel's arithmetic (csrc/lmfit_core.hpp: tile_sums_poly_host) executed on the host under ASan / UBSan
(tests/emul/lmfit_poly_emul.cpp, a program of its own) against numpy, the fp64 joint reference loop the GPU tests compare with (and
that it converges on the inputs those tests use), and fit_joint's argument checks.  The kernel itself: tests/test_lmfit_poly_gpu.py,
which shares the helpers defined here.

Bounds, derived:
  sums   The rows of R = [p dm/dtheta ; m T_j ; f - m p] are rebuilt here operation by operation as the core forms them -- T_j and p by
         its recurrence with every fma evaluated in exact rational arithmetic and rounded once, the products in fp64 -- so the
         reference's rows are the core's, bit for bit, whatever P is: P lengthens the evaluation of a row's entries, which is repeated
         exactly, not the sums.  What is left is the rounding of the two sums over n terms, u = 2^-53 a rounding.  The core's: a term
         is R_i fl(R_j w), one rounding, and passes through at most n rounded accumulations (fused multiply-adds), (n + 1) u.  The
         einsum's: (R_i R_j) w, two roundings, and at most n - 1 additions, (n + 1) u.  Together
         |G - einsum| <= (n + 1) 2^-52 sum_p |R_i R_j| w: the form of tests/test_contfit.py's (a), whose n 2^-52 leaves the
         reference's own rounding out and cannot hold at n = 1, where each side is rounded twice.
  (b)    tests/test_contfit.py's: max_p |p(x_p) - p_oracle(x_p)| <= max(n, 16) 2^-52 cond_2(A^) max_p |p_oracle|.
  step   tests/test_lmfit.py's STEP_TOL, 1e-10 of a parameter's conditional sigma."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from numpy.polynomial.chebyshev import chebvander

from thepayne_amd import _lib, synth
from test_lmfit import (DEFAULTS, RUNNING, CONVERGED, NAN, STEP_TOL, RECOVERY_MAX_EVALS, g20, sums_case, parse_state, lm_reference, OracleModel,   # noqa: F401
                        recovery_inputs, sigma_distance)
from test_contfit import (EPS, ALT_NOBS, ALT_STARS, ALT_P, abscissa_of, cheb_table, contfit_case, unaligned, oracle_star, alternation_inputs,
                          alternation_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_N = (1, 5, 37, 1000)
SHAPES = ((0, 1), (0, 4), (4, 4), (5, 9), (1, 14), (14, 1))      # (K_m, P)
BIG = 1e30


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def poly_case(rng, B, Km, P, n, ld, ld_f):
    """tests/test_lmfit.py's sums_case with Km derivative rows (rows fp32 [B, 1 + Km, ld], w fp64 [B, ld_f]: a tenth of the pixels has
    w = 0, star 1 holds NaN in rows and flux there, 1e30 beyond n) whose flux is multiplied by a Chebyshev series (c_0 in [0.5, 2],
    |c_j| <= 0.1); the trial coefficients are 10 % off it.  Returns dict(rows, flux, w, x [n], coef [B, P] (the trial), n, Km, P)."""
    rows, flux, w = sums_case(rng, B, Km, n, ld, ld_f)
    x = abscissa_of(n)
    truth = np.concatenate([rng.uniform(0.5, 2.0, (B, 1)), rng.uniform(-0.1, 0.1, (B, P - 1))], axis=1)
    flux[:, :n] = (flux[:, :n].astype(np.float64) * (chebvander(x, P - 1) @ truth.T).T).astype(np.float32)
    coef = truth * (1.0 + 0.1 * rng.normal(0, 1, (B, P)))
    return dict(rows=rows, flux=flux, w=w, x=x, coef=coef, n=n, Km=Km, P=P, B=B, ld=ld, ld_f=ld_f)


def fma_exact(a, b, c):
    """fma(a, b, c) element by element: the exact rational a b + c, rounded once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    with np.errstate(invalid="ignore", over="ignore"):
        out[~fin] = (a * b + c)[~fin]                                 # (NaN or infinity: no rounding to speak of)
    flat = out.reshape(-1)
    for k in np.flatnonzero(fin.reshape(-1)):
        flat[k] = float(Fraction(a.flat[k]) * Fraction(b.flat[k]) + Fraction(c.flat[k]))
    return flat.reshape(a.shape)


def poly_rows(case, coef=None, stars=None):
    """R [B, K + 1, n] in fp64 as lmfit_core.hpp forms it (operand_poly on series_value), zero where w == 0."""
    n, Km, P = case["n"], case["Km"], case["P"]
    stars = range(case["B"]) if stars is None else stars
    coef = case["coef"] if coef is None else coef
    T = cheb_table(case["x"], P)                                       # [n, P], the core's recurrence, exact
    out = []
    for b in stars:
        c = coef[b]
        p = np.full(n, c[0])
        for k in range(1, P):
            p = fma_exact(c[k], T[:, k], p)
        m = case["rows"][b, 0, :n].astype(np.float64)
        f = case["flux"][b, :n].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            R = np.concatenate([case["rows"][b, 1:, :n].astype(np.float64) * p[None, :], m[None, :] * T.T, fma_exact(-m, p, f)[None, :]], axis=0)
        out.append(np.where(case["w"][b, :n][None, :] == 0.0, 0.0, R))
    return np.array(out)


def check_poly_tiles(G, case, what, coef=None, stars=None):
    """G [len(stars), 16, 16] inside the sums' bound; zero outside the (K + 1) x (K + 1) block.  Returns the largest ratio met."""
    n, K = case["n"], case["Km"] + case["P"]
    stars = list(range(case["B"]) if stars is None else stars)
    R = poly_rows(case, coef=coef, stars=stars)
    ww = case["w"][stars, :n]
    want = np.einsum("bip,bjp,bp->bij", R, R, ww)
    bound = (n + 1) * EPS * np.einsum("bip,bjp,bp->bij", np.abs(R), np.abs(R), ww)
    got = G[:, :K + 1, :K + 1]
    ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print("%s Km=%d P=%d n=%d: max |dG| / bound = %.3g" % (what, case["Km"], case["P"], n, ratio))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound), (what, case["Km"], case["P"], n, ratio)
    outside = G.copy()
    outside[:, :K + 1, :K + 1] = 0.0
    assert not outside.any()
    return ratio


# ---- the emulator -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poly_emul(tmp_path_factory):
    """tests/emul/lmfit_poly_emul.cpp built with the sanitizers as a program of its own; run(x0 [B, K], lo, hi, flux, w, x,
    rows_per_update, n, P, expect=0, **opts) -> (state after begin, [G [B, 16, 16] per update], [state per update])."""
    build = tmp_path_factory.mktemp("lmfit_poly_emul")
    exe = str(build / "lmfit_poly_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "lmfit_poly_emul.cpp")],
                   check=True)
    count = [0]

    def run(x0, lo, hi, flux, w, x, rows_per_update, n, P, expect=0, K=None, **opts):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        o = dict(DEFAULTS, **opts)
        B = x0.shape[0]
        K = x0.shape[1] if K is None else K
        ld, ld_f, T = rows_per_update[0].shape[2], flux.shape[1], len(rows_per_update)
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d %d\n%s %d\n" % (B, K, P, n, ld, ld_f, T, " ".join(repr(float(o[k])) for k in ("lambda0", "down", "up", "lambda_min", "lambda_max", "xtol")),
                                                     o["maxiter"]))
        for nm, a, dt in (("x0", x0, np.float64), ("lo", lo, np.float64), ("hi", hi, np.float64), ("flux", flux, np.float32), ("w", w, np.float64), ("x", x, np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        for t, r in enumerate(rows_per_update):
            np.ascontiguousarray(r, dtype=np.float32).tofile(str(d / ("rows%d.bin" % t)))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        if expect:
            return None
        begin = parse_state(np.fromfile(str(d / "state_begin.bin")), B, K)
        Gs = [np.fromfile(str(d / ("G%d.bin" % t))).reshape(B, 16, 16) for t in range(T)]
        states = [parse_state(np.fromfile(str(d / ("state%d.bin" % t))), B, K) for t in range(T)]
        return begin, Gs, states
    return run


def start_of(case):
    """(x0 [B, K], lo, hi): zeros for the model's parameters, the case's trial coefficients, a box that holds both."""
    Km, P = case["Km"], case["P"]
    x0 = np.concatenate([np.zeros((case["B"], Km)), case["coef"]], axis=1)
    return x0, np.full(Km + P, -1e6), np.full(Km + P, 1e6)


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Km,P", SHAPES)
@pytest.mark.parametrize("n", SUM_N)
def test_sums_against_einsum_on_the_host(poly_emul, Km, P, n):
    rng = np.random.default_rng(10000 * Km + 100 * P + n)
    K = Km + P
    case = poly_case(rng, 3, Km, P, n, n + 3, n + 6)
    x0, lo, hi = start_of(case)
    begin, Gs, states = poly_emul(x0, lo, hi, case["flux"], case["w"], case["x"], [case["rows"]], n, P)
    check_poly_tiles(Gs[0], case, "emulator")
    st = states[0]                                                    # the stored matrix, gradient and chi^2 are the tile's
    assert np.array_equal(st["A"], np.triu(Gs[0][:, :K, :K]) + np.swapaxes(np.triu(Gs[0][:, :K, :K], 1), 1, 2))
    assert np.array_equal(st["g"], Gs[0][:, :K, K]) and np.array_equal(st["chisq"], Gs[0][:, K, K]) and np.all(st["niter"] == 1)
    # a NaN at a weighted pixel reaches chi^2
    p = int(np.flatnonzero(case["w"][2, :n] > 0)[0])
    rows2 = case["rows"].copy()
    rows2[2, 0, p] = np.nan
    begin, G2, st2 = poly_emul(x0, lo, hi, case["flux"], case["w"], case["x"], [rows2], n, P)
    assert np.isnan(G2[0][2, K, K]) and st2[0]["status"][2] == NAN and np.array_equal(G2[0][:2], Gs[0][:2]) and np.all(st2[0]["status"][:2] != NAN)


# ---- 2. a linear model ----------------------------------------------------------------------------------------------------------
def linear_case(n, P, N=3):
    """tests/test_contfit.py's contfit_case as a K_m = 0 problem: (case, rows fp32 [N, 1, ld_m], an arbitrary start c [N, P])."""
    rng = np.random.default_rng(50 * P + n)
    case = contfit_case(rng, N, P, n, unaligned(n))
    start = case["truth"] * (1.0 + 0.3 * rng.normal(0, 1, (N, P))) + 0.05 * rng.normal(0, 1, (N, P))
    return case, np.ascontiguousarray(case["model"][:, None, :]), start


def check_linear(case, coef, what):
    """coef [N, P] against oracle_star's within bound (b)."""
    n, P = case["n"], case["P"]
    V = chebvander(case["x"], P - 1)
    worst = 0.0
    for s in range(case["N"]):
        o = oracle_star(case["flux"][s, :n], case["w"][s, :n], case["model"][s, :n], case["x"], P)
        assert o["status"] == 0
        p_o, p_g = V @ o["coef"], V @ coef[s]
        bound = max(n, 16) * EPS * o["cond"] * np.abs(p_o).max()
        worst = max(worst, float(np.abs(p_g - p_o).max() / bound))
        assert np.all(np.isfinite(coef[s])) and np.abs(p_g - p_o).max() <= bound, (what, n, P, s, np.abs(p_g - p_o).max(), bound)
    print("%s n=%d P=%d: |dp| / bound (b) = %.3g" % (what, n, P, worst))


LINEAR = [(5, 1), (37, 4), (1000, 4), (1000, 9), (37, 15), (3600, 15)]


@pytest.mark.parametrize("n,P", LINEAR)
def test_one_gauss_newton_step_solves_the_polynomial(poly_emul, n, P):
    """K_m = 0: the model is linear in c, so with lambda0 = lambda_min = 0 one update from an arbitrary c lands on the least-squares
    polynomial, which tests/test_contfit.py's numpy oracle gives."""
    case, rows, start = linear_case(n, P)
    begin, Gs, states = poly_emul(start, np.full(P, -BIG), np.full(P, BIG), case["flux"], case["w"], case["x"], [rows], n, P, lambda0=0.0, lambda_min=0.0, xtol=0.0)
    assert np.all(states[0]["status"] == RUNNING) and np.all(states[0]["lam"] == 0.0) and np.all(states[0]["at_bound"] == 0)
    check_linear(case, states[0]["x_trial"], "emulator")


# ---- 3. the joint reference loop ------------------------------------------------------------------------------------------------
_JOINT = {}


def joint_inputs(g20, nobs):
    """(net, nntype, case, coef [stars, P], flux fp64 [stars, nobs], x): tests/test_contfit.py's alternation_inputs at its nobs, and the
    same construction (the recovery stars' spectra at the truth times a P = 4 series) at another."""
    if nobs == ALT_NOBS:
        return alternation_inputs(g20)
    if ("in", nobs) not in _JOINT:
        from thepayne_amd.fitting.contfit import abscissa
        net, nntype, case, _ = recovery_inputs(g20, "synth5", nobs, False)
        rng = np.random.default_rng(321)
        coef = np.concatenate([rng.uniform(0.5, 2.0, (ALT_STARS, 1)), rng.uniform(-0.1, 0.1, (ALT_STARS, ALT_P - 1))], axis=1)
        x = abscissa(case["obs_wave"])
        poly = chebvander(x, ALT_P - 1) @ coef.T
        flux = np.array([OracleModel(net, nntype, case["obs_wave"], case["truth"][i])(case["truth"][i][case["cols"]])[0] * poly[:, i] for i in range(ALT_STARS)])
        _JOINT[("in", nobs)] = (net, nntype, case, coef, flux, x)
    return _JOINT[("in", nobs)]


def joint_fit(g20, star, nobs, P, fit_vrad, dtype=None):
    """lm_reference on the joint model of one star: model = m p, J = [p dm ; m T_j], the start the case's plus oracle_star's
    polynomial at the start model, the coefficients' box +-1e30.  The flux is the fp32 one the device is given."""
    net, nntype, case, _, flux, x = joint_inputs(g20, nobs)
    V = chebvander(x, P - 1)
    cols = case["cols"] + ([4] if fit_vrad else [])
    Km = len(cols)
    om = OracleModel(net, nntype, case["obs_wave"], case["start"][star], fit_vrad=fit_vrad, dtype=dtype)
    f = flux[star].astype(np.float32).astype(np.float64)
    w = 1.0 / case["eflux"][star] ** 2
    o = oracle_star(f.astype(np.float32), w, om(case["start"][star][cols])[0].astype(np.float32), x, P)
    assert o["status"] == 0
    start = np.concatenate([case["start"][star][cols], o["coef"]])

    def fun(z):
        m, J = om(z[:Km])
        p = V @ z[Km:]
        return m * p, np.concatenate([J * p[None, :], m[None, :] * V.T], axis=0)
    lo = np.concatenate([net["xmin"], [-500.0] if fit_vrad else [], np.full(P, -BIG)])
    hi = np.concatenate([net["xmax"], [500.0] if fit_vrad else [], np.full(P, BIG)])
    return lm_reference(fun, start, lo, hi, f, w)


def joint_reference(g20, nobs, P, fit_vrad):
    """The fp64 joint loop on every star of joint_inputs, cached for the GPU test."""
    key = ("ref", nobs, P, fit_vrad)
    if key not in _JOINT:
        _JOINT[key] = [joint_fit(g20, i, nobs, P, fit_vrad) for i in range(ALT_STARS)]
    return _JOINT[key]


def marginal_distance(a, b, A, Km):
    """max over the first Km parameters of |a - b| in marginal sigma, sqrt(diag(inv(A)))."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))[:Km] / np.sqrt(np.diag(np.linalg.inv(A)))[:Km]))


JOINT_CASES = [(ALT_NOBS, ALT_P, False), (ALT_NOBS, 9, True), (37, ALT_P, False)]


@pytest.mark.parametrize("nobs,P,fit_vrad", JOINT_CASES)
def test_joint_reference_loop_converges(g20, nobs, P, fit_vrad):
    """The inputs tests/test_lmfit_poly_gpu.py fits on the device: the fp64 joint loop ends CONVERGED on every star within
    RECOVERY_MAX_EVALS evaluations and, on tests/test_contfit.py's own inputs, within 1e-2 marginal sigma (its own A) of where the
    40-round alternation ends; elsewhere of the truth.  Measured: 3 evaluations, 2.2e-3 sigma at most."""
    net, nntype, case, coef, flux, x = joint_inputs(g20, nobs)
    D = len(case["cols"])
    ends = [r[0]["x"] for r in alternation_reference(g20)] if nobs == ALT_NOBS else [case["truth"][i][case["cols"]] for i in range(ALT_STARS)]
    for i, res in enumerate(joint_reference(g20, nobs, P, fit_vrad)):
        d = marginal_distance(res["x"][:D], ends[i], res["A"], D) if res["status"] == CONVERGED else np.inf
        print("nobs=%d P=%d fit_vrad=%s star %d: status %d after %d evaluations, chi^2 %.3g, %.3g marginal sigma from %s"
              % (nobs, P, fit_vrad, i, res["status"], res["niter"], res["chisq"], d, "the alternation's end" if nobs == ALT_NOBS else "the truth"))
        assert res["status"] == CONVERGED and res["niter"] <= RECOVERY_MAX_EVALS and res["at_bound"] == 0, (nobs, P, fit_vrad, i, res["status"], res["niter"])
        assert d <= 1e-2, (nobs, P, fit_vrad, i, d)
        assert res["x"].shape == (D + int(fit_vrad) + P,)


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------
def test_fit_joint_argument_checks():
    from thepayne_amd.fitting import optfit
    xmin, xmax = synth.SPEC_LABEL_MIN, synth.SPEC_LABEL_MAX
    N, nobs = 3, 10
    flux, eflux = np.ones((N, nobs)), np.full((N, nobs), 0.01)
    start = np.tile([5000.0, 4.0, 0.0, 0.1, 10.0, 5.0, np.nan, 20000.0], (N, 1))

    def check(n_labels=4, **kw):
        return optfit.check_joint_args(flux, eflux, start, nobs, n_labels, xmin, xmax, **kw)
    f, e, s, lo, hi, o, coef, clip = check()
    assert len(lo) == len(hi) == 8 and np.array_equal(lo[:4], xmin) and np.all(lo[4:] == -optfit.COEF_BOUND) and np.all(hi[4:] == optfit.COEF_BOUND)
    assert coef is None and clip == {} and o == optfit.LM_DEFAULTS and np.isfinite(optfit.COEF_BOUND)
    f, e, s, lo, hi, o, coef, clip = check(npoly=2, fit_vrad=True, coef=np.ones((N, 2)), coef_bounds=[(0.0, 3.0), (-1.0, 1.0)], bounds={"Vrad": (-50.0, 60.0)}, xtol=1e-4)
    assert list(lo[4:]) == [-50.0, 0.0, -1.0] and list(hi[4:]) == [60.0, 3.0, 1.0] and coef.dtype == np.float64 and o["xtol"] == 1e-4
    assert check(clip=dict(nclip=3, kappa=2.5, rescale=True))[7] == dict(nclip=3, kappa=2.5, rescale=True)
    assert len(check(npoly=11)[3]) == 15 and len(check(npoly=10, fit_vrad=True)[3]) == 15                    # a full tile
    for bad in (dict(npoly=12), dict(npoly=11, fit_vrad=True), dict(npoly=0), dict(npoly=2.5), dict(npoly=True),   # K_m + P > 15; no integer >= 1
                dict(coef=np.ones((N, 3))), dict(coef=np.ones((N + 1, 4))), dict(coef=np.full((N, 4), np.nan)),
                dict(coef_bounds=np.zeros((3, 2))), dict(coef_bounds=[(1.0, 0.0)] * 4), dict(coef_bounds=[(0.0, np.inf)] * 4),
                dict(clip=dict(drop_clipped=False)), dict(clip=dict(nclip=2), coef=np.ones((N, 4))),
                dict(bounds={"Teff": (6000.0, 4000.0)}), dict(vrad_step=0.0), dict(maxiter=0), dict(n_labels=5)):
        with pytest.raises(ValueError):
            check(**bad)
    with pytest.raises(TypeError):
        check(ftol=1e-3)
    F = object.__new__(optfit.OptFit)
    with pytest.raises(NotImplementedError):
        F.fit_joint(flux, eflux, start, lsf=np.full(nobs, 0.1))
    assert "payne_lmfit_update_poly" in _lib.SYMBOLS and hasattr(optfit.LMHandle, "update_poly")
    assert "fit_joint" in optfit.OptFit.fit_with_continuum.__doc__


def test_the_emulator_refuses_what_the_library_refuses(poly_emul):
    case = poly_case(np.random.default_rng(1), 2, 2, 3, 37, 40, 44)
    x0, lo, hi = start_of(case)
    args = (case["flux"], case["w"], case["x"], [case["rows"]], 37)
    assert poly_emul(x0, lo, hi, *args, 3) is not None
    for P in (0, -1, 6):                                              # P < 1, P > K
        assert poly_emul(x0, lo, hi, *args, P, expect=3) is None
    assert poly_emul(x0, lo, hi, *args, 3, expect=3, K=16) is None and poly_emul(x0, lo, hi, *args, 3, expect=3, K=0) is None
    assert poly_emul(x0, lo, hi, case["flux"], case["w"], case["x"], [case["rows"]], 0, 3, expect=3) is None      # n < 1
    assert poly_emul(x0, lo, hi, case["flux"], case["w"], case["x"], [case["rows"]], 41, 3, expect=3) is None     # ld < n
    assert poly_emul(x0, lo, np.where(np.arange(5) == 4, np.inf, hi), *args, 3, expect=3) is None                 # a box that is not finite
    assert poly_emul(x0, lo, hi, *args, 3, expect=3, lambda0=-1.0) is None
