"""Two-component spectra in one Levenberg-Marquardt fit (payne_lmfit_update_pair, OptFit.fit_binary) -- what runs without a GPU: the
kernel's arithmetic (csrc/lmfit_pair_core.hpp: tile_sums_pair_host) executed on the host under ASan / UBSan
(tests/emul/lmfit_pair_emul.cpp, a program of its own) against numpy, the fp64 reference loop on the mixed model that the GPU tests
compare with (and that it converges on the inputs those tests use), and fit_binary's argument checks.  The kernel itself:
tests/test_lmfit_pair_gpu.py, which shares the helpers defined here.

Bounds, derived:
  sums    tests/test_lmfit_poly.py's: the rows of R are rebuilt here operation by operation as lmfit_pair_core.hpp states them -- 1 - q
          rounded once, mix = fma(cb, b, ca a) with the product rounded and the fma exact-then-rounded (fma_exact), the series by the
          core's recurrence, R_i = mix s, R_K = fma(-mix, s, f) -- so the reference's rows are the core's bit for bit and what is left
          is the rounding of the sums, |G - einsum| <= (n + 1) 2^-52 sum_p |R_i R_j| w.
  linear  K = 1 (only q), lambda = 0: the update lands on q' = q + g / A with A = sum w d^2, g = sum w d r, d = m_B - m_A (exact: two
          fp32 values of order one), r = f - ((1 - q) m_A + q m_B).  Against q* = sum w (f - m_A) d / A in exact arithmetic: r carries
          three roundings of terms no larger than |m_A| + |m_B| + |f| (the product, the two fmas) and the rounding of 1 - q, 4 2^-53
          (|m_A| + |m_B| + |f|) in all; each of the two sums (n + 1) 2^-53 relative to its terms' absolute sum (the sums' bound above);
          the scaled solve a square root, two products and two quotients, 6 2^-53 of |g / A|; the final addition 2^-53 of |q'|.  With
          max(n, 16) 2^-52 in front as in tests/test_lmfit_poly.py's bound (b):
          |q' - q*| <= max(n, 16) 2^-52 (sum w |d| (|r| + |m_A| + |m_B| + |f|) / A + |q| + |q*|).
  step    tests/test_lmfit.py's STEP_TOL, 1e-10 of a parameter's conditional sigma."""
import os
import subprocess

import numpy as np
import pytest
from numpy.polynomial.chebyshev import chebvander

from thepayne_amd import _lib, synth
from test_lmfit import (DEFAULTS, RUNNING, CONVERGED, NAN, STEP_TOL, RECOVERY_MAX_EVALS, g20, sums_case, parse_state, lm_reference, OracleModel,   # noqa: F401
                        recovery_net, recovery_case, sigma_distance)
from test_lmfit_poly import BIG, fma_exact
from test_contfit import EPS, abscissa_of, cheb_table, oracle_star

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_N = (1, 5, 37, 1000)
Q_LO, Q_HI = 0.01, 0.99


def maps_of(Ka, Kb, tied):
    """(ia, ib, Kl) of OptFit.fit_binary's order: A's columns, then B's that are not in `tied` (a tied column k is both components')."""
    free_b = [k for k in range(Kb) if k not in tied]
    ia = np.array(list(range(Ka)) + [-1] * len(free_b), dtype=np.int32)
    ib = np.array([k if k in tied else -1 for k in range(Ka)] + free_b, dtype=np.int32)
    return ia, ib, len(ia)


# (Ka, Kb, tied columns, P) -> (Ka, Kb, Kl, P) = (0, 0, 0, 0), (6, 6, 12, 0), (6, 6, 10, 2), (5, 5, 5, 4), (14, 0, 14, 0)
SHAPES = ((0, 0, (), 0), (6, 6, (), 0), (6, 6, (2, 3), 2), (5, 5, (0, 1, 2, 3, 4), 4), (14, 0, (), 0))
SHAPE_IDS = ["Ka%d-Kb%d-tied%d-P%d" % (s[0], s[1], len(s[2]), s[3]) for s in SHAPES]


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def pair_case(rng, B, Ka, Kb, tied, P, n, ld, ld_f):
    """tests/test_lmfit.py's sums_case twice: rows_a fp32 [B, 1 + Ka, ld], rows_b fp32 [B, 1 + Kb, ld], flux fp32 [B, ld_f], w fp64
    [B, ld_f] -- a tenth of the pixels has w = 0, star 1 holds NaN in both row blocks and in the flux there, 1e30 beyond n.  The flux
    is the mixed model at a ratio in [0.2, 0.8] times a Chebyshev series (c_0 in [0.5, 2], |c_j| <= 0.1) plus sums_case's noise; the
    trial ratio is 0.05 off it and the trial coefficients 10 %, as tests/test_lmfit_poly.py's poly_case has them.  x [n] is
    ContinuumFit's abscissa."""
    rows_a, flux, w = sums_case(rng, B, Ka, n, ld, ld_f)
    rows_b = sums_case(rng, B, Kb, n, ld, ld_f)[0]
    if B > 1:                                                         # B's NaN under A's mask, which is w's, and nowhere else
        fill = sums_case(rng, B, Kb, n, ld, ld_f)[0]
        rows_b[1] = np.where(np.isnan(rows_b[1]), np.where(np.isnan(fill[1]), np.float32(1.0), fill[1]), rows_b[1])
        rows_b[1, :, :n][:, w[1, :n] == 0.0] = np.nan
    ia, ib, Kl = maps_of(Ka, Kb, tied)
    x = abscissa_of(n)
    q_true = rng.uniform(0.2, 0.8, B)
    c_true = np.concatenate([rng.uniform(0.5, 2.0, (B, 1)), rng.uniform(-0.1, 0.1, (B, max(P - 1, 0)))], axis=1)[:, :P]
    noise = flux[:, :n].astype(np.float64) - rows_a[:, 0, :n].astype(np.float64)                    # (NaN where star 1 holds NaN)
    series = (chebvander(x, P - 1) @ c_true.T).T if P else 1.0
    flux[:, :n] = (series * ((1.0 - q_true[:, None]) * rows_a[:, 0, :n].astype(np.float64) + q_true[:, None] * rows_b[:, 0, :n].astype(np.float64)) + noise).astype(np.float32)
    q = np.clip(q_true + 0.05 * rng.normal(0, 1, B), 0.05, 0.95)
    coef = c_true * (1.0 + 0.1 * rng.normal(0, 1, (B, P)))
    return dict(rows_a=rows_a, rows_b=rows_b, flux=flux, w=w, x=x, q=q, coef=coef, n=n, Ka=Ka, Kb=Kb, Kl=Kl, P=P, B=B, ld=ld, ld_f=ld_f,
                ia=ia, ib=ib)


def pair_rows(case, q=None, coef=None, stars=None, rows_a=None, rows_b=None):
    """R [B, K + 1, n] in fp64 as lmfit_pair_core.hpp forms it (its header states the sequence), zero where w == 0."""
    n, Kl, P = case["n"], case["Kl"], case["P"]
    K = Kl + 1 + P
    stars = range(case["B"]) if stars is None else stars
    q = case["q"] if q is None else q
    coef = case["coef"] if coef is None else coef
    rows_a = case["rows_a"] if rows_a is None else rows_a
    rows_b = case["rows_b"] if rows_b is None else rows_b
    T = cheb_table(case["x"], P) if P else None                       # [n, P], the core's recurrence, exact
    out = []
    for b in stars:
        qb = float(q[b])
        omq = 1.0 - qb                                                # rounded once
        if P:
            p = np.full(n, coef[b][0])
            for k in range(1, P):
                p = fma_exact(coef[b][k], T[:, k], p)
        else:
            p = np.ones(n)
        f = case["flux"][b, :n].astype(np.float64)
        zero = np.zeros(n)
        R = []
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(K + 1):
                a = (rows_a[b, 1 + case["ia"][i], :n].astype(np.float64) if case["ia"][i] >= 0 else zero) if i < Kl else rows_a[b, 0, :n].astype(np.float64)
                c = (rows_b[b, 1 + case["ib"][i], :n].astype(np.float64) if case["ib"][i] >= 0 else zero) if i < Kl else rows_b[b, 0, :n].astype(np.float64)
                ca, cb = (-1.0, 1.0) if i == Kl else (omq, qb)
                mix = fma_exact(cb, c, ca * a)
                s = T[:, i - Kl - 1] if Kl < i < K else p
                R.append(mix * s if i < K else fma_exact(-mix, s, f))
        out.append(np.where(case["w"][b, :n][None, :] == 0.0, 0.0, np.array(R)))
    return np.array(out)


def check_pair_tiles(G, case, what, stars=None, **kw):
    """G [len(stars), 16, 16] inside the sums' bound; zero outside the (K + 1) x (K + 1) block.  Returns the largest ratio met."""
    n, K = case["n"], case["Kl"] + 1 + case["P"]
    stars = list(range(case["B"]) if stars is None else stars)
    R = pair_rows(case, stars=stars, **kw)
    ww = case["w"][stars, :n]
    want = np.einsum("bip,bjp,bp->bij", R, R, ww)
    bound = (n + 1) * EPS * np.einsum("bip,bjp,bp->bij", np.abs(R), np.abs(R), ww)
    got = G[:, :K + 1, :K + 1]
    ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print("%s Ka=%d Kb=%d Kl=%d P=%d n=%d: max |dG| / bound = %.3g" % (what, case["Ka"], case["Kb"], case["Kl"], case["P"], n, ratio))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound), (what, case["Kl"], case["P"], n, ratio)
    outside = G.copy()
    outside[:, :K + 1, :K + 1] = 0.0
    assert not outside.any()
    return ratio


def start_of(case):
    """(x0 [B, K], lo, hi): zeros for the components' parameters, the case's trial ratio and coefficients, a box that holds them."""
    Kl, P = case["Kl"], case["P"]
    x0 = np.concatenate([np.zeros((case["B"], Kl)), case["q"][:, None], case["coef"]], axis=1)
    return x0, np.concatenate([np.full(Kl, -1e6), [Q_LO], np.full(P, -1e6)]), np.concatenate([np.full(Kl, 1e6), [Q_HI], np.full(P, 1e6)])


# ---- the emulator -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_emul(tmp_path_factory):
    """tests/emul/lmfit_pair_emul.cpp built with the sanitizers as a program of its own; run(x0 [B, K], lo, hi, case, updates = [(rows_a,
    rows_b), ..], expect=0, **over) -> (state after begin, [G [B, 16, 16] per update], [state per update]).  `over` replaces entries of
    the configuration (K, Kl, P, Ka, Kb, n, ld, ia, ib; ia / ib None: no file, a null pointer) or of payne_lmfit_opts."""
    build = tmp_path_factory.mktemp("lmfit_pair_emul")
    exe = str(build / "lmfit_pair_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "lmfit_pair_emul.cpp")],
                   check=True)
    count = [0]

    def run(x0, lo, hi, case, updates=None, expect=0, **over):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        o = dict(DEFAULTS, **{k: v for k, v in over.items() if k in DEFAULTS})
        updates = [(case["rows_a"], case["rows_b"])] if updates is None else updates
        B = x0.shape[0]
        c = dict(K=x0.shape[1], Kl=case["Kl"], P=case["P"], Ka=case["Ka"], Kb=case["Kb"], n=case["n"], ld=updates[0][0].shape[2], ia=case["ia"], ib=case["ib"])
        c.update({k: v for k, v in over.items() if k in c})
        ld_f, T = case["flux"].shape[1], len(updates)
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d %d %d %d %d\n%s %d\n" % (B, c["K"], c["Kl"], c["P"], c["Ka"], c["Kb"], c["n"], c["ld"], ld_f, T,
                                                              " ".join(repr(float(o[k])) for k in ("lambda0", "down", "up", "lambda_min", "lambda_max", "xtol")), o["maxiter"]))
        for nm, a, dt in (("x0", x0, np.float64), ("lo", lo, np.float64), ("hi", hi, np.float64), ("flux", case["flux"], np.float32), ("w", case["w"], np.float64),
                          ("x", case["x"], np.float64), ("ia", c["ia"], np.int32), ("ib", c["ib"], np.int32)):
            if a is not None:
                np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        for t, (ra, rb) in enumerate(updates):
            np.ascontiguousarray(ra, dtype=np.float32).tofile(str(d / ("rowsa%d.bin" % t)))
            np.ascontiguousarray(rb, dtype=np.float32).tofile(str(d / ("rowsb%d.bin" % t)))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        if expect:
            return None
        K = c["K"]
        begin = parse_state(np.fromfile(str(d / "state_begin.bin")), B, K)
        Gs = [np.fromfile(str(d / ("G%d.bin" % t))).reshape(B, 16, 16) for t in range(T)]
        states = [parse_state(np.fromfile(str(d / ("state%d.bin" % t))), B, K) for t in range(T)]
        return begin, Gs, states
    return run


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ka,Kb,tied,P", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n", SUM_N)
def test_sums_against_einsum_on_the_host(pair_emul, Ka, Kb, tied, P, n):
    rng = np.random.default_rng(100000 * Ka + 1000 * Kb + 100 * P + n)
    case = pair_case(rng, 3, Ka, Kb, tied, P, n, n + 3, n + 6)
    K = case["Kl"] + 1 + P
    x0, lo, hi = start_of(case)
    begin, Gs, states = pair_emul(x0, lo, hi, case)
    check_pair_tiles(Gs[0], case, "emulator")
    st = states[0]                                                    # the stored matrix, gradient and chi^2 are the tile's
    assert np.array_equal(st["A"], np.triu(Gs[0][:, :K, :K]) + np.swapaxes(np.triu(Gs[0][:, :K, :K], 1), 1, 2))
    assert np.array_equal(st["g"], Gs[0][:, :K, K]) and np.array_equal(st["chisq"], Gs[0][:, K, K]) and np.all(st["niter"] == 1)
    # a NaN at a weighted pixel of either component's model reaches chi^2
    p = int(np.flatnonzero(case["w"][2, :n] > 0)[0])
    for name in ("rows_a", "rows_b"):
        bad = {name: case[name].copy()}
        bad[name][2, 0, p] = np.nan
        begin, G2, st2 = pair_emul(x0, lo, hi, dict(case, **bad))
        assert np.isnan(G2[0][2, K, K]) and st2[0]["status"][2] == NAN and np.array_equal(G2[0][:2], Gs[0][:2]) and np.all(st2[0]["status"][:2] != NAN)


# ---- 1b. the inputs of the device's comparison with the emulator ------------------------------------------------------------------
# Three updates on fresh random rows.  Random rows drive q to its bound, where one component's rows all but vanish and the scaled
# matrix of a later update can have a condition number of 1e6 (13 parameters on the 33 counting pixels of n = 37: 2e6, and two orders
# of the same sums then move the step by 5e-10 sigma).  STEP_TOL is the rounding of a well-conditioned solve, so the K = 13 shape with
# a polynomial runs at n = 1000; the test below holds every case to a quarter of STEP_TOL between two orders of the sums.
STATE_CASES = [(6, 6, (2, 3), 2, 1000), (5, 5, (0, 1, 2, 3, 4), 4, 1000), (6, 6, (), 0, 37)]
STATE_IDS = ["two-tied-P2-n1000", "all-tied-P4-n1000", "none-tied-P0-n37"]


def state_case(Ka, Kb, tied, P, n, B=3, T=3):
    """(case, [(rows_a, rows_b) per update]): pair_case, and T - 1 more draws of its rows with star 1's NaN under the first's w == 0."""
    rng = np.random.default_rng(31 * Ka + 7 * len(tied) + P + n)
    case = pair_case(rng, B, Ka, Kb, tied, P, n, n + 3, n + 6)
    updates = [(case["rows_a"], case["rows_b"])]
    for _ in range(T - 1):
        c = pair_case(rng, B, Ka, Kb, tied, P, n, n + 3, n + 6)
        for name in ("rows_a", "rows_b"):
            c[name][1] = np.where(np.isnan(c[name][1]), np.float32(1.0), c[name][1])
            c[name][1, :, :n][:, case["w"][1, :n] == 0.0] = np.nan
        updates.append((c["rows_a"], c["rows_b"]))
    return case, updates


@pytest.mark.parametrize("Ka,Kb,tied,P,n", STATE_CASES, ids=STATE_IDS)
def test_two_orders_of_the_sums_take_the_same_step(pair_emul, Ka, Kb, tied, P, n):
    """What tests/test_lmfit_pair_gpu.py may ask of the device on these inputs: after every accepted update of a running star, the step
    from numpy's einsum of the same rows (another order of the same sums, as the matrix instruction's is) lands within STEP_TOL / 4
    of the emulator's x_trial, in units of the conditional sigma (the device is a third order: twice that distance is still half the bound)."""
    from test_lmfit import damped_step
    case, updates = state_case(Ka, Kb, tied, P, n)
    Kl = case["Kl"]
    K = Kl + 1 + P
    x0, lo, hi = start_of(case)
    prev, Gs, states = pair_emul(x0, lo, hi, case, updates)
    worst, steps = 0.0, 0
    for t, st in enumerate(states):
        xt = prev["x_trial"]
        R = pair_rows(case, q=xt[:, Kl], coef=xt[:, Kl + 1:], rows_a=updates[t][0], rows_b=updates[t][1])
        G = np.einsum("bip,bjp,bp->bij", R, R, case["w"][:, :n])
        for b in range(case["B"]):
            if prev["status"][b] != RUNNING or st["status"][b] != RUNNING or not np.array_equal(st["x_best"][b], xt[b]):
                continue                                              # (skipped, finished, or rejected: the stored matrix's step)
            A, g = G[b, :K, :K], G[b, :K, K]
            want = np.clip(st["x_best"][b] + damped_step(A.copy(), g, st["lam"][b]), lo, hi)
            worst, steps = max(worst, float(np.max(np.abs(want - st["x_trial"][b]) * np.sqrt(np.diag(A))))), steps + 1
        prev = st
    print("Kl=%d P=%d n=%d: %d accepted steps, einsum's against the emulator's %.3g sigma at most" % (Kl, P, n, steps, worst))
    assert steps >= 3 and worst <= STEP_TOL / 4.0


# ---- 2. a linear model ----------------------------------------------------------------------------------------------------------
LINEAR_N = (1, 5, 37, 1000)


def linear_case(n, B=3):
    """K = 1: two models of order one, the flux their mixture at q in [0.1, 0.9] plus noise, an arbitrary trial ratio."""
    rng = np.random.default_rng(77 + n)
    case = pair_case(rng, B, 0, 0, (), 0, n, n + 3, n + 6)
    truth = rng.uniform(0.1, 0.9, B)
    mA, mB = case["rows_a"][:, 0, :n].astype(np.float64), case["rows_b"][:, 0, :n].astype(np.float64)
    with np.errstate(invalid="ignore"):
        f = (1.0 - truth[:, None]) * mA + truth[:, None] * mB + 0.01 * rng.normal(0, 1, (B, n))
    case["flux"][:, :n] = np.where(np.isnan(case["flux"][:, :n]), np.nan, f).astype(np.float32)
    case["q"] = rng.uniform(-2.0, 3.0, B)                            # any q: the box of this test is wide open
    return case


def check_linear(case, q_new, what):
    """q_new [B] against q* = sum w (f - m_A) d / sum w d^2 within the module docstring's bound."""
    n = case["n"]
    worst = 0.0
    for b in range(case["B"]):
        ok = case["w"][b, :n] != 0.0
        w = case["w"][b, :n][ok]
        mA, mB, f = (a[ok].astype(np.float64) for a in (case["rows_a"][b, 0, :n], case["rows_b"][b, 0, :n], case["flux"][b, :n]))
        d = mB - mA
        A = np.sum(w * d * d)
        q_star = np.sum(w * (f - mA) * d) / A
        q0 = case["q"][b]
        r = f - ((1.0 - q0) * mA + q0 * mB)
        bound = max(n, 16) * EPS * (np.sum(w * np.abs(d) * (np.abs(r) + np.abs(mA) + np.abs(mB) + np.abs(f))) / A + abs(q0) + abs(q_star))
        worst = max(worst, abs(q_new[b] - q_star) / bound)
        assert np.isfinite(q_new[b]) and abs(q_new[b] - q_star) <= bound, (what, n, b, q_new[b], q_star, bound)
    print("%s n=%d: |q' - q*| / bound = %.3g" % (what, n, worst))


@pytest.mark.parametrize("n", LINEAR_N)
def test_one_gauss_newton_step_solves_the_ratio(pair_emul, n):
    """K = 1 (K_l = 0, P = 0): the model is linear in q, so with lambda0 = lambda_min = 0 one update from any q lands on q*."""
    case = linear_case(n)
    begin, Gs, states = pair_emul(case["q"][:, None], np.array([-BIG]), np.array([BIG]), case, lambda0=0.0, lambda_min=0.0, xtol=0.0)
    assert np.all(states[0]["status"] == RUNNING) and np.all(states[0]["lam"] == 0.0) and np.all(states[0]["at_bound"] == 0)
    check_linear(case, states[0]["x_trial"][:, 0], "emulator")


# ---- 3. the reference loop on the mixed model -----------------------------------------------------------------------------------
BINARY_CASES = [(37, (), 0), (37, ("feh", "afe"), 2), (200, ("feh", "afe"), 2)]      # (nobs, tie, P): K = 13 in all three
BINARY_PAIRS = 4
BINARY_Q, BINARY_Q_START, BINARY_DV = 0.3, 0.4, 40.0
_BINARY = {}


def binary_inputs(g20, nobs, tie, P):
    """Stars 2 s and 2 s + 1 of recovery_case(recovery_net('synth5'), nobs) as the components of pair s: B's Vrad is A's -+ 40 km/s
    (the sign alternates with s), its Inst_R A's, a tied label A's.  The flux is the fp64 mixed model at the truth with q = 0.3, times a
    series (c_0 in [0.5, 2], |c_1| <= 0.1) with P = 2, rounded to fp32; errors of S/N 100.  The starts are the case's (10 % of the box
    off in every label) with Vrad 1 km/s off and q = 0.4.  Returns a dict: net, nntype, obs_wave, x, args (check_binary_args'),
    truth_a, truth_b, start_a, start_b [pairs, 8], q0 [pairs], flux fp32 [pairs, nobs], eflux, ctruth [pairs, P], ztruth [pairs, K]."""
    key = ("in", nobs, tie, P)
    if key not in _BINARY:
        from thepayne_amd.fitting import optfit
        from thepayne_amd.fitting.contfit import abscissa
        net, nntype = recovery_net(g20, "synth5")
        case = recovery_case(net, nobs)
        S = BINARY_PAIRS
        rng = np.random.default_rng(4242)
        ta, tb, sa, sb = (case[k][i:2 * S:2].copy() for k in ("truth", "start") for i in (0, 1))
        sign = np.where(np.arange(S) % 2 == 0, -1.0, 1.0)
        tb[:, 4], tb[:, 7] = ta[:, 4] + sign * BINARY_DV, ta[:, 7]
        sb[:, 7] = ta[:, 7]
        sa[:, 4], sb[:, 4] = ta[:, 4] + 1.0, tb[:, 4] - 1.0
        eflux = case["eflux"][:S]
        args = optfit.check_binary_args(np.ones((S, nobs)), eflux, sa, sb, nobs, len(net["xmin"]), net["xmin"], net["xmax"], ratio=BINARY_Q_START, tie=tie,
                                        fit_vrad=True, npoly=P)
        cols, Ka, b_pos = args["cols"], args["Ka"], args["b_pos"]
        for k in range(Ka):
            if b_pos[k] < Ka:                                         # tied: B has A's value
                tb[:, cols[k]] = ta[:, cols[k]]
                sb[:, cols[k]] = sa[:, cols[k]]
        x = abscissa(case["obs_wave"])
        ctruth = np.concatenate([rng.uniform(0.5, 2.0, (S, 1)), rng.uniform(-0.1, 0.1, (S, 1))], axis=1)[:, :P]
        flux = np.empty((S, nobs), dtype=np.float32)
        for s in range(S):
            mA = OracleModel(net, nntype, case["obs_wave"], ta[s], fit_vrad=True)(ta[s][cols])[0]
            mB = OracleModel(net, nntype, case["obs_wave"], tb[s], fit_vrad=True)(tb[s][cols])[0]
            p = chebvander(x, P - 1) @ ctruth[s] if P else 1.0
            flux[s] = (p * ((1.0 - BINARY_Q) * mA + BINARY_Q * mB)).astype(np.float32)
        assert np.all(np.isfinite(flux))
        free_b = [k for k in range(Ka) if b_pos[k] >= Ka]
        ztruth = np.concatenate([ta[:, cols], tb[:, [cols[k] for k in free_b]], np.full((S, 1), BINARY_Q), ctruth], axis=1)
        _BINARY[key] = dict(net=net, nntype=nntype, obs_wave=case["obs_wave"], x=x, args=args, truth_a=ta, truth_b=tb, start_a=sa, start_b=sb,
                            q0=np.full(S, BINARY_Q_START), flux=flux, eflux=eflux, ctruth=ctruth, ztruth=ztruth, nobs=nobs, P=P, tie=tie)
    return _BINARY[key]


def binary_fit(g20, s, nobs, tie, P, dtype=None):
    """lm_reference on the mixed model of two OracleModels for pair s: model = p ((1 - q) m_A + q m_B), J as payne_lmfit_update_pair
    forms its rows.  The start's coefficients are oracle_star's polynomial at the start's mixed model."""
    inp = binary_inputs(g20, nobs, tie, P)
    a = inp["args"]
    cols, Ka, Kl, ia, ib, b_pos = a["cols"], a["Ka"], a["Kl"], a["ia"], a["ib"], a["b_pos"]
    omA = OracleModel(inp["net"], inp["nntype"], inp["obs_wave"], inp["start_a"][s], fit_vrad=True, dtype=dtype)
    omB = OracleModel(inp["net"], inp["nntype"], inp["obs_wave"], inp["start_b"][s], fit_vrad=True, dtype=dtype)
    V = chebvander(inp["x"], P - 1) if P else None
    f = inp["flux"][s].astype(np.float64)
    w = 1.0 / inp["eflux"][s] ** 2
    free_b = [k for k in range(Ka) if b_pos[k] >= Ka]
    z0 = np.concatenate([inp["start_a"][s][cols], inp["start_b"][s][[cols[k] for k in free_b]], [inp["q0"][s]]])
    if P:
        q0 = inp["q0"][s]
        m0 = (1.0 - q0) * omA(z0[:Ka])[0] + q0 * omB(z0[b_pos])[0]
        o = oracle_star(inp["flux"][s], w, m0.astype(np.float32), inp["x"], P)
        assert o["status"] == 0
        z0 = np.concatenate([z0, o["coef"]])

    def fun(z):
        mA, JA = omA(z[:Ka])
        mB, JB = omB(z[b_pos])
        q = z[Kl]
        p = V @ z[Kl + 1:] if P else np.ones(nobs)
        mix = (1.0 - q) * mA + q * mB
        J = [p * ((1.0 - q) * (JA[ia[k]] if ia[k] >= 0 else 0.0) + q * (JB[ib[k]] if ib[k] >= 0 else 0.0)) for k in range(Kl)]
        J.append(p * (mB - mA))
        J.extend(mix * V[:, j] for j in range(P))
        return p * mix, np.array(J)
    return lm_reference(fun, z0, a["lo"], a["hi"], f, w)


def binary_reference(g20, nobs, tie, P):
    """The fp64 loop on every pair of binary_inputs, cached for the GPU test."""
    key = ("ref", nobs, tie, P)
    if key not in _BINARY:
        _BINARY[key] = [binary_fit(g20, s, nobs, tie, P) for s in range(BINARY_PAIRS)]
    return _BINARY[key]


@pytest.mark.parametrize("nobs,tie,P", BINARY_CASES, ids=["n%d-tie%d-P%d" % (c[0], len(c[1]), c[2]) for c in BINARY_CASES])
def test_binary_reference_loop_converges(g20, nobs, tie, P):
    """The inputs tests/test_lmfit_pair_gpu.py fits on the device: the fp64 loop on the mixed model ends CONVERGED on every pair within
    RECOVERY_MAX_EVALS evaluations and 1e-2 conditional sigma of the truth.  No pair is left out.  Measured: 4 - 5 evaluations,
    1e-3 sigma at most."""
    inp = binary_inputs(g20, nobs, tie, P)
    assert len(inp["args"]["lo"]) == 13 == inp["ztruth"].shape[1]
    for s, res in enumerate(binary_reference(g20, nobs, tie, P)):
        d = sigma_distance(res["x"], inp["ztruth"][s], res["A"]) if res["status"] == CONVERGED else np.inf
        print("nobs=%d tie=%s P=%d pair %d: status %d after %d evaluations, chi^2 %.3g, %.3g sigma from the truth" % (nobs, tie, P, s, res["status"], res["niter"], res["chisq"], d))
        assert res["status"] == CONVERGED and res["niter"] <= RECOVERY_MAX_EVALS and res["at_bound"] == 0, (nobs, tie, P, s, res["status"], res["niter"])
        assert d <= 1e-2, (nobs, tie, P, s, d)


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------
def test_fit_binary_argument_checks():
    from thepayne_amd.fitting import optfit
    xmin, xmax = synth.SPEC_LABEL_MIN, synth.SPEC_LABEL_MAX
    N, nobs = 3, 10
    flux, eflux = np.ones((N, nobs)), np.full((N, nobs), 0.01)
    start = np.tile([5000.0, 4.0, 0.0, 0.1, 10.0, 5.0, np.nan, 20000.0], (N, 1))

    def check(n_labels=4, **kw):
        return optfit.check_binary_args(flux, eflux, start, start, nobs, n_labels, xmin, xmax, **kw)
    a = check()
    assert a["Ka"] == 5 and a["Kl"] == 10 and a["P"] == 0 and len(a["lo"]) == 11 and list(a["ia"]) == [0, 1, 2, 3, 4] + [-1] * 5 and list(a["ib"]) == [-1] * 5 + [0, 1, 2, 3, 4]
    assert a["names"] == ["Teff_a", "log(g)_a", "[Fe/H]_a", "[a/Fe]_a", "Vrad_a", "Teff_b", "log(g)_b", "[Fe/H]_b", "[a/Fe]_b", "Vrad_b", "ratio"]
    assert a["lo"][10] == 0.01 and a["hi"][10] == 0.99 and np.all(a["ratio"] == 0.3) and list(a["b_pos"]) == [5, 6, 7, 8, 9]
    a = check(tie=("feh", "afe"), npoly=4, ratio=[0.2, 0.3, 0.4], bounds={"Vrad_b": (-50.0, 60.0)}, ratio_bounds=(0.1, 0.5), xtol=1e-4)
    assert a["Kl"] == 8 and len(a["lo"]) == 13 and list(a["ia"]) == [0, 1, 2, 3, 4, -1, -1, -1] and list(a["ib"]) == [-1, -1, 2, 3, -1, 0, 1, 4]
    assert a["names"] == ["Teff_a", "log(g)_a", "[Fe/H]_a", "[a/Fe]_a", "Vrad_a", "Teff_b", "log(g)_b", "Vrad_b", "ratio", "pc_0", "pc_1", "pc_2", "pc_3"]
    assert list(a["b_pos"]) == [5, 6, 2, 3, 7] and a["lo"][7] == -50.0 and a["hi"][7] == 60.0 and a["lo"][8] == 0.1 and a["opts"]["xtol"] == 1e-4
    assert np.all(a["lo"][9:] == -optfit.COEF_BOUND) and check(tie=("[Fe/H]",))["Kl"] == 9 and check(fit_vrad=False)["Kl"] == 8
    assert len(check(npoly=4)["lo"]) == 15 and len(check(n_labels=4, tie=("teff", "logg", "feh", "afe"), npoly=8)["lo"]) == 15     # a full tile
    for bad in (dict(npoly=5), dict(tie=("feh",), npoly=6),                                                  # K > 15
                dict(tie=("vmic",)), dict(tie=("Vrad",)), dict(tie=("nope",)), dict(tie=("feh", "[Fe/H]")),  # not a label of the network; twice
                dict(ratio=0.005), dict(ratio=0.995), dict(ratio=[0.3, 0.3, 1.5]), dict(ratio=np.nan), dict(ratio=0.3, ratio_bounds=(0.35, 0.9)),
                dict(ratio_bounds=(0.0, 0.9)), dict(ratio_bounds=(0.1, 1.0)), dict(ratio_bounds=(0.6, 0.4)), dict(ratio_bounds=(0.1, 0.5, 0.9)),
                dict(npoly=-1), dict(npoly=1.5), dict(npoly=True), dict(coef=np.ones((N, 2))), dict(npoly=2, coef=np.ones((N, 3))),
                dict(npoly=2, coef=np.full((N, 2), np.nan)), dict(bounds={"ratio": (0.1, 0.2)}), dict(bounds={"Vmic_a": (0.0, 1.0)}),
                dict(bounds={"Teff_b": (6000.0, 4000.0)}), dict(bounds=np.zeros((11, 2))), dict(vrad_step=0.0), dict(check_every=0), dict(maxiter=0)):
        with pytest.raises(ValueError):
            check(**bad)
    with pytest.raises(ValueError):
        optfit.check_binary_args(flux, eflux, start, start[:2], nobs, 4, xmin, xmax)
    with pytest.raises(TypeError):
        check(ftol=1e-3)
    assert "payne_lmfit_update_pair" in _lib.SYMBOLS and hasattr(optfit.LMHandle, "update_pair") and hasattr(optfit.OptFit, "fit_binary")
    doc = optfit.OptFit.fit_binary.__doc__
    assert "1 - q" in doc and "fit_joint" in doc and "narrow range" in doc and "caller's" in doc


def test_the_emulator_refuses_what_the_library_refuses(pair_emul):
    case = pair_case(np.random.default_rng(1), 2, 3, 3, (1,), 2, 37, 40, 44)                  # Kl = 5, K = 8
    x0, lo, hi = start_of(case)
    assert pair_emul(x0, lo, hi, case) is not None
    for bad in (dict(n=0), dict(n=41),                                                         # n < 1, ld < n
                dict(Kl=-1), dict(P=-1), dict(P=1), dict(Kl=4), dict(K=9), dict(K=16), dict(K=0),   # Kl + 1 + P != K; the handle's K
                dict(Ka=-1), dict(Kb=-1), dict(ia=None), dict(ib=None),                        # null maps with Kl > 0
                dict(Ka=2), dict(Kb=2),                                                        # an index beyond the block
                dict(ia=np.array([0, 1, 2, -2, -1])), dict(ib=np.array([-1, 1, -1, 0, 3])),    # below -1; Kb itself
                dict(ia=np.array([0, 1, 2, -1, -1]), ib=np.array([-1, 1, -1, -1, 2])),         # both -1 for parameter 3
                dict(lambda0=-1.0)):
        assert pair_emul(x0, lo, hi, case, expect=3, **bad) is None, bad
    wide = dict(case, rows_a=np.concatenate([case["rows_a"], case["rows_a"][:, :, :8]], axis=2), rows_b=np.concatenate([case["rows_b"], case["rows_b"][:, :, :8]], axis=2))
    assert pair_emul(x0, lo, hi, wide, expect=3, n=45) is None                                 # ld = 48 >= n = 45 > ld_f = 44
    assert pair_emul(x0, np.where(np.arange(8) == 4, -np.inf, lo), hi, case, expect=3) is None   # a box that is not finite
    # Kl == 0 takes null maps; P == 0 reads no x
    lone = pair_case(np.random.default_rng(2), 2, 0, 0, (), 0, 37, 40, 44)
    x1, lo1, hi1 = start_of(lone)
    assert pair_emul(x1, lo1, hi1, dict(lone, x=None), ia=None, ib=None) is not None
