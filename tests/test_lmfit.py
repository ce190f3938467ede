"""Batched Levenberg-Marquardt (payne_lmfit_*, thepayne_amd/fitting/optfit.py) -- what runs without a GPU: the kernel's arithmetic
(csrc/lmfit_core.hpp) executed on the host under ASan / UBSan (tests/emul/lmfit_emul.cpp) against numpy, the state machine on
scripted inputs, the fp64 reference loop the GPU tests compare with (and that it converges on the inputs those tests use), and
OptFit's argument checks.  The kernels themselves: tests/test_lmfit_gpu.py, which shares the helpers defined here.

Bounds.  The sums: |G - einsum| <= n 2^-52 sum|a_i a_j w| on the same fp32 rows, the bound tests/test_specjac_gpu.py states for the
Fisher matrices.  A step: 1e-10 of each parameter's conditional sigma 1 / sqrt(A_kk) -- fp64 rounding of a K <= 15 Cholesky
factorisation of a matrix with a unit diagonal."""
import os
import subprocess

import numpy as np
import pytest

from thepayne_amd import _lib, synth
from test_specjac import jac_numpy64, synth_layers, torch_jac, encode32
from test_trainspec import G20, g20_net, names_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(lambda0=1e-3, down=10.0, up=10.0, lambda_min=1e-12, lambda_max=1e8, xtol=1e-3, maxiter=50)
RUNNING, CONVERGED, STALLED, MAXITER, SINGULAR, NAN = range(6)
STEP_TOL = 1e-10                                     # of a parameter's conditional sigma
SUM_N, SUM_K = (1, 5, 37, 1000), (1, 4, 5, 15)


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_trainspec")


# ---- the sums' reference ------------------------------------------------------------------------------------------------------
def sums_case(rng, B, K, n, ld, ld_f):
    """Random rows fp32 [B, 1 + K, ld], flux fp32 [B, ld_f], w fp64 [B, ld_f]; beyond n the arrays hold 1e30.  A tenth of the pixels
    has zero weight (n > 1), and star 1 holds NaN in every row and in the flux there."""
    rows = np.full((B, 1 + K, ld), np.float32(1e30))
    rows[:, 1:, :n] = (rng.normal(0, 1, (B, K, n)) * 10.0 ** rng.uniform(-4, 0, (1, K, 1))).astype(np.float32)
    rows[:, 0, :n] = (1.0 + 0.1 * rng.normal(0, 1, (B, n))).astype(np.float32)
    flux = np.full((B, ld_f), np.float32(1e30))
    flux[:, :n] = rows[:, 0, :n] + (0.01 * rng.normal(0, 1, (B, n))).astype(np.float32)
    w = np.full((B, ld_f), 1e30)
    w[:, :n] = 1.0 / rng.uniform(0.005, 0.05, (B, n)) ** 2
    if n > 1:
        zero = rng.uniform(size=(B, n)) < 0.1
        zero[:, 0] = False
        w[:, :n][zero] = 0.0
        if B > 1:
            rows[1, :, :n][:, zero[1]] = np.nan
            flux[1, :n][zero[1]] = np.nan
    return rows.astype(np.float32), flux.astype(np.float32), w


def einsum_tile(rows, flux, w, n):
    """(G [B, K + 1, K + 1] by numpy.einsum in fp64 on the same fp32 values, the bound n 2^-52 sum|a_i a_j w|)."""
    R = np.concatenate([rows[:, 1:, :n].astype(np.float64), (flux[:, :n].astype(np.float64) - rows[:, 0, :n].astype(np.float64))[:, None, :]], axis=1)
    ww = w[:, :n]
    R = np.where(ww[:, None, :] == 0.0, 0.0, R)
    return np.einsum("bip,bjp,bp->bij", R, R, ww), n * 2.0 ** -52 * np.einsum("bip,bjp,bp->bij", np.abs(R), np.abs(R), ww)


def check_tiles(G, rows, flux, w, n, K, what):
    """G [B, 16, 16] inside the bound; zero outside the (K + 1) x (K + 1) block."""
    want, bound = einsum_tile(rows, flux, w, n)
    got = G[:, :K + 1, :K + 1]
    ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print("%s K=%d n=%d: max |dG| / bound = %.3g" % (what, K, n, ratio))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound), (what, K, n, ratio)
    outside = G.copy()
    outside[:, :K + 1, :K + 1] = 0.0
    assert not outside.any()


# ---- the per-star step in numpy -----------------------------------------------------------------------------------------------
def damped_step(A, g, lam):
    """delta of (S A S + lambda I) u = S g, delta = S u; None where the library says SINGULAR."""
    d = np.diag(A)
    if not np.all(np.isfinite(d)) or np.any(d <= 0.0):
        return None
    s = 1.0 / np.sqrt(d)
    M = A * np.outer(s, s)
    M[np.diag_indices_from(M)] = 1.0 + lam
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None
    u = np.linalg.solve(L.T, np.linalg.solve(L, g * s)) * s
    return u if np.all(np.isfinite(u)) else None


def lm_reference(fun, x0, lo, hi, flux, w, **opts):
    """The library's algorithm for one star in numpy fp64 (include/payne_hip.h states it).  fun(x) -> (model [n], J [K, n]).
    Returns dict(x, chisq, A, status, niter, at_bound, lam)."""
    o = dict(DEFAULTS, **opts)
    K = len(x0)
    xt = np.clip(np.asarray(x0, dtype=np.float64), lo, hi)
    xb, A, g, chisq, lam, niter, mask = xt.copy(), None, None, np.nan, o["lambda0"], 0, 0
    ok = w != 0.0
    while True:
        model, J = fun(xt)
        r = np.where(ok, flux - model, 0.0)
        Jm = np.where(ok[None, :], J, 0.0)
        c_t = float(np.sum(w * r * r))
        first = niter == 0
        niter += 1
        if first and not np.isfinite(c_t):
            return dict(x=xb, chisq=c_t, A=A, status=NAN, niter=niter, at_bound=mask, lam=lam)
        accept = first or (np.isfinite(c_t) and c_t <= chisq)
        tried = lam
        if accept:
            xb, A, g, chisq = xt.copy(), (Jm * w) @ Jm.T, (Jm * w) @ r, c_t
            lam = max(lam / o["down"], o["lambda_min"])
        else:
            lam = min(lam * o["up"], o["lambda_max"])
        delta = damped_step(A, g, lam)
        status = RUNNING
        if delta is None:
            status = SINGULAR
        else:
            xt = np.clip(xb + delta, lo, hi)
            mask = int(sum(1 << k for k in range(K) if xt[k] != xb[k] + delta[k]))
            dmax = float(np.max(np.abs(xt - xb) * np.sqrt(np.diag(A))))
            if accept and dmax < o["xtol"]:
                status = CONVERGED
            elif not accept and tried >= o["lambda_max"]:
                status = STALLED
            elif niter >= o["maxiter"]:
                status = MAXITER
        if status != RUNNING:
            return dict(x=xb, chisq=chisq, A=A, status=status, niter=niter, at_bound=mask, lam=lam)


# ---- the emulator -------------------------------------------------------------------------------------------------------------
def parse_state(a, B, K):
    a = a.reshape(B, 3 * K + K * K + 5)
    o = 3 * K + K * K
    return dict(x_best=a[:, :K], x_trial=a[:, K:2 * K], A=a[:, 2 * K:2 * K + K * K].reshape(B, K, K), g=a[:, 2 * K + K * K:o], chisq=a[:, o],
                lam=a[:, o + 1], status=a[:, o + 2].astype(int), niter=a[:, o + 3].astype(int), at_bound=a[:, o + 4].astype(np.int64))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/lmfit_emul.cpp built with the sanitizers; run(x0, lo, hi, flux, w, rows_per_update, n, opts) -> (state after
    begin, [G [B, 16, 16] per update], [state per update])."""
    build = tmp_path_factory.mktemp("lmfit_emul")
    exe = str(build / "lmfit_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "lmfit_emul.cpp")],
                   check=True)
    count = [0]

    def run(x0, lo, hi, flux, w, rows_per_update, n, **opts):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        o = dict(DEFAULTS, **opts)
        B, K = x0.shape
        ld, ld_f, T = rows_per_update[0].shape[2], flux.shape[1], len(rows_per_update)
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d\n%s %d\n" % (B, K, n, ld, ld_f, T, " ".join(repr(float(o[k])) for k in ("lambda0", "down", "up", "lambda_min", "lambda_max", "xtol")),
                                                  o["maxiter"]))
        for nm, a, dt in (("x0", x0, np.float64), ("lo", lo, np.float64), ("hi", hi, np.float64), ("flux", flux, np.float32), ("w", w, np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        for t, r in enumerate(rows_per_update):
            assert r.shape == (B, 1 + K, ld)
            np.ascontiguousarray(r, dtype=np.float32).tofile(str(d / ("rows%d.bin" % t)))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        begin = parse_state(np.fromfile(str(d / "state_begin.bin")), B, K)
        Gs = [np.fromfile(str(d / ("G%d.bin" % t))).reshape(B, 16, 16) for t in range(T)]
        states = [parse_state(np.fromfile(str(d / ("state%d.bin" % t))), B, K) for t in range(T)]
        return begin, Gs, states
    return run


# ---- scripted inputs of the state machine ---------------------------------------------------------------------------------------
class Script(object):
    """One star whose chi^2 sequence is written down: the K derivative rows J are constant, the residual of update t is c[t] * r with
    r = J^T a + a little that J does not span, so that chi^2 = c^2 sum w r^2 and the step is about c * a.  a_k sqrt(A_kk) is 5: far
    above xtol; the chi^2 ratios between updates are far from one.  c = NaN puts NaN into the model at one weighted pixel."""

    K, n, ld, ld_f = 3, 37, 40, 44

    def __init__(self, name, c, expect, x0=(0.0, 0.0, 0.0), lo=(-1e3, -1e3, -1e3), hi=(1e3, 1e3, 1e3), a_sign=(1, 1, 1), zero_row=None, **opts):
        self.name, self.c, self.expect, self.opts = name, list(c), expect, opts
        rng = np.random.default_rng(2024)
        K, n = self.K, self.n
        self.x0, self.lo, self.hi = np.array([x0], dtype=np.float64), np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        J = (rng.normal(0, 1, (K, n)) * np.array([[1.0], [1e-2], [1e-3]])).astype(np.float32)
        if zero_row is not None:
            J[zero_row] = 0.0
        w = 1.0 / rng.uniform(0.005, 0.05, n) ** 2
        w[[5, 20]] = 0.0
        Akk = np.maximum(np.einsum("kp,kp,p->k", J.astype(np.float64), J.astype(np.float64), w), 1e-300)
        a = 5.0 * np.array(a_sign) / np.sqrt(Akk)
        if zero_row is not None:
            a[zero_row] = 0.0
        r = a @ J.astype(np.float64) + 1e-3 * rng.normal(0, 1, n) / np.sqrt(np.where(w > 0, w, 1.0))
        self.flux = np.full((1, self.ld_f), np.float32(1e30))
        self.flux[0, :n] = (1.0 + 0.1 * rng.normal(0, 1, n)).astype(np.float32)
        self.w = np.full((1, self.ld_f), 1e30)
        self.w[0, :n] = w
        self.rows = []
        for c in self.c:
            rows = np.full((1, 1 + K, self.ld), np.float32(1e30))
            rows[0, 1:, :n] = J
            rows[0, 0, :n] = (self.flux[0, :n].astype(np.float64) - (0.0 if np.isnan(c) else c) * r).astype(np.float32)
            if np.isnan(c):
                rows[0, 0, 7] = np.nan
            rows[0, :, [5, 20]] = np.nan                              # zero weight: whatever the rows hold
            self.rows.append(rows)

    def run(self, emul):
        return emul(self.x0, self.lo, self.hi, self.flux, self.w, self.rows, self.n, **self.opts)


def scripts():
    """expect: per update (status, lambda, at_bound, niter); None = the star is finished and nothing may change."""
    l0 = DEFAULTS["lambda0"]
    d1 = l0 / 10.0                                                  # (the library's own operations, so that the bits agree)
    d2, d3 = d1 / 10.0, d1 / 10.0 / 10.0
    return [
        Script("accept reject accept", [1.0, 2.0, 0.5, 0.25], [(RUNNING, d1, 0, 1), (RUNNING, d1 * 10.0, 0, 2), (RUNNING, d1 * 10.0 / 10.0, 0, 3),
                                                              (RUNNING, d1 * 10.0 / 10.0 / 10.0, 0, 4)]),
        Script("clipping", [1.0, 0.5], [(RUNNING, d1, 0b101, 1), (RUNNING, d2, 0b101, 2)], a_sign=(1, 1, -1), lo=(-1e3, -1e3, -1e-9), hi=(1e-9, 1e3, 1e3)),
        Script("begin clips", [1e-7], [(CONVERGED, d1, 0, 1)], x0=(7.0, 0.0, -7.0), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), a_sign=(-1, 1, 1)),
        Script("maxiter", [1.0, 0.9, 0.8, 0.7, 0.6], [(RUNNING, d1, 0, 1), (RUNNING, d2, 0, 2), (MAXITER, d3, 0, 3), None, None], maxiter=3),
        Script("stalled", [1.0, 2.0, 3.0, 4.0, 0.1], [(RUNNING, 1e7 / 10.0, 0, 1), (RUNNING, 1e7 / 10.0 * 10.0, 0, 2), (RUNNING, 1e8, 0, 3), (STALLED, 1e8, 0, 4), None],
               lambda0=1e7, xtol=0.0),                                   # (with lambda this large every step is below the default xtol)
        Script("NaN at the first evaluation", [np.nan, 1.0], [(NAN, l0, 0, 1), None]),
        Script("NaN later is a rejection", [1.0, np.nan, 0.5], [(RUNNING, d1, 0, 1), (RUNNING, d1 * 10.0, 0, 2), (RUNNING, d1 * 10.0 / 10.0, 0, 3)]),
        Script("singular", [1.0, 0.5], [(SINGULAR, d1, 0, 1), None], zero_row=1),
        Script("converged", [1e-7, 1.0], [(CONVERGED, d1, 0, 1), None]),
        Script("Gauss-Newton", [1.0, 2.0, 0.5], [(RUNNING, 0.0, 0, 1), (RUNNING, 0.0, 0, 2), (RUNNING, 0.0, 0, 3)], lambda0=0.0, lambda_min=0.0),
    ]


def check_script(sc, begin, states, what):
    """The statuses, lambda, at_bound and niter as written down (exactly); x_trial against numpy's solve of the stored matrix."""
    assert begin["status"][0] == RUNNING and begin["niter"][0] == 0 and begin["lam"][0] == dict(DEFAULTS, **sc.opts)["lambda0"]
    assert np.array_equal(begin["x_trial"][0], np.clip(sc.x0[0], sc.lo, sc.hi))
    assert begin["at_bound"][0] == sum(1 << k for k in range(sc.K) if not sc.lo[k] <= sc.x0[0, k] <= sc.hi[k])
    prev = begin
    for t, (exp, st) in enumerate(zip(sc.expect, states)):
        if exp is None:
            for key in st:
                assert np.array_equal(st[key], prev[key], equal_nan=True), (what, sc.name, t, key)
            continue
        status, lam, mask, niter = exp
        got = (int(st["status"][0]), float(st["lam"][0]), int(st["at_bound"][0]), int(st["niter"][0]))
        assert got == (status, lam, mask, niter), (what, sc.name, t, got, exp)
        if status in (RUNNING, CONVERGED, MAXITER, STALLED):
            A, g, xb = st["A"][0], st["g"][0], st["x_best"][0]
            delta = damped_step(A, g, lam)
            want = xb if status != RUNNING else np.clip(xb + delta, sc.lo, sc.hi)
            assert np.all(np.abs(st["x_trial"][0] - want) * np.sqrt(np.diag(A)) <= STEP_TOL), (what, sc.name, t)
            assert np.array_equal(A, A.T)
        else:
            assert np.array_equal(st["x_trial"][0], st["x_best"][0])
        prev = st


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SUM_K)
@pytest.mark.parametrize("n", SUM_N)
def test_sums_against_einsum_on_the_host(emul, K, n):
    rng = np.random.default_rng(100 * K + n)
    B, ld, ld_f = 3, n + 3, n + 6
    rows, flux, w = sums_case(rng, B, K, n, ld, ld_f)
    x0, lo, hi = np.zeros((B, K)), np.full(K, -1.0), np.full(K, 1.0)
    begin, Gs, states = emul(x0, lo, hi, flux, w, [rows], n)
    check_tiles(Gs[0], rows, flux, w, n, K, "emulator")
    # the stored matrix, gradient and chi^2 are the tile's
    st = states[0]
    assert np.array_equal(st["A"], np.triu(Gs[0][:, :K, :K]) + np.swapaxes(np.triu(Gs[0][:, :K, :K], 1), 1, 2))
    assert np.array_equal(st["g"], Gs[0][:, :K, K]) and np.array_equal(st["chisq"], Gs[0][:, K, K])
    # a NaN at a weighted pixel reaches chi^2
    p = int(np.flatnonzero(w[2, :n] > 0)[0])
    rows2 = rows.copy()
    rows2[2, 0, p] = np.nan
    begin, G2, st2 = emul(x0, lo, hi, flux, w, [rows2], n)
    assert np.isnan(G2[0][2, K, K]) and st2[0]["status"][2] == NAN and np.array_equal(G2[0][:2], Gs[0][:2]) and np.all(st2[0]["status"][:2] != NAN)


# ---- 2. a linear model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n", [(1, 5), (4, 37), (5, 1000), (15, 37), (15, 1000)])
def test_one_gauss_newton_step_solves_a_linear_model(emul, K, n):
    """The rows are constant and the model is their combination: with lambda0 = lambda_min = 0 one update lands on lstsq's solution."""
    rng = np.random.default_rng(7 * K + n)
    B, ld = 2, n + 3
    J = (rng.normal(0, 1, (B, K, n)) * 10.0 ** rng.uniform(-4, 0, (1, K, 1))).astype(np.float32)
    w = 1.0 / rng.uniform(0.005, 0.05, (B, n)) ** 2
    sig = 1.0 / np.sqrt(np.einsum("bkp,bkp,bp->bk", J.astype(np.float64), J.astype(np.float64), w))
    x_true = rng.normal(0, 1, (B, K)) * sig * 100.0
    x0 = x_true + rng.normal(0, 1, (B, K)) * sig * 30.0
    flux = np.einsum("bk,bkp->bp", x_true, J.astype(np.float64)).astype(np.float32)
    rows = np.zeros((B, 1 + K, ld), dtype=np.float32)
    rows[:, 1:, :n] = J
    rows[:, 0, :n] = np.einsum("bk,bkp->bp", x0, J.astype(np.float64)).astype(np.float32)
    big = 1e30 * np.maximum(np.abs(x0).max(), 1.0)
    begin, Gs, states = emul(x0, np.full(K, -big), np.full(K, big), flux, w, [rows], n, lambda0=0.0, lambda_min=0.0, xtol=0.0)
    for b in range(B):
        r = flux[b].astype(np.float64) - rows[b, 0, :n].astype(np.float64)
        Js = J[b].astype(np.float64) * sig[b][:, None]                  # columns in units of sigma: lstsq sees a well-scaled matrix
        u = np.linalg.lstsq((Js * np.sqrt(w[b])).T, r * np.sqrt(w[b]), rcond=None)[0]
        err = np.abs(states[0]["x_trial"][b] - (x0[b] + u * sig[b])) / sig[b]
        print("K=%d n=%d star %d: |x_trial - lstsq| = %.3g sigma at most" % (K, n, b, err.max()))
        assert err.max() <= STEP_TOL and states[0]["status"][b] == RUNNING and states[0]["lam"][b] == 0.0


# ---- 3. the state machine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", scripts(), ids=lambda s: s.name.replace(" ", "_"))
def test_state_machine_on_scripted_inputs(emul, sc):
    begin, Gs, states = sc.run(emul)
    check_script(sc, begin, states, "emulator")
    for t, exp in enumerate(sc.expect):
        if exp is None:
            assert not Gs[t].any()                                    # the workgroup of a finished star returns at once


def test_reference_loop_walks_the_scripted_sequence():
    """The numpy loop the GPU tests compare with takes the emulator's decisions: a quadratic model, from a start far enough for a
    rejection or two, ends CONVERGED at the truth; a truth outside the box ends on the bound with its bit set (the clipped step is
    not the constrained optimum's, so the free parameters creep there under a growing lambda and the status may be MAXITER)."""
    rng = np.random.default_rng(5)
    K, n = 3, 60
    Jc = rng.normal(0, 1, (K, n))
    Q = 0.3 * rng.normal(0, 1, (K, K, n))
    w = np.full(n, 1e4)

    def fun(x):
        return 1.0 + x @ Jc + np.einsum("i,j,ijp->p", x, x, Q), Jc + 2.0 * np.einsum("j,ijp->ip", x, Q)
    truth = np.array([0.2, -0.1, 0.3])
    flux = fun(truth)[0]
    res = lm_reference(fun, np.zeros(K), np.full(K, -1.0), np.full(K, 1.0), flux, w)
    assert res["status"] == CONVERGED and res["at_bound"] == 0 and np.max(np.abs(res["x"] - truth) * np.sqrt(np.diag(res["A"]))) <= 1e-2
    res = lm_reference(fun, np.zeros(K), np.full(K, -1.0), np.array([1.0, 1.0, 0.25]), flux, w)
    print("truth outside the box: status %d after %d evaluations" % (res["status"], res["niter"]))
    assert res["status"] in (CONVERGED, STALLED, MAXITER) and res["at_bound"] == 0b100 and res["x"][2] == 0.25


# ---- 4. the recovery tests' inputs ----------------------------------------------------------------------------------------------
FIVE_MIN, FIVE_MAX = np.append(synth.SPEC_LABEL_MIN, 0.5), np.append(synth.SPEC_LABEL_MAX, 2.5)
RECOVERY_BMAX = 16
RECOVERY_N = RECOVERY_BMAX + 5
SNR = 100.0


def g20_spec_net(g20, name):
    """The fixture's network as a state dict ``nnio`` reads (synth.make_torch_net's keys) on a model grid of its own."""
    layers, x, t = g20_net(g20, name)
    D, npix = layers[0][0].shape[1], layers[-1][0].shape[0]
    wave, Rsig = synth.ann_wavelength(npix, 5150.0, 32000.0)
    net = {"kind": G20[name], "xmin": FIVE_MIN[:D].copy(), "xmax": FIVE_MAX[:D].copy(), "wavelength": wave, "resolution": float(Rsig)}
    for nm, (W, b) in zip(names_of(G20[name]), layers):
        net[nm + ".weight"], net[nm + ".bias"] = np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return net


def recovery_net(g20, which):
    """(net, nntype): the g20 fixture's SMLP and LinNet, and a five-label synth network (its output layer's weights times 30, so that
    S/N 100 constrains the labels to a fraction of the box)."""
    if which in G20:
        return g20_spec_net(g20, which), G20[which]
    net = synth.make_torch_net("LinNet", npix=512, H=(16, 16, 16), seed=31, D=5)
    net["xmin"], net["xmax"] = FIVE_MIN.copy(), FIVE_MAX.copy()
    net["lin6.weight"] = (30.0 * net["lin6.weight"]).astype(np.float32)
    return net, "LinNet"


def recovery_case(net, nobs, seed=0, N=RECOVERY_N):
    """Truths in the inner half of the box, starts 10 % of the box off them, each star with its own Vrad / Vrot / inst_R; errors of
    S/N 100 on a flux of order one; the observed grid is the inner 60 % of the model's range (|Vrad| <= 5 km/s keeps it inside).
    Returns dict(obs_wave, truth [N, 8], start [N, 8], eflux [N, nobs], cols)."""
    rng = np.random.default_rng(1000 + seed)
    D = len(net["xmin"])
    span = net["xmax"] - net["xmin"]
    cols = [0, 1, 2, 3] + ([6] if D == 5 else [])
    truth = np.full((N, 8), np.nan)
    truth[:, cols] = net["xmin"] + (0.5 + rng.uniform(-0.25, 0.25, (N, D))) * span
    truth[:, 4], truth[:, 5], truth[:, 7] = rng.uniform(-5, 5, N), rng.uniform(3, 30, N), rng.uniform(15000.0, 30000.0, N)
    start = truth.copy()
    start[:, cols] += 0.1 * span * rng.choice([-1.0, 1.0], (N, D))
    wave = net["wavelength"]
    width = wave[-1] - wave[0]
    return dict(obs_wave=np.linspace(wave[0] + 0.2 * width, wave[-1] - 0.2 * width, nobs), truth=truth, start=start,
                eflux=np.full((N, nobs), 1.0 / SNR), cols=cols)


class OracleModel(object):
    """The model OptFit minimises, in fp64 on the host: the network and its Jacobian (tests/test_specjac.py: numpy fp64, or torch's
    CPU jvp in `dtype`), pushed through the numpy oracle's getspec chain at the star's Vrad / Vrot / inst_R, as
    test_getgrad_against_the_oracle_chain builds it.  With `fit_vrad` the last parameter is Vrad and its row the central difference
    of the chain at Vrad +- vrad_step."""

    def __init__(self, net, nntype, obs_wave, fixed, fit_vrad=False, vrad_step=0.25, dtype=None):
        self.net, self.nntype, self.obs_wave, self.fixed = net, nntype, np.asarray(obs_wave, dtype=np.float64), fixed
        self.layers = synth_layers(net, nntype)
        self.fit_vrad, self.h, self.dtype = fit_vrad, vrad_step, dtype
        self.D = len(net["xmin"])

    def chain(self, spec, vrad):
        import oracle.payne_oracle as PO
        old = PO.ann_forward
        PO.ann_forward = lambda net_, labels: np.array(spec, dtype=np.float64)
        try:
            return PO.getspec(self.net, rot_vel=float(self.fixed[5]), rad_vel=float(vrad), inst_R=float(self.fixed[7]), outwave=self.obs_wave)[1]
        finally:
            PO.ann_forward = old

    def __call__(self, x):
        D = self.D
        span = self.net["xmax"] - self.net["xmin"]
        if self.dtype is None:
            e = ((x[:D] - self.net["xmin"]) / span - 0.5)[None, :]
            y, J, _ = jac_numpy64(self.layers, self.nntype, e)
        else:
            y, J = torch_jac(self.layers, self.nntype, encode32(x[None, :D], self.net["xmin"], self.net["xmax"]), self.dtype)
            y, J = y.astype(np.float64), J.astype(np.float64)
        vrad = x[D] if self.fit_vrad else self.fixed[4]
        rows = [self.chain(J[0, k] / span[k], vrad) for k in range(D)]
        if self.fit_vrad:
            rows.append((self.chain(y[0], vrad + self.h) - self.chain(y[0], vrad - self.h)) / (2.0 * self.h))
        return self.chain(y[0], vrad), np.array(rows)


def reference_fit(net, nntype, case, flux, star, fit_vrad=False, start=None, dtype=None, **opts):
    """lm_reference for one star of a recovery case on `flux` [nobs]."""
    D = len(net["xmin"])
    cols = case["cols"] + ([4] if fit_vrad else [])
    lo = np.concatenate([net["xmin"], [-500.0] if fit_vrad else []])
    hi = np.concatenate([net["xmax"], [500.0] if fit_vrad else []])
    fixed = case["start"][star]
    model = OracleModel(net, nntype, case["obs_wave"], fixed, fit_vrad=fit_vrad, dtype=dtype)
    e = case["eflux"][star]
    w = np.where(np.isfinite(e) & (e != 0) & np.isfinite(flux), 1.0 / e ** 2, 0.0)
    x0 = case["start"][star][cols] if start is None else start
    return lm_reference(model, x0, lo, hi, np.where(np.isfinite(flux), flux, 0.0), w, **opts), model


def sigma_distance(x, x_ref, F):
    return float(np.max(np.abs(np.asarray(x) - np.asarray(x_ref)) * np.sqrt(np.diag(F))))


RECOVERY_MAX_EVALS = 12
_RECOVERY = {}


def recovery_inputs(g20, which, nobs, fit_vrad):
    """(net, nntype, case of RECOVERY_N stars, the fp64 loop's results): the first stars of a pool of 3 RECOVERY_N on which the fp64
    reference loop, on the oracle's spectrum at the truth, ends CONVERGED within RECOVERY_MAX_EVALS evaluations and 10 xtol sigma of
    the truth.  (A start 10 % of the box off can lie in the basin of another minimum of a random leaky network; what is left out is
    decided by the reference alone.)"""
    key = (which, nobs, fit_vrad)
    if key not in _RECOVERY:
        net, nntype = recovery_net(g20, which)
        pool = recovery_case(net, nobs, N=3 * RECOVERY_N)
        cols = pool["cols"] + ([4] if fit_vrad else [])
        keep, results = [], []
        for star in range(3 * RECOVERY_N):
            truth = pool["truth"][star]
            flux = OracleModel(net, nntype, pool["obs_wave"], truth, fit_vrad=fit_vrad)(truth[cols])[0]
            assert np.all(np.isfinite(flux))
            res, _ = reference_fit(net, nntype, pool, flux, star, fit_vrad=fit_vrad)
            res["d"] = sigma_distance(res["x"], truth[cols], res["A"]) if res["status"] == CONVERGED else np.inf
            if res["status"] == CONVERGED and res["niter"] <= RECOVERY_MAX_EVALS and res["d"] <= 10.0 * DEFAULTS["xtol"]:
                keep.append(star)
                results.append(res)
            if len(keep) == RECOVERY_N:
                break
        assert len(keep) == RECOVERY_N, (key, len(keep))
        case = dict(pool, truth=pool["truth"][keep], start=pool["start"][keep], eflux=pool["eflux"][keep])
        _RECOVERY[key] = (net, nntype, case, results)
    return _RECOVERY[key]


@pytest.mark.parametrize("fit_vrad", (False, True), ids=("labels", "labels+vrad"))
@pytest.mark.parametrize("nobs", (37, 1000))
@pytest.mark.parametrize("which", ("smlp", "linnet", "synth5"))
def test_reference_loop_converges_on_the_recovery_inputs(g20, which, nobs, fit_vrad):
    """The inputs tests/test_lmfit_gpu.py recovers on the device: the fp64 loop ends CONVERGED on every star, at the truth."""
    net, nntype, case, results = recovery_inputs(g20, which, nobs, fit_vrad)
    assert len(results) == RECOVERY_N == len(case["truth"])
    for star, res in enumerate(results):
        assert res["status"] == CONVERGED and res["niter"] <= DEFAULTS["maxiter"] and res["d"] <= 10.0 * DEFAULTS["xtol"], (which, nobs, star)
    sig = np.array([1.0 / np.sqrt(np.diag(r["A"])) for r in results])
    box = np.concatenate([net["xmax"] - net["xmin"], [1000.0] if fit_vrad else []])
    print("%s nobs=%d fit_vrad=%s: evaluations %s; worst distance %.3g sigma; sigma / box between %.3g and %.3g"
          % (which, nobs, fit_vrad, [r["niter"] for r in results], max(r["d"] for r in results), (sig / box).min(), (sig / box).max()))


# ---- 5. OptFit's argument checks ------------------------------------------------------------------------------------------------
def test_optfit_argument_checks():
    from thepayne_amd.fitting import optfit
    xmin, xmax = synth.SPEC_LABEL_MIN, synth.SPEC_LABEL_MAX
    N, nobs = 3, 10
    flux, eflux = np.ones((N, nobs)), np.full((N, nobs), 0.01)
    start = np.tile([5000.0, 4.0, 0.0, 0.1, 10.0, 5.0, np.nan, 20000.0], (N, 1))

    def check(flux=flux, eflux=eflux, start=start, n_labels=4, **kw):
        return optfit.check_fit_args(flux, eflux, start, nobs, n_labels, xmin, xmax, **kw)
    f, e, s, lo, hi, o = check()
    assert f.dtype == np.float32 and e.dtype == np.float64 and np.array_equal(lo, xmin) and np.array_equal(hi, xmax) and o == optfit.LM_DEFAULTS
    assert o == DEFAULTS and _lib.LmfitOpts().maxiter == 50 and _lib.LmfitOpts().lambda_max == 1e8
    f, e, s, lo, hi, o = check(fit_vrad=True, bounds={"Vrad": (-50.0, 60.0), "Teff": (4000.0, 6000.0)}, xtol=1e-4)
    assert lo[4] == -50.0 and hi[4] == 60.0 and lo[0] == 4000.0 and hi[1] == xmax[1] and o["xtol"] == 1e-4
    assert check(fit_vrad=True)[3][4] == -optfit.VRAD_BOUND
    assert np.array_equal(check(bounds=np.stack([xmin + 0.1, xmax - 0.1], axis=1))[3], xmin + 0.1)
    for bad in (dict(flux=np.ones((N, nobs + 1))), dict(eflux=np.ones((N + 1, nobs))), dict(start=start[:, :7]), dict(start=start[:2]),
                dict(start=np.where(np.arange(8) == 1, np.nan, start)), dict(start=np.where(np.arange(8) == 5, np.nan, start)),
                dict(start=np.where(np.arange(8) == 4, np.nan, start)), dict(n_labels=5),
                dict(bounds={"Vrad": (-1.0, 1.0)}), dict(bounds={"Teff": (6000.0, 4000.0)}), dict(bounds=np.zeros((3, 2))),
                dict(bounds={"Teff": (4000.0, np.inf)}), dict(vrad_step=0.0), dict(check_every=0), dict(maxiter=0), dict(lambda0=-1.0),
                dict(lambda_min=1.0, lambda_max=0.5), dict(down=0.5), dict(up=0.5), dict(xtol=-1.0), dict(xtol=np.nan), dict(lambda0=1e9)):
        with pytest.raises(ValueError):
            check(**bad)
    with pytest.raises(TypeError):
        check(ftol=1e-3)
    assert optfit.fitted_columns(4, False) == [0, 1, 2, 3] and optfit.fitted_columns(5, True) == [0, 1, 2, 3, 6, 4]
    # what is not linear is refused before anything touches the device
    with pytest.raises(NotImplementedError):
        optfit.OptFit("net.npz", "SMLP", np.linspace(5200.0, 5201.0, nobs), Cnnpath="cont.npz")
    F = object.__new__(optfit.OptFit)
    with pytest.raises(NotImplementedError):
        F.fit(flux, eflux, start, lsf=np.full(nobs, 0.1))
    assert all(s in _lib.SYMBOLS for s in ("payne_lmfit_create", "payne_lmfit_begin", "payne_lmfit_trial", "payne_lmfit_update", "payne_lmfit_result", "payne_lmfit_destroy"))
    assert (_lib.LMFIT_RUNNING, _lib.LMFIT_CONVERGED, _lib.LMFIT_STALLED, _lib.LMFIT_MAXITER, _lib.LMFIT_SINGULAR, _lib.LMFIT_NAN) == tuple(range(6))
