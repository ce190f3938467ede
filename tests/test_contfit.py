"""Continuum polynomials for many stars (payne_contfit_batch, thepayne_amd/fitting/contfit.py) -- what runs without a GPU: the
kernel's arithmetic (csrc/contfit_core.hpp) executed on the host under ASan / UBSan (tests/emul/contfit_emul.cpp) against a numpy fp64
oracle (numpy.linalg.lstsq on sqrt(w) [m T_j], chebvander, plus the clipping loop), the statuses, the argument checks, and the fp64
reference of OptFit.fit_with_continuum's alternation (and that it recovers the truth on the inputs the GPU test uses).  The kernel
itself: tests/test_contfit_gpu.py, which shares the helpers defined here.

Bounds, derived:
  (a) the sums: |G - einsum| <= n 2^-52 sum_p |R_i R_j| w on the same fp64 rows R (tests/test_lmfit.py: check_tiles' bound).  The rows
      are rebuilt here with the core's own recurrence, fma included (exact rational arithmetic, rounded once).
  (b) the polynomial: max_p |p(x_p) - p_oracle(x_p)| <= max(n, 16) 2^-52 cond_2(A^) max_p |p_oracle|, A^ the unit-diagonal normal
      matrix of the kept pixels: the forward error of a backward-stable solve of the scaled normal equations whose entries carry
      (a)'s relative error.
  (c) chi^2 = e^T G e, e = (c, -1): (n + P + 3) 2^-52 sum_ij |e_i e_j| sum_p |R_i R_j| w for the sums and the (P + 1)^2-term quadratic
      form, plus bound_b^2 sum_kept w m^2 for the coefficients' error, which enters in second order at the minimum.
  (d) the outputs: flux_out is f / p rounded to fp32 and w_out = w p^2 with p inside (b), so |flux_out p_o / f - 1| and
      |w_out / (w p_o^2) - 1| stay within 2^-24 resp. 2^-51 plus (b)'s relative error (once resp. twice)."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from numpy.polynomial.chebyshev import chebvander

from thepayne_amd import _lib
from thepayne_amd.fitting import fitutils
from test_lmfit import (DEFAULTS, CONVERGED, g20, recovery_inputs, reference_fit, sigma_distance, OracleModel, lm_reference)   # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NONPOSITIVE, TOO_FEW, SINGULAR, NAN, BAD_MODEL = range(6)
SENTINEL = -777.25
EPS = 2.0 ** -52
SHAPES = [(1, 1), (5, 1), (5, 2), (5, 4), (37, 1), (37, 2), (37, 4), (37, 8), (37, 15), (1000, 1), (1000, 2), (1000, 4), (1000, 8), (1000, 15),
          (3600, 1), (3600, 2), (3600, 4), (3600, 8), (3600, 15)]
LONG = (70001, 8)
_T = {}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def abscissa_of(n):
    """x [n] in [-1, 1]: ContinuumFit's for a grid that is not uniform; one point: 0.3."""
    if n == 1:
        return np.array([0.3])
    from thepayne_amd.fitting.contfit import abscissa
    return abscissa(5000.0 + np.cumsum(np.random.default_rng(n).uniform(0.5, 1.5, n)))


def aligned(n):
    return (n + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8, (n + 3) // 4 * 4 + 4


def unaligned(n):
    return n + 6, n + 3, n + 5


def contfit_case(rng, N, P, n, lds, index=None, n_models=None, noise=0.01):
    """flux fp32 [N, ld_f], w fp64 [N, ld_f], model fp32 [M, ld_m] (M = N without `index`), x [n]; flux = model * (a Chebyshev series
    with c_0 in [0.5, 2], |c_j| <= 0.1) + noise.  A tenth of the pixels has w = 0 (n > 1); star 1 holds NaN in the flux (and, without
    `index`, in its model row) exactly there; every array holds 1e30 beyond n (tests/test_lmfit.py: sums_case)."""
    ld_f, ld_m, ld_o = lds
    M = N if index is None else n_models
    x = abscissa_of(n)
    model = np.full((M, ld_m), np.float32(1e30))
    model[:, :n] = (1.0 + 0.1 * rng.normal(0, 1, (M, n))).astype(np.float32)
    coef = np.concatenate([rng.uniform(0.5, 2.0, (N, 1)), rng.uniform(-0.1, 0.1, (N, P - 1))], axis=1)
    rows = model[:, :n] if index is None else model[np.clip(index, 0, M - 1), :n]
    flux = np.full((N, ld_f), np.float32(1e30))
    flux[:, :n] = (rows.astype(np.float64) * (chebvander(x, P - 1) @ coef.T).T + noise * rng.normal(0, 1, (N, n))).astype(np.float32)
    w = np.full((N, ld_f), 1e30)
    w[:, :n] = 1.0 / rng.uniform(0.005, 0.05, (N, n)) ** 2
    if n > 1:
        zero = rng.uniform(size=(N, n)) < 0.1
        zero[:, 0] = False
        w[:, :n][zero] = 0.0
        if N > 1:
            flux[1, :n][zero[1]] = np.nan
            if index is None:
                model[1, :n][zero[1]] = np.nan
    return dict(flux=flux, w=w, model=model, x=x, n=n, P=P, N=N, lds=lds, index=None if index is None else np.asarray(index, dtype=np.int32), truth=coef)


def model_rows(case):
    """The model row of every star [N, n] (zeros for an index out of range) and whether it has one."""
    M = case["model"].shape[0]
    idx = np.arange(case["N"]) if case["index"] is None else case["index"]
    has = (idx >= 0) & (idx < M)
    return np.where(has[:, None], case["model"][np.clip(idx, 0, M - 1), :case["n"]], np.float32(0)), has


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def oracle_star(f, w, m, x, P, nclip=0, kappa=(3.0, 3.0), rescale=False, has_model=True):
    """One star in numpy fp64 as include/payne_hip.h states it.  dict(status, coef, chisq, npix, rounds, masks [rounds][n], margin (the
    smallest |z - threshold| / s met over the counting pixels), cond (of the unit-diagonal normal matrix of the last solve))."""
    n = len(f)
    out = dict(status=BAD_MODEL, coef=np.full(P, np.nan), chisq=np.nan, npix=0, rounds=0, masks=[], margin=np.inf, cond=np.nan)
    if not has_model:
        return out
    counting = w != 0.0
    kept = counting.copy()
    out["npix"] = int(kept.sum())
    f64, m64 = f.astype(np.float64), m.astype(np.float64)
    if not (np.all(np.isfinite(f64[counting])) and np.all(np.isfinite(m64[counting])) and np.all(np.isfinite(w[counting]))):
        return dict(out, status=NAN)
    fz, mz = np.where(counting, f64, 0.0), np.where(counting, m64, 0.0)
    V = chebvander(x, P - 1) * mz[:, None]
    sw = np.sqrt(w)
    for rnd in range(nclip + 1):
        out["npix"] = int(kept.sum())
        if kept.sum() < P:
            return dict(out, status=TOO_FEW, coef=np.full(P, np.nan), chisq=np.nan)
        A, b = sw[kept, None] * V[kept], sw[kept] * fz[kept]
        d = np.einsum("pi,pi->i", A, A)
        if np.any(d <= 0.0):
            return dict(out, status=SINGULAR, coef=np.full(P, np.nan), chisq=np.nan)
        c = np.linalg.lstsq(A, b, rcond=None)[0]
        As = A / np.sqrt(d)
        out.update(status=OK, coef=c, chisq=float(np.sum((b - A @ c) ** 2)), rounds=rnd + 1, cond=float(np.linalg.cond(As.T @ As)))
        out["masks"].append(kept.copy())
        if rnd == nclip:
            break
        s = np.sqrt(out["chisq"] / max(1, int(kept.sum()) - P)) if rescale else 1.0
        z = sw * (fz - V @ c)
        new = counting & (z >= -kappa[0] * s) & (z <= kappa[1] * s)
        out["margin"] = min(out["margin"], float(np.min(np.minimum(np.abs(z + kappa[0] * s), np.abs(z - kappa[1] * s))[counting]) / s))
        if np.array_equal(new, kept):
            break
        kept = new
    return out


def oracle(case, **kw):
    rows, has = model_rows(case)
    n = case["n"]
    return [oracle_star(case["flux"][s, :n], case["w"][s, :n], rows[s], case["x"], case["P"], has_model=bool(has[s]), **kw) for s in range(case["N"])]


def cheb_table(x, P):
    """T_j(x_p) [n, P] by contfit_core.hpp's recurrence, T_k = fma(2 x, T_k-1, -T_k-2): exact rationals, rounded once."""
    key = (x.tobytes(), P)
    if key not in _T:
        T = np.ones((len(x), P))
        if P > 1:
            T[:, 1] = x
        for p in range(len(x)):
            two_x = Fraction(2.0 * x[p])
            for k in range(2, P):
                T[p, k] = float(two_x * Fraction(T[p, k - 1]) - Fraction(T[p, k - 2]))
        _T[key] = T
    return _T[key]


def rows_of(f, w, m, x, P, kept):
    """R [P + 1][n] as the core forms it, zero outside `kept`."""
    R = np.concatenate([(m.astype(np.float64)[:, None] * cheb_table(x, P)).T, f.astype(np.float64)[None, :]], axis=0)
    return np.where(kept[None, :], R, 0.0)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def compare(case, got, orc, what, nclip=0, drop_clipped=True, ratios=None):
    """`got`: dict(coef [N, P], chisq, npix, status, rounds, flux_out [N, ld_o], w_out [N, ld_o]) of the emulator or the device,
    against the oracle's list: statuses, rounds and npix exactly, bounds (b), (c), (d), the failure outputs, the sentinels beyond n."""
    n, P, N = case["n"], case["P"], case["N"]
    rows, has = model_rows(case)
    x = case["x"]
    V0 = chebvander(x, P - 1)
    ratios = ratios if ratios is not None else {}
    for s in range(N):
        o = orc[s]
        f, w, m = case["flux"][s, :n], case["w"][s, :n], rows[s]
        tag = (what, n, P, N, s)
        fo, wo = got["flux_out"][s, :n], got["w_out"][s, :n]
        counting = w != 0.0
        if o["status"] in (TOO_FEW, SINGULAR, NAN, BAD_MODEL):
            assert got["status"][s] == o["status"] and got["rounds"][s] == o["rounds"] and got["npix"][s] == o["npix"], (tag, got["status"][s], o["status"])
            assert np.all(np.isnan(got["coef"][s])) and np.isnan(got["chisq"][s]), tag
            assert not wo.any() and np.array_equal(fo, f, equal_nan=True), tag
            continue
        p_o = V0 @ o["coef"]
        nonpos = bool(np.any(p_o[counting] <= 0.0))
        assert got["status"][s] == (NONPOSITIVE if nonpos else OK), (tag, got["status"][s])
        assert got["rounds"][s] == o["rounds"] and got["npix"][s] == o["npix"], (tag, got["rounds"][s], o["rounds"], got["npix"][s], o["npix"])
        kept = o["masks"][-1]
        # (b)
        p_g = V0 @ got["coef"][s]
        bound_b = max(n, 16) * EPS * o["cond"] * np.abs(p_o).max()
        ratios["b"] = max(ratios.get("b", 0.0), float(np.abs(p_g - p_o).max() / bound_b))
        assert np.all(np.isfinite(got["coef"][s])) and np.abs(p_g - p_o).max() <= bound_b, (tag, np.abs(p_g - p_o).max(), bound_b)
        # (c)
        R = np.abs(rows_of(f, w, m, x, P, kept))
        e = np.abs(np.append(o["coef"], -1.0))
        bound_c = (n + P + 3) * EPS * float(e @ np.einsum("ip,jp,p->ij", R, R, w) @ e) + bound_b ** 2 * float(np.sum((w * m.astype(np.float64) ** 2)[kept]))
        ratios["c"] = max(ratios.get("c", 0.0), abs(got["chisq"][s] - o["chisq"]) / bound_c)
        assert abs(got["chisq"][s] - o["chisq"]) <= bound_c, (tag, got["chisq"][s], o["chisq"], bound_c)
        # (d)
        sure = np.abs(p_o) > 10.0 * bound_b                          # (where the oracle's sign of p decides)
        pos = (p_o > 0.0) & sure
        rel_b = bound_b / np.maximum(np.abs(p_o), 1e-300)
        live = counting & pos & ~(drop_clipped & ~kept)
        assert np.all(wo[~live & sure] == 0.0) and np.all(wo[live] > 0.0), tag
        assert np.all(np.abs(wo[live] / (w[live] * p_o[live] ** 2) - 1.0) <= 2 * EPS + 2.5 * rel_b[live]), tag
        fin = pos & np.isfinite(f) & (f != 0)
        q = fo[fin].astype(np.float64) * p_o[fin] / f[fin].astype(np.float64)
        assert np.all(np.abs(q - 1.0) <= 2.0 ** -24 + 2 * EPS + 1.5 * rel_b[fin]), (tag, np.abs(q - 1.0).max())
        assert np.all(fo[~pos & sure] == 0.0) and np.all(np.isnan(fo[pos & np.isnan(f)])), tag
    for name in ("flux_out", "w_out"):
        assert np.all(got[name][:, n:] == np.asarray(SENTINEL, dtype=got[name].dtype)), (what, name)
    return ratios


# ---- the emulator -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/contfit_emul.cpp built with the sanitizers; run(case, nclip, kappa, rescale, drop_clipped) -> compare's dict plus G
    [solves][16][16] and kept [solves][n], star after star."""
    build = tmp_path_factory.mktemp("contfit_emul")
    exe = str(build / "contfit_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "contfit_emul.cpp")],
                   check=True)
    count = [0]

    def run(case, nclip=0, kappa=(3.0, 3.0), rescale=False, drop_clipped=True, expect=0):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        N, n, P = case["N"], case["n"], case["P"]
        ld_f, ld_m, ld_o = case["lds"]
        M = case["model"].shape[0]
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d %d %d %d %d %d %r %r %r\n" % (N, n, ld_f, ld_m, ld_o, M, case["index"] is not None, P, nclip, rescale, drop_clipped,
                                                                   float(kappa[0]), float(kappa[1]), SENTINEL))
        for nm, a, dt in (("flux", case["flux"], np.float32), ("w", case["w"], np.float64), ("model", case["model"], np.float32), ("x", case["x"], np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        if case["index"] is not None:
            case["index"].astype(np.int32).tofile(str(d / "index.bin"))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        if expect:
            return None
        coef = np.fromfile(str(d / "coef.bin")).reshape(N + 1, P)
        assert np.all(coef[N] == SENTINEL)
        return dict(coef=coef[:N], chisq=np.fromfile(str(d / "chisq.bin")), npix=np.fromfile(str(d / "npix.bin"), dtype=np.int32),
                    status=np.fromfile(str(d / "status.bin"), dtype=np.int32), rounds=np.fromfile(str(d / "rounds.bin"), dtype=np.int32),
                    flux_out=np.fromfile(str(d / "flux_out.bin"), dtype=np.float32).reshape(N, ld_o), w_out=np.fromfile(str(d / "w_out.bin")).reshape(N, ld_o),
                    G=np.fromfile(str(d / "G.bin")).reshape(-1, 16, 16), kept=np.fromfile(str(d / "kept.bin"), dtype=np.uint8).reshape(-1, n).astype(bool))
    return run


def check_tiles(case, got, orc, what):
    """(a) on the tile of every solve the trace holds; zero outside the (P + 1) x (P + 1) block; the trace's masks are the oracle's."""
    n, P = case["n"], case["P"]
    rows, _ = model_rows(case)
    k, worst = 0, 0.0
    for s in range(case["N"]):
        assert got["rounds"][s] == orc[s]["rounds"], (what, s)
        for r in range(orc[s]["rounds"]):
            kept = orc[s]["masks"][r]
            assert np.array_equal(got["kept"][k], kept), (what, s, r, int((got["kept"][k] != kept).sum()))
            R = rows_of(case["flux"][s, :n], case["w"][s, :n], rows[s], case["x"], P, kept)
            want = np.einsum("ip,jp,p->ij", R, R, case["w"][s, :n])
            bound = n * EPS * np.einsum("ip,jp,p->ij", np.abs(R), np.abs(R), case["w"][s, :n])
            G = got["G"][k]
            worst = max(worst, float((np.abs(G[:P + 1, :P + 1] - want) / np.maximum(bound, 1e-300)).max()))
            assert np.all(np.abs(G[:P + 1, :P + 1] - want) <= bound), (what, n, P, s, r, worst)
            outside = G.copy()
            outside[:P + 1, :P + 1] = 0.0
            assert not outside.any()
            k += 1
    assert k == len(got["G"])
    return worst


def index_for(rng, N, M):
    """Repeated and permuted rows of M models for N stars."""
    idx = rng.permutation(np.arange(N) % M)
    return idx.astype(np.int32)


def shape_cases(n, P, seed=0):
    """The (N, leading dimensions, index) sets of one (n, P): 70 stars unaligned with a row each, 3 aligned through an index, 1
    unaligned through an index."""
    rng = np.random.default_rng(1000 * P + n + seed)
    yield contfit_case(rng, 70, P, n, unaligned(n))
    yield contfit_case(rng, 3, P, n, aligned(n), index=index_for(rng, 3, 2), n_models=2)
    yield contfit_case(rng, 1, P, n, unaligned(n), index=np.array([4]), n_models=5)


# ---- 1. sums and fit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", SHAPES)
def test_sums_and_fit_on_the_host(emul, n, P):
    ratios, worst = {}, 0.0
    for case in shape_cases(n, P):
        got, orc = emul(case), oracle(case)
        worst = max(worst, check_tiles(case, got, orc, "emulator"))
        compare(case, got, orc, "emulator", ratios=ratios)
    print("n=%d P=%d: max |dG| / bound (a) = %.3g, |dp| / bound (b) = %.3g, |dchi^2| / bound (c) = %.3g" % (n, P, worst, ratios.get("b", 0), ratios.get("c", 0)))


def test_one_long_row_on_the_host(emul):
    n, P = LONG
    case = contfit_case(np.random.default_rng(9), 2, P, n, unaligned(n))
    got, orc = emul(case, nclip=2), oracle(case, nclip=2)
    worst = check_tiles(case, got, orc, "emulator")
    ratios = compare(case, got, orc, "emulator", nclip=2)
    print("n=%d P=%d: (a) %.3g (b) %.3g (c) %.3g" % (n, P, worst, ratios.get("b", 0), ratios.get("c", 0)))


# ---- 2. clipping -------------------------------------------------------------------------------------------------------------------
CLIP_N, CLIP_P, NCLIP = (37, 1000, 3600), 4, 5
MARGIN = 1e-6


def clip_case(n, rescale, N=3):
    """Cosmic rays (+0.2 .. 2 on 3 % of the pixels) and dips (x 0.3 .. 0.8 on 3 %) on contfit_case's spectra.  The first seed for
    which the oracle alone keeps every counting pixel's z at least MARGIN s off both thresholds in every round (and clips something)."""
    for seed in range(50):
        rng = np.random.default_rng(7000 + 10 * n + seed)
        case = contfit_case(rng, N, CLIP_P, n, unaligned(n))
        f = case["flux"][:, :n]
        hit = rng.uniform(size=(N, n))
        f[hit < 0.03] += rng.uniform(0.2, 2.0, int((hit < 0.03).sum())).astype(np.float32)
        dip = (hit >= 0.03) & (hit < 0.06)
        f[dip] *= rng.uniform(0.3, 0.8, int(dip.sum())).astype(np.float32)
        orc = oracle(case, nclip=NCLIP, rescale=rescale)
        if all(o["status"] == OK and o["margin"] >= MARGIN and o["rounds"] >= 2 for o in orc):
            return case, orc
    raise AssertionError("no seed satisfies the condition")


@pytest.mark.parametrize("rescale", (False, True), ids=("unit", "rescale"))
@pytest.mark.parametrize("n", CLIP_N)
def test_clipping_on_the_host(emul, n, rescale):
    case, orc = clip_case(n, rescale)
    assert min(o["margin"] for o in orc) >= MARGIN
    for drop in (True, False):
        got = emul(case, nclip=NCLIP, rescale=rescale, drop_clipped=drop)
        check_tiles(case, got, orc, "emulator")                      # (the kept mask of every round equals the oracle's)
        compare(case, got, orc, "emulator", nclip=NCLIP, drop_clipped=drop)
        for s, o in enumerate(orc):
            clipped = (case["w"][s, :n] != 0) & ~o["masks"][-1]
            assert clipped.any() and got["npix"][s] == o["masks"][-1].sum() and got["rounds"][s] == o["rounds"]
            assert np.all((got["w_out"][s, :n][clipped] == 0.0) == drop)
    print("n=%d rescale=%s: rounds %s, clipped %s, smallest margin %.3g s" % (n, rescale, [o["rounds"] for o in orc],
          [int(((case["w"][s, :n] != 0) & ~o["masks"][-1]).sum()) for s, o in enumerate(orc)], min(o["margin"] for o in orc)))
    # fewer re-fits than the loop wants: the rounds stop at nclip + 1
    got = emul(case, nclip=1, rescale=rescale)
    orc1 = oracle(case, nclip=1, rescale=rescale)
    assert np.all(got["rounds"] == 2) and all(o["rounds"] == 2 for o in orc1)
    compare(case, got, orc1, "emulator", nclip=1)


# ---- 3. statuses -------------------------------------------------------------------------------------------------------------------
def status_case(n=37, P=4):
    """Seven stars: 0 OK, 1 TOO_FEW from the start (P - 1 counting pixels), 2 SINGULAR (its model row is zero), 3 NAN (a NaN flux at a
    counting pixel), 4 OK, 5 NAN (an infinite model value), 6 NONPOSITIVE (the flux negative on half the grid).  Returns the case;
    with `index`, stars 1 and 4 become BAD_MODEL (-1 and n_models)."""
    rng = np.random.default_rng(42)
    case = contfit_case(rng, 7, P, n, unaligned(n))
    f, w, m = case["flux"], case["w"], case["model"]
    w[1, :n] = 0.0
    w[1, [2, 9, 30]] = 1e4
    f[1, [2, 9, 30]], m[1, [2, 9, 30]] = 1.3, 1.0
    m[2, :n] = 0.0
    f[3, int(np.flatnonzero(w[3, :n])[3])] = np.nan
    m[5, int(np.flatnonzero(w[5, :n])[0])] = np.inf
    f[6, :n // 2] = -np.abs(f[6, :n // 2])
    return case


def test_statuses_on_the_host(emul):
    case = status_case()
    got, orc = emul(case), oracle(case)
    assert [o["status"] for o in orc] == [OK, TOO_FEW, SINGULAR, NAN, OK, NAN, OK] and list(got["status"]) == [OK, TOO_FEW, SINGULAR, NAN, OK, NAN, NONPOSITIVE]
    compare(case, got, orc, "emulator")
    assert np.all(np.isfinite(got["coef"][6])) and got["npix"][1] == 3 and got["rounds"][1] == 0
    # BAD_MODEL through an index: -1 and n_models; the neighbours are as before
    idx = np.arange(7, dtype=np.int32)
    idx[1], idx[4] = -1, 7
    case2 = dict(case, index=idx)
    got2, orc2 = emul(case2), oracle(case2)
    assert list(got2["status"]) == [OK, BAD_MODEL, SINGULAR, NAN, BAD_MODEL, NAN, NONPOSITIVE]
    compare(case2, got2, orc2, "emulator")
    for s in (0, 2, 3, 5, 6):
        for key in ("coef", "chisq", "npix", "status", "rounds", "flux_out", "w_out"):
            assert got2[key][s].tobytes() == got[key][s].tobytes(), (s, key)


def test_too_few_after_a_clip_on_the_host(emul):
    """Five counting pixels, P = 4, two of them far off: the first fit runs, the clip leaves three."""
    n, P = 37, 4
    case = contfit_case(np.random.default_rng(3), 3, P, n, unaligned(n), noise=1e-4)
    w, f = case["w"], case["flux"]
    w[1, :n] = 0.0
    w[1, [3, 11, 19, 27, 35]] = 1e4
    f[1, [3, 11, 19, 27, 35]], case["model"][1, [3, 11, 19, 27, 35]] = 1.3, 1.0
    f[1, 11] += 5.0
    f[1, 27] -= 5.0
    # with kappa = 0.5 the two outliers' own pull on the fit still leaves them outside
    got, orc = emul(case, nclip=3, kappa=(0.5, 0.5)), oracle(case, nclip=3, kappa=(0.5, 0.5))
    assert orc[1]["status"] == TOO_FEW and orc[1]["rounds"] >= 1 and orc[1]["margin"] >= MARGIN, (orc[1]["status"], orc[1]["rounds"], orc[1]["margin"])
    assert got["status"][1] == TOO_FEW and got["rounds"][1] == orc[1]["rounds"] and got["npix"][1] == orc[1]["npix"] < P
    assert np.all(np.isnan(got["coef"][1])) and not got["w_out"][1, :n].any() and np.array_equal(got["flux_out"][1, :n], f[1, :n], equal_nan=True)
    assert orc[0]["margin"] >= MARGIN and orc[2]["margin"] >= MARGIN
    compare(case, got, orc, "emulator", nclip=3)


# ---- 4. arguments ------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from thepayne_amd.fitting import contfit
    wave = np.linspace(5150.0, 5300.0, 10)
    w_, x, o = contfit.check_setup(wave)
    assert o == dict(P=4, nclip=0, rescale=False, drop_clipped=True, kappa_lo=3.0, kappa_hi=3.0) and x[0] == -1.0 and x[-1] == 1.0
    assert np.array_equal(fitutils.polycalc([0.0, 1.0], wave), x)
    assert contfit.check_setup(wave, npoly=15, nclip=16, kappa=2.5)[2]["kappa_hi"] == 2.5
    for bad in (dict(obs_wave=wave[:1]), dict(obs_wave=wave[::-1]), dict(obs_wave=np.where(np.arange(10) == 3, np.nan, wave)), dict(obs_wave=wave.reshape(2, 5)),
                dict(npoly=0), dict(npoly=16), dict(npoly=2.5), dict(nclip=-1), dict(nclip=17), dict(kappa=(3.0, 0.0)), dict(kappa=(-1.0, 3.0)),
                dict(kappa=(1.0, 2.0, 3.0)), dict(kappa=np.nan)):
        with pytest.raises(ValueError):
            contfit.check_setup(**dict(dict(obs_wave=wave), **bad))
    N, nobs = 3, 10
    flux, eflux, model = np.ones((N, nobs)), np.full((N, nobs), 0.01), np.ones((N, nobs))
    eflux[0, 2], eflux[1, 3] = 0.0, np.inf
    f, w, m, idx = contfit.check_contfit_args(flux, eflux, model, None, nobs)
    assert f.dtype == np.float32 and w.dtype == np.float64 and m.dtype == np.float32 and idx is None and w[0, 2] == 0.0 and w[1, 3] == 0.0 and w[2, 2] == 1e4
    idx = contfit.check_contfit_args(flux, eflux, np.ones((5, nobs)), [0, -7, 9], nobs)[3]
    assert idx.dtype == np.int32 and list(idx) == [0, -1, 5]
    for bad in (dict(flux=np.ones((N, nobs + 1))), dict(eflux=np.ones((N + 1, nobs))), dict(model=np.ones((N, nobs - 1))), dict(model=np.ones((N + 1, nobs))),
                dict(model=np.ones((5, nobs)), index=[0, 1]), dict(model=np.ones((5, nobs)), index=[0.0, 1.0, 2.0])):
        kw = dict(dict(flux=flux, eflux=eflux, model=model, index=None), **bad)
        with pytest.raises(ValueError):
            contfit.check_contfit_args(kw["flux"], kw["eflux"], kw["model"], kw["index"], nobs)
    assert "payne_contfit_batch" in _lib.SYMBOLS and _lib.CONTFIT_MAX_P == 15 and _lib.CONTFIT_MAX_N == 262144
    assert (_lib.CONTFIT_OK, _lib.CONTFIT_NONPOSITIVE, _lib.CONTFIT_TOO_FEW, _lib.CONTFIT_SINGULAR, _lib.CONTFIT_NAN, _lib.CONTFIT_BAD_MODEL) == tuple(range(6))
    o = _lib.ContfitOpts(P=8, nclip=3, rescale=True, drop_clipped=False, kappa_lo=2.0, kappa_hi=4.0)
    assert (o.P, o.nclip, o.rescale, o.drop_clipped, o.kappa_lo, o.kappa_hi) == (8, 3, 1, 0, 2.0, 4.0)
    import ctypes
    assert ctypes.sizeof(_lib.ContfitOpts) == 32
    from thepayne_amd.fitting import optfit
    assert hasattr(optfit.OptFit, "fit_with_continuum") and hasattr(contfit.ContinuumFit, "fit_to_bank")


def test_the_emulator_refuses_what_the_library_refuses(emul):
    case = contfit_case(np.random.default_rng(1), 2, 4, 37, unaligned(37))
    for bad in (dict(nclip=17), dict(nclip=-1), dict(kappa=(0.0, 3.0)), dict(kappa=(3.0, -1.0))):
        assert emul(case, expect=3, **bad) is None
    assert emul(dict(case, P=16), expect=3) is None and emul(dict(case, P=0), expect=3) is None


# ---- 5. polycalc -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 4, 15))
def test_coefficients_are_polycalc_s(emul, P):
    """fitutils.polycalc(coef, obs_wave) equals flux / flux_out on the counting pixels within the rounding of the quotient: flux_out is
    f / p rounded to fp32 (2^-24), and polycalc's Clenshaw sum differs from the core's forward sum by a few 2^-53 sum |c_j|: 2^-23."""
    from thepayne_amd.fitting.contfit import abscissa
    n = 1000
    wave = 5000.0 + np.cumsum(np.random.default_rng(n).uniform(0.5, 1.5, n))
    case = contfit_case(np.random.default_rng(11 + P), 3, P, n, unaligned(n))
    assert np.array_equal(case["x"], abscissa(wave))
    got = emul(case)
    for s in range(3):
        ok = (case["w"][s, :n] != 0) & (case["flux"][s, :n] != 0)
        p = fitutils.polycalc(got["coef"][s], wave)
        q = case["flux"][s, :n][ok].astype(np.float64) / got["flux_out"][s, :n][ok].astype(np.float64)
        assert got["status"][s] == OK and np.all(np.abs(q - p[ok]) <= 2.0 ** -23 * np.abs(p[ok]))


# ---- 6. the alternation's fp64 reference -------------------------------------------------------------------------------------------
# Block-coordinate descent converges linearly, and slowly where a label moves the spectrum's mean level as c_0 does: on these stars
# the fp64 loop is 0.7 .. 1.1 sigma from the truth after 3 rounds, 0.01 .. 0.16 after 16, and stops moving at 0.005 .. 0.007 (every
# label fit CONVERGED at its first evaluation) within 40.  40 rounds it is, decided by this reference alone.
ALT_WHICH, ALT_NOBS, ALT_STARS, ALT_P, ALT_ROUNDS = "synth5", 1000, 3, 4, 40
_ALT = {}


def alternation_inputs(g20):
    """tests/test_lmfit.py's recovery stars (the first ALT_STARS) with their spectrum at the truth multiplied by a P = 4 series,
    c_0 in [0.5, 2], |c_j| <= 0.1.  Returns (net, nntype, case, coef [stars, P], flux fp64 [stars, nobs], x)."""
    if "in" not in _ALT:
        from thepayne_amd.fitting.contfit import abscissa
        net, nntype, case, _ = recovery_inputs(g20, ALT_WHICH, ALT_NOBS, False)
        rng = np.random.default_rng(321)
        coef = np.concatenate([rng.uniform(0.5, 2.0, (ALT_STARS, 1)), rng.uniform(-0.1, 0.1, (ALT_STARS, ALT_P - 1))], axis=1)
        x = abscissa(case["obs_wave"])
        poly = chebvander(x, ALT_P - 1) @ coef.T
        flux = np.array([OracleModel(net, nntype, case["obs_wave"], case["truth"][i])(case["truth"][i][case["cols"]])[0] * poly[:, i] for i in range(ALT_STARS)])
        _ALT["in"] = (net, nntype, case, coef, flux, x)
    return _ALT["in"]


def reference_alternation(net, nntype, case, star, flux, x, rounds=ALT_ROUNDS, P=ALT_P, dtype=None, start=None):
    """OptFit.fit_with_continuum for one star in numpy fp64: the oracle's polynomial against the model at the current labels, then
    lm_reference on flux / p with the errors e / p, `rounds` times.  Returns (lm_reference's dict of the last round, coef, chisq per
    round)."""
    cols = case["cols"]
    pars = case["start"][star].copy()
    if start is not None:
        pars[cols] = start
    e = case["eflux"][star]
    w = 1.0 / e ** 2
    res, c, chis = None, None, []
    for r in range(rounds):
        model = OracleModel(net, nntype, case["obs_wave"], pars, dtype=dtype)(pars[cols])[0]
        o = oracle_star(flux.astype(np.float32), w, model.astype(np.float32), x, P)
        assert o["status"] == OK
        c = o["coef"]
        p = chebvander(x, P - 1) @ c
        sub = dict(case, eflux=np.where(np.arange(len(case["eflux"]))[:, None] == star, e / p, case["eflux"]))
        res, _ = reference_fit(net, nntype, sub, (flux.astype(np.float32) / p).astype(np.float32).astype(np.float64), star, start=pars[cols], dtype=dtype)
        pars[cols] = res["x"]
        chis.append(res["chisq"])
    return res, c, chis


def alternation_reference(g20):
    """The fp64 alternation on every star of alternation_inputs, cached for the GPU test."""
    if "ref" not in _ALT:
        net, nntype, case, coef, flux, x = alternation_inputs(g20)
        _ALT["ref"] = [reference_alternation(net, nntype, case, i, flux[i], x) for i in range(ALT_STARS)]
    return _ALT["ref"]


def test_reference_alternation_recovers_the_truth(g20):
    """The numpy alternation alone ends CONVERGED within 10 xtol sigma of the truth (tests/test_lmfit.py's sense for its own inputs),
    with the polynomial back; the GPU test leans on this."""
    net, nntype, case, coef, flux, x = alternation_inputs(g20)
    V = chebvander(x, ALT_P - 1)
    for i, (res, c, chis) in enumerate(alternation_reference(g20)):
        d = sigma_distance(res["x"], case["truth"][i][case["cols"]], res["A"])
        dp = float(np.abs(V @ (c - coef[i])).max())
        print("star %d: status %d, %.3g sigma from the truth, polynomial off by %.3g at most, chi^2 per round %s" % (i, res["status"], d, dp, ["%.3g" % v for v in chis]))
        assert res["status"] == CONVERGED and d <= 10.0 * DEFAULTS["xtol"], (i, res["status"], d)
        assert dp <= 1e-3                                             # (far inside the errors' 1e-2)
