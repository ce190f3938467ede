"""payne_tmatch_match_poly on the host (thepayne_amd/csrc/tmatch_poly_core.hpp through tests/emul/tmatch_poly_emul.cpp, built with
ASan + UBSan): the chi^2 of every star against every template with a Chebyshev series minimised out, inside the derived bound of the
long double reference; the lists with their coefficients and flags; the rules for NaN; a bank of decoys on which only the search with
a polynomial finds the truth; and the argument checks of ``TemplateBank.match(npoly=)`` and ``OptFit.fit_joint_from_bank``.
tests/test_tmatch_poly_gpu.py runs the same inputs through the library."""
import os
import subprocess

import numpy as np
import pytest

from thepayne_amd import _lib
from test_tmatch import SHAPE_N_PIX, TOPKS, U, check_lists, match_case, stable_topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STARS, CHUNK = 16, 64                                # payne_tmatch_poly_stars(), _chunk(): the emulator writes its own, which must be these
SHAPE_N_STARS = (1, STARS - 1, STARS + 1, 70)
SHAPE_M = (1, 15, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)    # test_tmatch.SHAPE_M on the chunk of 64
POLYS = (1, 2, 4, 8)
L = np.longdouble


# ---- inputs and the long double reference ------------------------------------------------------------------------------------------
def abscissa(n):
    return np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)


def poly_case(rng, N, M, n):
    """test_tmatch.match_case with every star multiplied by a positive cubic Chebyshev series; x [n]."""
    templates, flux, w = match_case(rng, N, M, n)
    x = abscissa(n)
    c = np.stack([rng.uniform(0.8, 1.6, N), rng.uniform(-0.3, 0.3, N), rng.uniform(-0.15, 0.15, N), rng.uniform(-0.08, 0.08, N)], axis=1)
    flux[:, :n] = (flux[:, :n] * np.polynomial.chebyshev.chebval(x, c.T)).astype(np.float32)
    return templates, flux, w, x


def reference(templates, flux, w, x, n, P):
    """Per pair in long double: c_ref [N, M, P] from the normal equations with one refinement step, chi^2_ref [N, M] = sum w (f - m
    p_ref)^2 summed directly, the bound B = (2 n + P^2 + 8) 2^-53 S_p, and a = sum |c_ref|.  NaN by the rules: a template value that is
    not finite at a counting pixel, fewer than P counting pixels, a template that is zero at every counting pixel."""
    ok = w[:, :n] != 0.0
    f = np.where(ok, flux[:, :n], 0.0).astype(L)
    ww = np.where(ok, w[:, :n], 0.0).astype(L)
    fin = np.isfinite(templates[:, :n])
    m = np.where(fin, templates[:, :n], 0.0).astype(L)
    N, M = flux.shape[0], templates.shape[0]
    T = np.polynomial.chebyshev.chebvander(x.astype(L), 2 * P - 2).T.astype(L)          # [2 P - 1, n]
    b = (((ww * f)[:, None, :] * T[None, :P]).reshape(N * P, n) @ m.T).reshape(N, P, M).transpose(0, 2, 1)
    S = ((ww[:, None, :] * T[None]).reshape(N * (2 * P - 1), n) @ (m * m).T).reshape(N, 2 * P - 1, M).transpose(0, 2, 1)
    jj, kk = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    A = 0.5 * (S[:, :, jj + kk] + S[:, :, np.abs(jj - kk)])                            # [N, M, P, P]
    nan = ((ok.astype(np.int64) @ (~fin).astype(np.int64).T) > 0) | (ok.sum(axis=1) < P)[:, None] | ~(S[:, :, 0] > 0)   # (a zero template)
    A64 = A.astype(np.float64)
    A64[nan] = np.eye(P)
    c = np.linalg.solve(A64, b.astype(np.float64)[..., None])[..., 0].astype(L)
    r = b - np.einsum("stjk,stk->stj", A, c)
    c = c + np.linalg.solve(A64, r.astype(np.float64)[..., None])[..., 0].astype(L)
    chi = np.empty((N, M), dtype=L)
    for s in range(N):
        d = f[s][None, :] - m * (c[s] @ T[:P])
        chi[s] = (ww[s][None, :] * d * d).sum(axis=1)
    a = np.abs(c).sum(axis=2)
    Sp = (ww * f * f).sum(axis=1)[:, None] + 2.0 * a * np.einsum("sp,tp->st", np.abs(ww * f), np.abs(m)) + a * a * np.einsum("sp,tp->st", ww, m * m)
    chi[nan], c[nan] = np.nan, np.nan
    return c, chi, (2 * n + P * P + 8) * L(U) * Sp, a


def check_poly_values(every, ref, what):
    c_ref, want, bound, a = ref
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(every), nan), what
    err = np.abs(every.astype(L) - want)[~nan]
    some = bound[~nan] > 0
    ratio = float((err[some] / bound[~nan][some]).max()) if some.any() else 0.0
    print("%s: max |dchi2| / B = %.3g" % (what, ratio))
    assert np.all(err <= bound[~nan]), (what, ratio)


def check_coef_and_flags(out, ref, w, x, n, P, what):
    """Listed pairs: coef within 1e-9 a of c_ref; flags against numpy; NaN and 0 in the empty slots."""
    c_ref, want, bound, a = ref
    idx, coef, flags = out["idx"], out["coef"], out["flags"]
    worst = 0.0
    for s in range(idx.shape[0]):
        counting = w[s, :n] != 0.0
        for j in range(idx.shape[1]):
            t = idx[s, j]
            if t < 0:
                assert np.all(np.isnan(coef[s, j])) and flags[s, j] == 0 and np.isinf(out["chisq"][s, j]), (what, s, j)
                continue
            d = float(np.abs(coef[s, j].astype(L) - c_ref[s, t]).max() / a[s, t])
            worst = max(worst, d)
            assert d <= 1e-9, (what, s, j, d)
            p = np.polynomial.chebyshev.chebval(x[counting], coef[s, j])
            if np.abs(p).min() > 1e-12:
                assert flags[s, j] == int(np.all(p > 0.0)), (what, s, j)
    return worst


def shape_cases(n, N):
    """The template counts, top-k and P of one (n, N): every M; topk walks 1, 3, 8 and P walks 1, 2, 4, 8, so that over the (n, N)
    grid every (M, topk) and every (M, P) occurs."""
    start = SHAPE_N_PIX.index(n) + SHAPE_N_STARS.index(N)
    return [(M, TOPKS[(start + j) % 3], POLYS[(start + j) % 4]) for j, M in enumerate(SHAPE_M)]


# ---- the emulator -------------------------------------------------------------------------------------------------------------------
def build_poly_emulator(build, sanitize=True):
    """tests/emul/tmatch_poly_emul.cpp -> run(templates, flux, w, x, n, topk, P) -> dict(idx, chisq, coef, flags, all); P = 0 runs the
    plain search (idx, chisq, all).  Sanitised as test_tmatch.build_emulator does it: linked statically, nothing preloaded."""
    exe = str(build / "tmatch_poly_emul")
    if sanitize:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    else:                                                           # (for the device tests, which compare bytes: fma is exact either way)
        flags = ["-O2"]
        try:
            if " fma " in open("/proc/cpuinfo").read():
                flags.append("-mfma")
        except OSError:
            pass
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "emul", "tmatch_poly_emul.cpp")], check=True)
    count = [0]

    def run(templates, flux, w, x, n, topk, P, expect=0):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        (M, ld_t), (N, ld_f) = templates.shape, flux.shape
        assert w.shape == flux.shape
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d %d\n" % (N, M, n, ld_t, ld_f, topk, P))
        for nm, a, dt in (("templates", templates, np.float32), ("flux", flux, np.float32), ("w", w, np.float64), ("x", x[:max(n, 0)], np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        assert open(str(d / "tile.txt")).read().split() == [str(STARS), str(CHUNK)]
        if expect:
            return None
        out = dict(idx=np.fromfile(str(d / "idx.bin"), dtype=np.int32).reshape(N, topk), chisq=np.fromfile(str(d / "chisq.bin")).reshape(N, topk),
                   all=np.fromfile(str(d / "all.bin")).reshape(N, M))
        if P:
            out["coef"] = np.fromfile(str(d / "coef.bin")).reshape(N, topk, P)
            out["flags"] = np.fromfile(str(d / "flags.bin"), dtype=np.int32).reshape(N, topk)
        return out
    return run


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_poly_emulator(tmp_path_factory.mktemp("tmatch_poly_emul"))


# ---- 1. values, lists, coefficients and flags on the shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPE_N_STARS)
@pytest.mark.parametrize("n", SHAPE_N_PIX)
def test_values_lists_and_coefficients_on_the_host(emul, n, N):
    """Every chi^2 within B = (2 n + P^2 + 8) 2^-53 S_p of the long double reference, NaN exactly where the rules say (n < P: all of
    it); lists exact against the own row and against the reference; coef within 1e-9 a; flags as numpy has them."""
    rng = np.random.default_rng(1000 * n + N)
    differ, worst = 0, 0.0
    for M, topk, P in shape_cases(n, N):
        templates, flux, w, x = poly_case(rng, N, M, n)
        out = emul(templates, flux, w, x, n, topk, P)
        what = "host n=%d N=%d M=%d topk=%d P=%d" % (n, N, M, topk, P)
        ref = reference(templates, flux, w, x, n, P)
        check_poly_values(out["all"], ref, what)
        if n < P:
            assert np.all(np.isnan(out["all"])) and np.all(out["idx"] == -1) and np.all(np.isinf(out["chisq"])), what
        differ += check_lists(out["idx"], out["chisq"], out["all"], ref[1], ref[2], what)
        worst = max(worst, check_coef_and_flags(out, ref, w, x, n, P, what))
    # (check_lists has asserted that an index differs only where the two values lie closer than 2 B: with as many coefficients as
    # counting pixels every template fits exactly and every chi^2 is a rounding error)
    print("n=%d N=%d: %d list entries differ from the reference row's; worst |dcoef| / a = %.3g" % (n, N, differ, worst))


# ---- 2. edge cases -------------------------------------------------------------------------------------------------------------------
SERIES = np.array([1.3, 0.25, -0.12, 0.06])


def poly_edge_case():
    """test_tmatch.edge_case on the chunk of 64, P = 4: N = 6 stars, M = 2 CHUNK + 3 templates, n = 37.  Templates 5, 9 and CHUNK - 1,
    CHUNK, CHUNK + 7 are copies of template 2 and star 0 is template 2 times SERIES: one chi^2 (zero within the bound) for all six,
    lower index first, SERIES as coefficients.  Template 11 is NaN at pixel 3, where stars 0 and 1 have weight and star 2 has none.
    Star 3 has w = 0 everywhere; star 4 has three counting pixels; star 5 is minus template 2, whose polynomial is negative.
    Template 20 is zero at every pixel."""
    rng = np.random.default_rng(5)
    n, M, N = 37, 2 * CHUNK + 3, 6
    templates, flux, w, x = poly_case(rng, N, M, n)
    templates[:, :n] = np.where(np.isnan(templates[:, :n]), np.float32(0.9), templates[:, :n])
    copies = [2, 5, 9, CHUNK - 1, CHUNK, CHUNK + 7]
    templates[copies[1:]] = templates[2]
    p = np.polynomial.chebyshev.chebval(x, SERIES)
    flux[0, :n] = (templates[2, :n].astype(np.float64) * p).astype(np.float32)
    w[0, :n] = 1e4
    w[1, 3], flux[1, 3] = 1e4, 1.0
    w[2, 3] = 0.0
    templates[11, 3] = np.nan
    w[3, :n] = 0.0
    w[4, :n] = 0.0
    w[4, [1, 17, 30]], flux[4, [1, 17, 30]] = 1e4, 1.0
    flux[5, :n], w[5, :n] = -templates[2, :n], 1e4
    templates[20, :n] = 0.0
    return templates, flux, w, x, n, copies


def check_poly_edge_case(out, copies):
    idx, chisq, every, coef, flags = out["idx"], out["chisq"], out["all"], out["coef"], out["flags"]
    assert idx[0, :6].tolist() == copies and np.all(chisq[0, :6] == chisq[0, 0]) and abs(chisq[0, 0]) < 1e-3 and np.all(chisq[0, 6:] > 1.0)
    assert np.all(np.abs(coef[0, :6] - SERIES) < 1e-6) and np.all(flags[0, :6] == 1)          # (the flux is fp32: 6e-8 relative)
    assert np.isnan(every[0, 11]) and np.isnan(every[1, 11]) and np.isfinite(every[2, 11])
    assert 11 not in idx[0] and 11 not in idx[1]
    for s in (3, 4):                                                # no counting pixel; fewer than P: nothing is listed
        assert np.all(np.isnan(every[s])) and np.all(idx[s] == -1) and np.all(np.isinf(chisq[s])) and np.all(np.isnan(coef[s])) and np.all(flags[s] == 0)
    assert idx[5, :6].tolist() == copies and np.all(flags[5, :6] == 0) and np.all(np.abs(coef[5, :6] - [-1.0, 0.0, 0.0, 0.0]) < 1e-9)
    assert np.all(np.isnan(every[:, 20])) and not np.any(idx == 20)                           # the solve refuses a zero template
    assert np.all(np.diff(chisq[[0, 1, 2, 5]], axis=1) >= 0.0)


def test_duplicates_nan_templates_unweighted_stars_and_negative_polynomials(emul):
    templates, flux, w, x, n, copies = poly_edge_case()
    out = emul(templates, flux, w, x, n, 8, 4)
    check_poly_edge_case(out, copies)
    ref = reference(templates, flux, w, x, n, 4)
    check_poly_values(out["all"], ref, "edge case")
    assert check_lists(out["idx"], out["chisq"], out["all"], ref[1], ref[2], "edge case") == 0


def test_a_nan_in_the_flux_or_weight_at_a_counting_pixel_reaches_chisq(emul):
    rng = np.random.default_rng(8)
    templates, flux, w, x = poly_case(rng, 3, 17, 37)
    good = np.flatnonzero(w[0, :37] != 0.0)
    flux[0, good[1]] = np.nan
    w[1, good[2]] = np.nan
    for P in (1, 4):
        out = emul(templates, flux, w, x, 37, 3, P)
        assert np.all(np.isnan(out["all"][:2])) and np.all(out["idx"][:2] == -1) and np.all(np.isfinite(out["all"][2])) and np.all(out["idx"][2] >= 0)


def test_arguments_the_library_rejects(emul):
    templates, flux, w, x = poly_case(np.random.default_rng(9), 2, 3, 5)
    for n, topk, P in ((5, 0, 1), (5, 9, 1), (9, 1, 1), (5, 1, 9)):
        emul(templates, flux, w, np.zeros(9), n, topk, P, expect=3)


def test_one_coefficient_is_the_free_amplitude(emul):
    """P = 1: chi^2 = c0 - b^2 / S against numpy's own fp64 sums."""
    rng = np.random.default_rng(12)
    templates, flux, w, x = poly_case(rng, 3, 17, 37)
    out = emul(templates, flux, w, x, 37, 3, 1)
    ok = w[:, :37] != 0.0
    f, ww, m = np.where(ok, flux[:, :37], 0.0).astype(np.float64), np.where(ok, w[:, :37], 0.0), np.nan_to_num(templates[:, :37].astype(np.float64))
    c0, b, S = (ww * f * f).sum(axis=1)[:, None], (ww * f) @ m.T, ww @ (m * m).T
    assert np.allclose(out["all"], c0 - b * b / S, rtol=1e-9, atol=1e-9 * float(c0.max()))
    assert np.allclose(out["coef"][:, 0, 0], (b / S)[np.arange(3), out["idx"][:, 0]], rtol=1e-12)


# ---- 3. the bank of decoys: only the search with a polynomial finds the truth -----------------------------------------------------------
DECOY_N, DECOY_K, DECOY_NPIX = 6, 12, 70


def decoy_case(seed):
    """K = 12 shapes m_k = 1 - 0.3 U(0, 1) per pixel, n = 70; N = 6 stars flux_s = m_s p_s + N(0, 0.01), w = 1e4, p_s a positive cubic;
    the bank is the 12 shapes plus 6 decoys d_s = m_u(s) p_s with u(s) from shapes 6 .. 11: at the star's level, of another shape."""
    rng = np.random.default_rng(seed)
    n, x = DECOY_NPIX, np.linspace(-1.0, 1.0, DECOY_NPIX)
    shapes = (1.0 - 0.3 * rng.uniform(size=(DECOY_K, n))).astype(np.float32)
    c = np.stack([rng.uniform(1.4, 1.8, DECOY_N), rng.uniform(-0.3, 0.3, DECOY_N), rng.uniform(-0.15, 0.15, DECOY_N), rng.uniform(-0.08, 0.08, DECOY_N)], axis=1)
    p = np.polynomial.chebyshev.chebval(x, c.T)
    flux = (shapes[:DECOY_N] * p + 0.01 * rng.normal(size=(DECOY_N, n))).astype(np.float32)
    u = rng.integers(6, DECOY_K, DECOY_N)
    bank = np.concatenate([shapes, (shapes[u] * p).astype(np.float32)])
    return bank, flux, np.full(flux.shape, 1e4), x, c


def decoy_reference(bank, flux, w, x):
    """(plain chi^2 [N, M], poly chi^2 with P = 4 [N, M], c_ref) in long double."""
    d = flux.astype(L)[:, None, :] - bank.astype(L)[None, :, :]
    c, chi, _, _ = reference(bank, flux, w, x, flux.shape[1], 4)
    return (w.astype(L)[:, None, :] * d * d).sum(axis=2), chi, c


def find_decoy_seed():
    """The first seed on which the reference alone gives: plain -> the star's decoy for all six, P = 4 -> the truth for all six with
    second - first > 1000."""
    for seed in range(200):
        bank, flux, w, x, c = decoy_case(seed)
        plain, poly, _ = decoy_reference(bank, flux, w, x)
        first = np.sort(poly.astype(np.float64), axis=1)
        if np.array_equal(np.argmin(plain, axis=1), DECOY_K + np.arange(DECOY_N)) and np.array_equal(np.argmin(poly, axis=1), np.arange(DECOY_N)) \
                and np.all(first[:, 1] - first[:, 0] > 1000.0):
            return seed
    raise AssertionError("no seed below 200 separates the two searches")


def check_decoy_reference(seed):
    bank, flux, w, x, c = decoy_case(seed)
    plain, poly, c_ref = decoy_reference(bank, flux, w, x)
    order = np.sort(poly.astype(np.float64), axis=1)
    assert np.array_equal(np.argmin(plain, axis=1), DECOY_K + np.arange(DECOY_N)), "plain chi^2 must rank every star's decoy first"
    assert np.array_equal(np.argmin(poly, axis=1), np.arange(DECOY_N)) and np.all(order[:, 1] - order[:, 0] > 1000.0)
    assert np.all(np.abs(c_ref[np.arange(DECOY_N), np.arange(DECOY_N)].astype(np.float64) - c) < 2e-2)
    return bank, flux, w, x, c


def check_decoy_result(poly_out, plain_idx, c):
    assert np.array_equal(poly_out["idx"][:, 0], np.arange(DECOY_N)), poly_out["idx"][:, 0]
    assert np.all(poly_out["chisq"][:, 1] - poly_out["chisq"][:, 0] > 1000.0) and np.all(poly_out["flags"][:, 0] == 1)
    assert np.all(np.abs(poly_out["coef"][:, 0] - c) < 2e-2)
    assert np.array_equal(plain_idx[:, 0], DECOY_K + np.arange(DECOY_N)), plain_idx[:, 0]


DECOY_SEED = 1                                       # find_decoy_seed()'s answer


def test_only_the_search_with_a_polynomial_finds_the_truth_among_decoys(emul):
    """On the reference first: plain chi^2 -> the decoy for all six, P = 4 -> the truth for all six.  Then the emulator's match_poly
    lists the truth first with its coefficients, and its plain twin (match_host) the decoy."""
    bank, flux, w, x, c = check_decoy_reference(DECOY_SEED)
    out = emul(bank, flux, w, x, DECOY_NPIX, 3, 4)
    plain = emul(bank, flux, w, x, DECOY_NPIX, 3, 0)
    check_decoy_result(out, plain["idx"], c)


# ---- 4. fitting/tmatch.py and optfit.py on the host ---------------------------------------------------------------------------------------
def test_match_npoly_and_fit_joint_from_bank_argument_checks():
    from thepayne_amd.fitting import optfit, tmatch
    nobs = 10
    flux, eflux = np.ones((3, nobs)), np.full((3, nobs), 0.01)
    assert [tmatch.check_npoly(p) for p in (0, 1, 8)] == [0, 1, 8]
    B = object.__new__(tmatch.TemplateBank)
    B.templates = None
    for bad in (-1, 9, 2.5, True):
        with pytest.raises(ValueError):
            tmatch.check_npoly(bad)
        with pytest.raises(ValueError):
            B.match(flux, eflux, npoly=bad)
    with pytest.raises(RuntimeError):
        B.match(flux, eflux, npoly=4)                               # the empty bank, as without npoly
    F = object.__new__(optfit.OptFit)
    F.obs_wave = np.linspace(5200.0, 5201.0, nobs)
    B.obs_wave = F.obs_wave + 0.01
    with pytest.raises(ValueError):
        F.fit_joint_from_bank(flux, eflux, B)
    with pytest.raises(TypeError):
        F.fit_joint_from_bank(flux, eflux, object())
    B.obs_wave = F.obs_wave.copy()
    for kw in (dict(start=np.zeros((3, 8))), dict(coef=np.zeros((3, 4)))):
        with pytest.raises(TypeError):
            F.fit_joint_from_bank(flux, eflux, B, **kw)
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError):
            F.fit_joint_from_bank(flux, eflux, B, npoly=bad)
    assert all(s in _lib.SYMBOLS for s in ("payne_tmatch_create_poly", "payne_tmatch_match_poly", "payne_tmatch_poly_stars", "payne_tmatch_poly_chunk"))
    assert _lib.TMATCH_MAX_POLY == 8
    import inspect
    assert inspect.signature(tmatch.TMatchHandle.__init__).parameters["max_poly"].default == 0
    assert inspect.signature(tmatch.TemplateBank.match).parameters["npoly"].default == 0
