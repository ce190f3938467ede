"""payne_tmatch_* on the host (thepayne_amd/csrc/tmatch_core.hpp through tests/emul/tmatch_emul.cpp, built with ASan + UBSan): the
chi^2 of every star against every template inside the derived bound of the direct sum in long double, the top-k lists, the edge
cases of the selection; and fitting/tmatch.py's host side (the lattice, the argument checks).  tests/test_tmatch_gpu.py runs the same
inputs through the library."""
import os
import subprocess

import numpy as np
import pytest

from thepayne_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 128                                          # payne_tmatch_chunk(): the emulator writes its own value, which must be this
SHAPE_N_PIX, SHAPE_N_STARS, TOPKS = (1, 5, 37, 1000), (1, 3, 17, 70), (1, 3, 8)
SHAPE_M = (1, 15, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
U = 2.0 ** -53


# ---- inputs and the long double reference ------------------------------------------------------------------------------------------
def match_case(rng, N, M, n, ld_t=None, ld_f=None):
    """templates fp32 [M, ld_t], flux fp32 [N, ld_f], w fp64 [N, ld_f]: spectra of order one, each star a template plus noise of
    S/N ~ 100.  Beyond n: 1e30 in the templates and in w, NaN in the flux.  For n > 1 a tenth of the pixels has w = 0 for every star
    with NaN in the flux AND in the templates there, and another tenth per star has w = 0 with NaN in that star's flux."""
    ld_t = n + 3 if ld_t is None else ld_t
    ld_f = n + 5 if ld_f is None else ld_f
    templates = np.full((M, ld_t), np.float32(1e30))
    templates[:, :n] = (1.0 - 0.3 * rng.uniform(size=(M, n)) ** 3).astype(np.float32)
    sigma = rng.uniform(0.005, 0.02, (N, n))
    flux = np.full((N, ld_f), np.float32(np.nan))
    flux[:, :n] = (templates[rng.integers(0, M, N), :n] + sigma * rng.normal(size=(N, n))).astype(np.float32)
    w = np.full((N, ld_f), 1e30)
    w[:, :n] = 1.0 / sigma ** 2
    if n > 1:
        common = rng.uniform(size=n) < 0.1
        common[0] = False
        own = rng.uniform(size=(N, n)) < 0.1
        own[:, 0] = False
        w[:, :n][:, common] = 0.0
        w[:, :n][own] = 0.0
        flux[:, :n][w[:, :n] == 0.0] = np.nan
        templates[:, :n][:, common] = np.nan
    return templates, flux, w


def direct_longdouble(templates, flux, w, n):
    """(chi^2 [N, M] as the direct sum of w (f - m)^2 in long double over the pixels with w != 0, the bound (2 n + 4) 2^-53 S with
    S = sum w f^2 + 2 sum |w f m| + sum w m^2).  A template value that is not finite at a weighted pixel gives NaN."""
    L = np.longdouble
    ok = w[:, :n] != 0.0
    f = np.where(ok, flux[:, :n], 0.0).astype(L)
    ww = np.where(ok, w[:, :n], 0.0).astype(L)
    fin = np.isfinite(templates[:, :n])
    T = np.where(fin, templates[:, :n], 0.0).astype(L)               # (a pixel without weight adds w (f - m)^2 = 0 for any finite m)
    N, M = flux.shape[0], templates.shape[0]
    chi = np.empty((N, M), dtype=L)
    d = np.empty_like(T)
    for s in range(N):
        np.subtract(T, f[s][None, :], out=d)
        np.square(d, out=d)
        chi[s] = np.einsum("tp,p->t", d, ww[s])
    S = (ww * f * f).sum(axis=1)[:, None] + 2.0 * np.einsum("sp,tp->st", np.abs(ww * f), np.abs(T)) + np.einsum("sp,tp->st", ww, np.square(T))
    chi[(ok.astype(np.int64) @ (~fin).astype(np.int64).T) > 0] = np.nan
    return chi, (2 * n + 4) * L(U) * S


def check_values(every, templates, flux, w, n, what):
    """every [N, M] inside the bound of the long double row; NaN exactly where the reference is.  Returns (reference, bound)."""
    want, bound = direct_longdouble(templates, flux, w, n)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(every), nan), what
    err = np.abs(every.astype(np.longdouble) - want)[~nan]
    some = bound[~nan] > 0
    ratio = float((err[some] / bound[~nan][some]).max()) if some.any() else 0.0
    print("%s: max |dchi2| / bound = %.3g" % (what, ratio))
    assert np.all(err <= bound[~nan]), (what, ratio)
    return want, bound


def stable_topk(row, k):
    """(idx [k], chisq [k]) of one row by a stable argsort; NaN left out; -1 / +inf where nothing is left."""
    order = np.argsort(row, kind="stable")
    order = order[~np.isnan(row[order])][:k]
    idx, c = np.full(k, -1, dtype=np.int32), np.full(k, np.inf)
    idx[:len(order)], c[:len(order)] = order, row[order]
    return idx, c


def check_lists(idx, chisq, every, want, bound, what):
    """The lists against the row they were taken from (exact), and against the long double row: an index may differ only where
    the two reference values lie closer than twice the bound.  Returns how many differed."""
    N, k = idx.shape
    differ = 0
    for s in range(N):
        i_own, c_own = stable_topk(every[s], k)
        assert np.array_equal(idx[s], i_own) and np.array_equal(chisq[s], c_own), (what, s, idx[s], i_own)
        i_ref, _ = stable_topk(np.asarray(want[s], dtype=np.float64), k)
        for j in range(k):
            if idx[s, j] != i_ref[j]:
                differ += 1
                assert idx[s, j] >= 0 and i_ref[j] >= 0 and abs(want[s, idx[s, j]] - want[s, i_ref[j]]) < 2.0 * max(bound[s, idx[s, j]], bound[s, i_ref[j]]), (what, s, j)
    return differ


def shape_cases(n, N):
    """The template counts and top-k of one (n, N): every M; topk walks 1, 3, 8 so that over the (n, N) grid every (M, topk) occurs."""
    start = SHAPE_N_PIX.index(n) + SHAPE_N_STARS.index(N)
    return [(M, TOPKS[(start + j) % 3]) for j, M in enumerate(SHAPE_M)]


# ---- the emulator -------------------------------------------------------------------------------------------------------------------
def build_emulator(build, sanitize=True):
    """tests/emul/tmatch_emul.cpp -> run(templates, flux, w, n, topk) -> (idx [N, topk], chisq [N, topk], all [N, M])."""
    exe = str(build / "tmatch_emul")
    if sanitize:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    else:                                                           # (for the device tests, which compare bytes: fma is exact either way)
        flags = ["-O2"]
        try:
            if " fma " in open("/proc/cpuinfo").read():
                flags.append("-mfma")
        except OSError:
            pass
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "emul", "tmatch_emul.cpp")], check=True)
    count = [0]

    def run(templates, flux, w, n, topk, expect=0):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        (M, ld_t), (N, ld_f) = templates.shape, flux.shape
        assert w.shape == flux.shape
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d\n" % (N, M, n, ld_t, ld_f, topk))
        for nm, a, dt in (("templates", templates, np.float32), ("flux", flux, np.float32), ("w", w, np.float64)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        assert int(open(str(d / "chunk.txt")).read()) == CHUNK
        if expect:
            return None
        return (np.fromfile(str(d / "idx.bin"), dtype=np.int32).reshape(N, topk), np.fromfile(str(d / "chisq.bin")).reshape(N, topk),
                np.fromfile(str(d / "all.bin")).reshape(N, M))
    return run


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emulator(tmp_path_factory.mktemp("tmatch_emul"))


# ---- 1. values and lists on the shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPE_N_STARS)
@pytest.mark.parametrize("n", SHAPE_N_PIX)
def test_values_and_lists_on_the_host(emul, n, N):
    """Every chi^2 within (2 n + 4) 2^-53 S of the long double sum; lists exact against the own row, and against the reference."""
    rng = np.random.default_rng(100 * n + N)
    differ = 0
    for M, topk in shape_cases(n, N):
        templates, flux, w = match_case(rng, N, M, n)
        idx, chisq, every = emul(templates, flux, w, n, topk)
        what = "host n=%d N=%d M=%d topk=%d" % (n, N, M, topk)
        want, bound = check_values(every, templates, flux, w, n, what)
        differ += check_lists(idx, chisq, every, want, bound, what)
    print("n=%d N=%d: %d list entries differ from the long double row's" % (n, N, differ))
    assert differ == 0


@pytest.mark.parametrize("topk", TOPKS)
def test_every_template_count_with_every_topk(emul, topk):
    rng = np.random.default_rng(7 + topk)
    for M in SHAPE_M:
        templates, flux, w = match_case(rng, 3, M, 37)
        idx, chisq, every = emul(templates, flux, w, 37, topk)
        want, bound = check_values(every, templates, flux, w, 37, "host M=%d topk=%d" % (M, topk))
        assert check_lists(idx, chisq, every, want, bound, (M, topk)) == 0
        assert np.all((idx >= 0).sum(axis=1) == min(topk, M))


# ---- 2. edge cases of the selection ---------------------------------------------------------------------------------------------------
def edge_case():
    """N = 4 stars, M = 2 CHUNK + 3 templates, n = 37.  Templates 5, 9 and CHUNK - 1, CHUNK, CHUNK + 7 are copies of template 2 (inside
    one chunk and across the boundary), and star 0 is template 2 itself: one chi^2 (zero within the bound: the expansion cancels, the
    result may be a rounding error below zero) for all six, lower index first.  Template 11 is NaN
    at pixel 3, where stars 0 and 1 have weight and star 2 has none.  Star 3 has w = 0 everywhere."""
    rng = np.random.default_rng(5)
    n, M, N = 37, 2 * CHUNK + 3, 4
    templates, flux, w = match_case(rng, N, M, n)
    templates[:, :n] = np.where(np.isnan(templates[:, :n]), np.float32(0.9), templates[:, :n])
    copies = [2, 5, 9, CHUNK - 1, CHUNK, CHUNK + 7]
    templates[copies[1:]] = templates[2]
    flux[0, :n] = templates[2, :n]
    w[0, :n] = 1e4
    w[1, 3], flux[1, 3] = 1e4, 1.0
    w[2, 3] = 0.0
    templates[11, 3] = np.nan
    w[3, :n] = 0.0
    return templates, flux, w, n, copies


def check_edge_case(idx, chisq, every, copies):
    assert idx[0, :6].tolist() == copies and np.all(chisq[0, :6] == chisq[0, 0]) and abs(chisq[0, 0]) < 1e-6 and np.all(chisq[0, 6:] > 1.0)
    assert np.isnan(every[0, 11]) and np.isnan(every[1, 11]) and np.isfinite(every[2, 11])
    assert 11 not in idx[0] and 11 not in idx[1]
    assert np.all(every[3] == 0.0) and idx[3].tolist() == list(range(8)) and np.all(chisq[3] == 0.0)
    assert np.all(np.diff(chisq, axis=1) >= 0.0)


def test_duplicates_nan_templates_and_unweighted_stars(emul):
    templates, flux, w, n, copies = edge_case()
    idx, chisq, every = emul(templates, flux, w, n, 8)
    check_edge_case(idx, chisq, every, copies)
    want, bound = check_values(every, templates, flux, w, n, "edge case")
    assert check_lists(idx, chisq, every, want, bound, "edge case") == 0


def few_templates_case():
    """topk = 8 > M = 3; and M = CHUNK + 2 templates that are all NaN at a weighted pixel."""
    rng = np.random.default_rng(6)
    a = match_case(rng, 3, 3, 5)
    b = list(match_case(rng, 3, CHUNK + 2, 5))
    b[0][:, 0] = np.nan
    return a, tuple(b)


def test_more_slots_than_templates(emul):
    a, b = few_templates_case()
    idx, chisq, every = emul(a[0], a[1], a[2], 5, 8)
    assert np.all(idx[:, :3] >= 0) and np.all(idx[:, 3:] == -1) and np.all(np.isinf(chisq[:, 3:])) and np.all(np.isfinite(chisq[:, :3]))
    for s in range(3):
        assert sorted(idx[s, :3].tolist()) == [0, 1, 2]
    idx, chisq, every = emul(b[0], b[1], b[2], 5, 3)
    assert np.all(np.isnan(every)) and np.all(idx == -1) and np.all(chisq == np.inf)


def test_a_nan_in_the_flux_or_weight_at_a_weighted_pixel_reaches_chisq(emul):
    rng = np.random.default_rng(8)
    templates, flux, w = match_case(rng, 3, 17, 37)
    good = np.flatnonzero(w[0, :37] != 0.0)
    flux[0, good[1]] = np.nan
    w[1, good[2]] = np.nan
    idx, chisq, every = emul(templates, flux, w, 37, 3)
    assert np.all(np.isnan(every[:2])) and np.all(idx[:2] == -1) and np.all(np.isfinite(every[2])) and np.all(idx[2] >= 0)


def test_arguments_the_library_rejects(emul):
    templates, flux, w = match_case(np.random.default_rng(9), 2, 3, 5)
    for n, topk in ((5, 0), (5, 9), (9, 1), (0, 1)):                # topk outside 1 .. 8, ld < n, n < 1
        emul(templates, flux, w, n, topk, expect=3)


# ---- 3. recovery inputs of tests/test_tmatch_gpu.py --------------------------------------------------------------------------------------
BANK_NOBS, BANK_POOL, BANK_N, BANK_VROT, BANK_INST_R = 100, 48, 16, 10.0, 20000.0
_BANK = {}


def bank_recovery_inputs(g20):
    """g20's SMLP, every star at Vrad 0, one Vrot and Inst_R, 100 pixels, S/N 100 errors, noiseless spectra of the fp64 oracle chain
    at truths in the inner 80 % of the box; the templates are the same chain at the cell centres of a 3-per-label lattice.  From a
    pool of 48 the first 16 stars on which the fp64 reference loop, started at the template that numpy's chi^2 ranks first, ends
    CONVERGED within 10 xtol sigma of the truth (the reference alone decides).  Returns dict(net, nntype, obs_wave, theta [3^D, 8], cols,
    truth [16, 8], eflux, best [16], results, kept of pool)."""
    if "case" not in _BANK:
        from test_lmfit import CONVERGED, DEFAULTS, OracleModel, lm_reference, recovery_net, sigma_distance
        from thepayne_amd.fitting.tmatch import lattice_theta
        net, nntype = recovery_net(g20, "smlp")
        rng = np.random.default_rng(4242)
        xmin, xmax = net["xmin"], net["xmax"]
        truth = np.full((BANK_POOL, 8), np.nan)
        D = len(xmin)
        cols = [0, 1, 2, 3] + ([6] if D == 5 else [])
        truth[:, cols] = xmin + (0.1 + 0.8 * rng.uniform(size=(BANK_POOL, D))) * (xmax - xmin)
        truth[:, 4], truth[:, 5], truth[:, 7] = 0.0, BANK_VROT, BANK_INST_R
        wave = net["wavelength"]
        width = wave[-1] - wave[0]
        obs_wave = np.linspace(wave[0] + 0.2 * width, wave[-1] - 0.2 * width, BANK_NOBS)
        theta = lattice_theta(xmin, xmax, 3, vrad=(0.0,), vrot=(BANK_VROT,), inst_R=(BANK_INST_R,))
        model = OracleModel(net, nntype, obs_wave, truth[0])
        templates = np.array([model(t[cols])[0] for t in theta])
        w = np.full(BANK_NOBS, 100.0 ** 2)
        keep, best, results = [], [], []
        for star in range(BANK_POOL):
            flux = model(truth[star, cols])[0]
            b = int(np.argmin(((flux[None, :] - templates) ** 2 * w).sum(axis=1)))
            res = lm_reference(model, theta[b, cols], xmin, xmax, flux, w)
            res["d"] = sigma_distance(res["x"], truth[star, cols], res["A"]) if res["status"] == CONVERGED else np.inf
            if res["status"] == CONVERGED and res["d"] <= 10.0 * DEFAULTS["xtol"]:
                keep.append(star)
                best.append(b)
                results.append(res)
            if len(keep) == BANK_N:
                break
        _BANK["case"] = dict(net=net, nntype=nntype, obs_wave=obs_wave, theta=theta, truth=truth[keep], eflux=np.full((len(keep), BANK_NOBS), 0.01),
                             best=np.array(best), results=results, kept=keep, cols=cols)
    return _BANK["case"]


def test_reference_loop_converges_from_the_best_template(golden):
    """The inputs tests/test_tmatch_gpu.py recovers through fit_from_bank: the pool yields its 16 stars."""
    case = bank_recovery_inputs(golden("g20_trainspec"))
    print("kept %s of the pool; evaluations %s; worst distance %.3g sigma" % (case["kept"], [r["niter"] for r in case["results"]], max(r["d"] for r in case["results"])))
    assert len(case["kept"]) == BANK_N


# ---- 4. fitting/tmatch.py on the host --------------------------------------------------------------------------------------------------
def test_lattice_counts_and_cell_centres():
    from thepayne_amd.fitting import tmatch
    xmin, xmax = np.array([4000.0, 0.0, -2.0, -0.2]), np.array([7000.0, 5.0, 0.5, 0.6])
    th = tmatch.lattice_theta(xmin, xmax, 3, vrad=(-30.0, 0.0, 30.0), vrot=(2.0, 20.0), inst_R=(20000.0,))
    assert th.shape == (3 ** 4 * 3 * 2, 8)
    for d in range(4):
        assert np.allclose(np.unique(th[:, d]), xmin[d] + (np.arange(3) + 0.5) / 3.0 * (xmax[d] - xmin[d]), rtol=1e-14)
    assert np.all(np.isnan(th[:, 6])) and np.all(th[:, 7] == 20000.0)
    assert th[0, 4] == -30.0 and th[1, 4] == -30.0 and th[0, 5] == 2.0 and th[1, 5] == 20.0 and th[2, 4] == 0.0   # Inst_R, then Vrot fastest
    assert th[-1, 0] == th[:, 0].max() and th[0, 0] == th[:, 0].min() and len(np.unique(th, axis=0)) == len(th)
    th = tmatch.lattice_theta(np.append(xmin, 0.5), np.append(xmax, 2.5), (2, 1, 4, 1, 3), inner=(0.1, 0.9))
    assert th.shape == (24, 8) and np.all(np.isnan(th[:, 7])) and np.all(th[:, 4] == 0.0) and np.all(th[:, 5] == 5.0)
    assert np.allclose(np.unique(th[:, 6]), 0.5 + (0.1 + 0.8 * (np.arange(3) + 0.5) / 3.0) * 2.0)
    assert np.allclose(np.unique(th[:, 1]), [2.5]) and np.allclose(np.unique(th[:, 0]), 4000.0 + 3000.0 * np.array([0.3, 0.7]))
    for bad in (dict(steps=0), dict(steps=(2, 2)), dict(inner=(0.5, 0.5)), dict(inner=(-0.1, 1.0)), dict(vrad=()), dict(vrad=(np.nan,)), dict(vrot=(np.inf,))):
        with pytest.raises(ValueError):
            tmatch.lattice_theta(xmin, xmax, **dict(dict(steps=2), **bad))
    with pytest.raises(ValueError):
        tmatch.lattice_theta(xmin[:3], xmax[:3], 2)


def test_match_and_fit_from_bank_argument_checks():
    from thepayne_amd.fitting import optfit, tmatch
    nobs = 10
    flux, eflux = np.ones((3, nobs)), np.full((3, nobs), 0.01)
    f, w = tmatch.check_match_args(flux, eflux, nobs, 4)
    assert f.dtype == np.float32 and w.dtype == np.float64 and np.allclose(w, 1e4)
    fl, ef = flux.copy(), eflux.copy()
    fl[0, 1], fl[1, 2], ef[2, 3], ef[2, 4], ef[0, 5] = np.nan, np.inf, 0.0, np.nan, np.inf
    w = tmatch.check_match_args(fl, ef, nobs, 1)[1]
    assert w[0, 1] == 0.0 and w[1, 2] == 0.0 and w[2, 3] == 0.0 and w[2, 4] == 0.0 and w[0, 5] == 0.0 and (w != 0.0).sum() == 3 * nobs - 5
    for bad in (dict(topk=0), dict(topk=9), dict(flux=np.ones((3, nobs + 1))), dict(eflux=np.ones((2, nobs)))):
        with pytest.raises(ValueError):
            tmatch.check_match_args(**dict(dict(flux=flux, eflux=eflux, nobs=nobs, topk=1), **bad))
    B = object.__new__(tmatch.TemplateBank)
    B.templates = None
    with pytest.raises(RuntimeError):
        B.match(flux, eflux)
    # fit_from_bank: another grid, something that is no bank, a start of the caller's
    F = object.__new__(optfit.OptFit)
    F.obs_wave = np.linspace(5200.0, 5201.0, nobs)
    B.obs_wave = F.obs_wave + 0.01
    with pytest.raises(ValueError):
        F.fit_from_bank(flux, eflux, B)
    B.obs_wave = F.obs_wave[:-1]
    with pytest.raises(ValueError):
        F.fit_from_bank(flux, eflux, B)
    with pytest.raises(TypeError):
        F.fit_from_bank(flux, eflux, object())
    B.obs_wave = F.obs_wave.copy()
    with pytest.raises(TypeError):
        F.fit_from_bank(flux, eflux, B, start=np.zeros((3, 8)))
    assert all(s in _lib.SYMBOLS for s in ("payne_tmatch_create", "payne_tmatch_match", "payne_tmatch_chunk", "payne_tmatch_destroy"))
    assert _lib.TMATCH_MAX_TOPK == 8


def test_one_result_per_star_over_the_ranks():
    """optfit.keep_best_rank, the rule of the three ``*_from_bank`` fits, on fabricated results of 4 stars at 3 ranks:
    star 0  valid at every rank, chi^2 5, 3, 3: rank 1 replaces rank 0, and rank 2's equal chi^2 does not replace rank 1;
    star 1  valid at rank 0, NAN at rank 1, SINGULAR with the lowest chi^2 at rank 2: neither replaces the valid one;
    star 2  SINGULAR at rank 0, NAN at rank 1, no template at rank 2: rank 0's is kept;
    star 3  SINGULAR at rank 0, valid with a higher chi^2 at rank 1 (which replaces it), no template at rank 2."""
    from thepayne_amd.fitting import optfit
    ok, sing, nan = _lib.LMFIT_CONVERGED, _lib.LMFIT_SINGULAR, _lib.LMFIT_NAN
    index = np.array([[10, 11, 12], [20, 21, 22], [30, 31, -1], [40, 41, -1]], dtype=np.int32)
    status = np.array([[ok, _lib.LMFIT_MAXITER, _lib.LMFIT_STALLED], [ok, nan, sing], [sing, nan, -9], [sing, ok, -9]], dtype=np.int32)
    chisq = np.array([[5.0, 3.0, 3.0], [4.0, np.nan, 1.0], [2.0, np.nan, -9.0], [1.0, 9.0, -9.0]])
    out = dict(optfit.empty_results(4, 2), pars=np.full((4, 8), np.nan), start_index=np.full(4, -1, dtype=np.int32),
               start_rank=np.full(4, -1, dtype=np.int32))
    asked = []

    def fit_rank(sel, r):
        asked.append((r, sel.tolist()))
        return dict(status=status[sel, r], chisq=chisq[sel, r], pars=np.tile((100.0 * r + sel)[:, None], (1, 8)), niter=np.full(len(sel), 7, dtype=np.int32))

    def record(dst, r):
        out["start_index"][dst] = index[dst, r]
    assert optfit.keep_best_rank(index, out, ("pars", "chisq", "status"), fit_rank, record) is out
    assert asked == [(0, [0, 1, 2, 3]), (1, [0, 1, 2, 3]), (2, [0, 1])]                              # a star without a template of a rank is not fitted there
    assert out["start_rank"].tolist() == [1, 0, 0, 1] and out["start_index"].tolist() == [11, 20, 30, 41]
    assert out["status"].tolist() == [_lib.LMFIT_MAXITER, ok, sing, ok] and out["chisq"].tolist() == [3.0, 4.0, 2.0, 9.0]
    assert np.array_equal(out["pars"], np.tile(np.array([100.0, 1.0, 2.0, 103.0])[:, None], (1, 8)))
    assert np.all(out["niter"] == 0) and np.all(np.isnan(out["fisher"]))                             # only the keys named are written
    # no template at any rank: nothing is fitted and the star stays as it was allocated
    out = dict(optfit.empty_results(1, 2), start_rank=np.full(1, -1, dtype=np.int32))
    optfit.keep_best_rank(np.full((1, 3), -1, dtype=np.int32), out, ("chisq", "status"), None, None)
    assert out["start_rank"][0] == -1 and out["status"][0] == nan and np.isnan(out["chisq"][0])
