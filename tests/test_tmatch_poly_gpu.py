"""The template search with a free continuum polynomial on the device: payne_tmatch_match_poly through the C ABI against the host
emulator (bytes) and the long double reference (the derived bound), ``TemplateBank.match(npoly=)`` and
``OptFit.fit_joint_from_bank`` end to end.  The inputs, the references and the bounds are tests/test_tmatch_poly.py's."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import RECOVERY_BMAX, g20                                                                        # noqa: F401
from test_lmfit_gpu import device_spectra
from test_tmatch import SHAPE_N_PIX, check_lists, match_case
from test_tmatch_gpu import SENTINEL, dev, run_abi, same, small_bank
from test_tmatch_poly import (CHUNK, DECOY_NPIX, DECOY_SEED, SERIES, SHAPE_N_STARS, STARS, build_poly_emulator, check_coef_and_flags, check_decoy_reference,
                              check_decoy_result, check_poly_edge_case, check_poly_values, poly_case, poly_edge_case, reference, shape_cases)

pytestmark = pytest.mark.gpu
MAX_STARS, MAX_TEMPLATES, MAX_POLY = 70, 1000, 8
KEYS = ("idx", "chisq", "coef", "flags", "all")


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_poly_emulator(tmp_path_factory.mktemp("tmatch_poly_emul_gpu"), sanitize=False)


@pytest.fixture(scope="module")
def handle(lib):
    import torch
    from thepayne_amd.fitting.tmatch import TMatchHandle
    h = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0), max_poly=MAX_POLY)
    yield h
    h.close()


def run_poly(lib, h, templates, flux, w, x, n, topk, P, want_all=True):
    """payne_tmatch_match_poly on host arrays with their own pitches -> dict(idx, chisq, coef, flags, all or None) on the host;
    what the call must not touch keeps a sentinel."""
    import torch
    (M, ld_t), (N, ld_f) = templates.shape, flux.shape
    t_d, f_d, w_d, x_d = dev(templates.astype(np.float32)), dev(flux.astype(np.float32)), dev(w.astype(np.float64)), dev(x.astype(np.float64))
    idx = torch.full((N, topk), -9, dtype=torch.int32, device="cuda:0")
    chisq = torch.full((N, topk), SENTINEL, dtype=torch.float64, device="cuda:0")
    coef = torch.full((N, topk, P), SENTINEL, dtype=torch.float64, device="cuda:0")
    flags = torch.full((N, topk), -9, dtype=torch.int32, device="cuda:0")
    every = torch.full((N, M + 2), SENTINEL, dtype=torch.float64, device="cuda:0") if want_all else None
    rc = lib.payne_tmatch_match_poly(h._h, t_d.data_ptr(), ld_t, M, f_d.data_ptr(), w_d.data_ptr(), ld_f, N, n, x_d.data_ptr(), P, topk, idx.data_ptr(),
                                     chisq.data_ptr(), coef.data_ptr(), flags.data_ptr(), every.data_ptr() if want_all else None, M + 2, None)
    assert rc == 0, (rc, lib.payne_last_error(None))
    torch.cuda.synchronize()
    out = dict(idx=idx.cpu().numpy(), chisq=chisq.cpu().numpy(), coef=coef.cpu().numpy(), flags=flags.cpu().numpy(), all=None)
    if want_all:
        e = every.cpu().numpy()
        assert np.all(e[:, M:] == SENTINEL)
        out["all"] = np.ascontiguousarray(e[:, :M])
    return out


def same_bytes(a, b, rows=slice(None)):
    return all(a[k].tobytes() == b[k][rows].tobytes() for k in KEYS if a[k] is not None and b[k] is not None)


def check_call(lib, handle, emul, templates, flux, w, x, n, topk, P, what, with_reference=True):
    """One call: the emulator's bytes; the bound; a second call, all_dev = NULL and the last star alone give the same bytes."""
    got = run_poly(lib, handle, templates, flux, w, x, n, topk, P)
    want = emul(templates, flux, w, x, n, topk, P)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, "differs from the emulator's")
    if with_reference:
        ref = reference(templates, flux, w, x, n, P)
        check_poly_values(got["all"], ref, what)
        check_lists(got["idx"], got["chisq"], got["all"], ref[1], ref[2], what)
        check_coef_and_flags(got, ref, w, x, n, P, what)
    assert same_bytes(run_poly(lib, handle, templates, flux, w, x, n, topk, P), got), (what, "a second call")
    assert same_bytes(run_poly(lib, handle, templates, flux, w, x, n, topk, P, want_all=False), got), (what, "all_dev NULL")
    N = flux.shape[0]
    if N > 1:
        alone = run_poly(lib, handle, templates, flux[N - 1:], w[N - 1:], x, n, topk, P)
        assert same_bytes(alone, got, slice(N - 1, N)), (what, "a star alone")


# ---- 1. through the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPE_N_STARS)
@pytest.mark.parametrize("n", SHAPE_N_PIX)
def test_shapes_through_the_abi(lib, handle, emul, n, N):
    assert lib.payne_tmatch_poly_stars() == STARS and lib.payne_tmatch_poly_chunk() == CHUNK
    rng = np.random.default_rng(1000 * n + N)
    for M, topk, P in shape_cases(n, N):
        templates, flux, w, x = poly_case(rng, N, M, n)
        check_call(lib, handle, emul, templates, flux, w, x, n, topk, P, "device n=%d N=%d M=%d topk=%d P=%d" % (n, N, M, topk, P))


def test_survey_length_spectra_through_the_abi(lib, handle, emul):
    rng = np.random.default_rng(3600)
    templates, flux, w = match_case(rng, 70, 300, 3600, ld_t=3600, ld_f=3604)
    x = np.linspace(-1.0, 1.0, 3600)
    flux[:, :3600] = (flux[:, :3600] * np.polynomial.chebyshev.chebval(x, SERIES)).astype(np.float32)
    check_call(lib, handle, emul, templates, flux, w, x, 3600, 4, 4, "device n=3600 N=70 M=300 topk=4 P=4", with_reference=False)


def test_edge_cases_through_the_abi(lib, handle, emul):
    templates, flux, w, x, n, copies = poly_edge_case()
    got = run_poly(lib, handle, templates, flux, w, x, n, 8, 4)
    check_poly_edge_case(got, copies)
    assert same_bytes(got, emul(templates, flux, w, x, n, 8, 4))
    rng = np.random.default_rng(8)
    templates, flux, w, x = poly_case(rng, 3, 17, 37)
    good = np.flatnonzero(w[0, :37] != 0.0)
    flux[0, good[1]] = np.nan
    w[1, good[2]] = np.nan
    for P in (1, 4):
        got = run_poly(lib, handle, templates, flux, w, x, 37, 3, P)
        assert np.all(np.isnan(got["all"][:2])) and np.all(got["idx"][:2] == -1) and np.all(np.isfinite(got["all"][2])) and np.all(got["idx"][2] >= 0)
        assert same_bytes(got, emul(templates, flux, w, x, 37, 3, P))


def test_refusals_old_handles_and_the_old_call_on_a_new_handle(lib, handle):
    import torch
    from thepayne_amd.fitting.tmatch import TMatchHandle
    templates, flux, w, x = poly_case(np.random.default_rng(9), 2, 3, 5)

    def call(h=handle._h, M=3, N=2, n=5, P=2, topk=1, ld_t=None, ld_f=None, ld_a=5, nulls=()):
        t_d, f_d, w_d, x_d = dev(templates), dev(flux), dev(w), dev(x)
        idx = torch.full((2, 8), -9, dtype=torch.int32, device="cuda:0")
        chisq = torch.full((2, 8), SENTINEL, dtype=torch.float64, device="cuda:0")
        coef = torch.full((2, 8, 8), SENTINEL, dtype=torch.float64, device="cuda:0")
        flags = torch.full((2, 8), -9, dtype=torch.int32, device="cuda:0")
        every = torch.full((2, 5), SENTINEL, dtype=torch.float64, device="cuda:0")
        ptr = dict(t=t_d.data_ptr(), f=f_d.data_ptr(), w=w_d.data_ptr(), x=x_d.data_ptr(), idx=idx.data_ptr(), chisq=chisq.data_ptr(), coef=coef.data_ptr(),
                   flags=flags.data_ptr(), all=every.data_ptr())
        for k in nulls:
            ptr[k] = None
        rc = lib.payne_tmatch_match_poly(h, ptr["t"], templates.shape[1] if ld_t is None else ld_t, M, ptr["f"], ptr["w"], flux.shape[1] if ld_f is None else ld_f,
                                         N, n, ptr["x"], P, topk, ptr["idx"], ptr["chisq"], ptr["coef"], ptr["flags"], ptr["all"], ld_a, None)
        torch.cuda.synchronize()
        touched = bool((idx != -9).any().item() or (chisq != SENTINEL).any().item() or (every != SENTINEL).any().item()
                       or (coef != SENTINEL).any().item() or (flags != -9).any().item())
        return rc, touched
    assert call() == (0, True)
    for kw in (dict(h=None), dict(P=0), dict(P=MAX_POLY + 1), dict(P=-1), dict(topk=0), dict(topk=9), dict(M=MAX_TEMPLATES + 1), dict(N=MAX_STARS + 1),
               dict(N=-1), dict(M=-1), dict(ld_t=4), dict(ld_f=4), dict(n=0), dict(ld_a=2), dict(nulls=("t",)), dict(nulls=("f",)), dict(nulls=("w",)),
               dict(nulls=("x",)), dict(nulls=("idx",)), dict(nulls=("chisq",)), dict(nulls=("coef",)), dict(nulls=("flags",))):
        assert call(**kw) == (-1, False), kw
        assert len(lib.payne_last_error(None)) > 0
    assert call(N=0) == (0, False) and call(M=0) == (0, False)       # succeed and do nothing
    out = C.c_void_p()
    for a in ((0, 0, 10, 4), (0, 10, 0, 4), (0, 10, 10, 0), (0, 10, 10, MAX_POLY + 1)):
        assert lib.payne_tmatch_create_poly(a[0], a[1], a[2], a[3], C.byref(out)) == -1 and not out.value
    assert lib.payne_tmatch_create_poly(0, 1, 1, 1, None) == -1
    # a handle of fewer coefficients refuses more; a handle of payne_tmatch_create refuses match_poly
    few = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0), max_poly=2)
    old = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0))
    assert call(h=few._h, P=2) == (0, True) and call(h=few._h, P=3) == (-1, False)
    assert call(h=old._h, P=1) == (-1, False)
    # payne_tmatch_match on a poly handle: the old call's bytes
    t2, f2, w2 = match_case(np.random.default_rng(10), 17, 2 * CHUNK + 3, 37)
    assert same(run_abi(lib, handle, t2, f2, w2, 37, 3), run_abi(lib, old, t2, f2, w2, 37, 3))
    few.close()
    old.close()


def test_the_decoy_bank_on_the_device(lib, handle):
    import torch
    bank, flux, w, x, c = check_decoy_reference(DECOY_SEED)
    got = run_poly(lib, handle, bank, flux, w, x, DECOY_NPIX, 3, 4)
    plain = run_abi(lib, handle, bank, flux, w, DECOY_NPIX, 3)
    check_decoy_result(got, plain[0], c)


# ---- 2. TemplateBank ----------------------------------------------------------------------------------------------------------------------
def test_bank_finds_its_own_rows_under_a_continuum(g20):
    import torch
    from thepayne_amd.fitting.contfit import abscissa
    net, nntype, obs_wave, bank = small_bank(g20, max_stars=7)      # 24 stars in blocks of 7
    M, nobs = len(bank), len(obs_wave)
    tmpl = bank.templates.cpu().numpy()
    x = abscissa(obs_wave)
    flux = (tmpl.astype(np.float64) * np.polynomial.chebyshev.chebval(x, SERIES)).astype(np.float32)
    eflux = np.full(flux.shape, 1e-3 * float(np.abs(tmpl).max()))
    before = bank.match(flux, eflux, topk=3, return_all=True)        # today's path, on a handle without the polynomial's workspace
    assert bank._handle.max_poly == 0 and "coef" not in before
    res = bank.match(flux, eflux, topk=3, return_all=True, npoly=4)
    c_ref, chi_ref, B, a = reference(tmpl, flux, 1.0 / eflux ** 2, x, nobs, 4)
    own = np.arange(M)
    print("own rows: max chi^2 = %.3g (numpy %.3g) against B >= %.3g; smallest second %.3g"
          % (float(np.abs(res["chisq"][:, 0]).max()), float(np.abs(chi_ref[own, own]).max()), float(B[own, own].min()), float(res["chisq"][:, 1].min())))
    assert np.array_equal(res["index"][:, 0], own) and np.all(np.abs(res["chisq"][:, 0]) <= B[own, own].astype(np.float64))
    assert np.all(res["chisq"][:, 1] > 100.0 * float(B.max()))
    assert np.all(np.abs(res["coef"][:, 0] - SERIES) < 1e-5) and np.all(res["positive"]) and res["positive"].dtype == np.bool_
    assert res["npoly"] == 4 and res["coef"].shape == (M, 3, 4) and np.all(res["npix"] == nobs) and res["all"].shape == (M, M)
    assert np.array_equal(res["pars"][:, 0], bank.theta, equal_nan=True)
    # without the polynomial the stars do not all find their own row: numpy's plain chi^2 of the same arrays decides
    plain = ((flux.astype(np.float64)[:, None, :] - tmpl.astype(np.float64)[None, :, :]) ** 2 / (eflux ** 2)[:, None, :]).sum(axis=2)
    assert not np.array_equal(np.argmin(plain, axis=1), own)
    assert np.array_equal(before["index"][:, 0], np.argmin(plain, axis=1))
    # device tensors in: the same bytes; npoly = 0 on the handle that now holds the workspace: the bytes of before
    keys = ("index", "chisq", "pars", "npix", "all", "coef", "positive")
    devres = bank.match(torch.as_tensor(flux).to("cuda:0"), torch.as_tensor(eflux).to("cuda:0"), topk=3, return_all=True, npoly=4)
    assert all(np.asarray(devres[k]).tobytes() == np.asarray(res[k]).tobytes() for k in keys)
    again = bank.match(flux, eflux, topk=3, return_all=True, npoly=0)
    assert bank._handle.max_poly == _lib.TMATCH_MAX_POLY
    assert all(np.asarray(again[k]).tobytes() == np.asarray(before[k]).tobytes() for k in ("index", "chisq", "pars", "npix", "all")) and "coef" not in again
    # a star without a valid pixel lists nothing
    fl = flux.copy()
    fl[1, :] = np.inf
    r2 = bank.match(fl, eflux, topk=2, npoly=4)
    assert r2["npix"][1] == 0 and np.all(r2["index"][1] == -1) and np.all(np.isinf(r2["chisq"][1])) and np.all(np.isnan(r2["coef"][1])) and not r2["positive"][1].any()
    assert np.all(np.isnan(r2["pars"][1])) and r2["index"][0, 0] == 0
    bank.close()


# ---- 3. fit_joint_from_bank ---------------------------------------------------------------------------------------------------------------
def test_fit_joint_from_bank_is_fit_joint_from_the_best_templates(g20):
    from thepayne_amd.fitting.contfit import abscissa
    from thepayne_amd.fitting.optfit import OptFit
    net, nntype, obs_wave, bank = small_bank(g20)
    fit = OptFit(net, nntype, obs_wave, b_max=RECOVERY_BMAX)
    rng = np.random.default_rng(11)
    N, D = 5, bank.n_labels
    cols = [0, 1, 2, 3] + ([6] if D == 5 else [])
    truth = np.full((N, 8), np.nan)
    truth[:, cols] = net["xmin"] + (0.2 + 0.6 * rng.uniform(size=(N, D))) * (net["xmax"] - net["xmin"])
    truth[:, 4], truth[:, 5], truth[:, 7] = rng.choice([-30.0, 0.0, 30.0], N), 10.0, 20000.0
    flux = (device_spectra(fit, truth).astype(np.float64) * np.polynomial.chebyshev.chebval(abscissa(obs_wave), SERIES)).astype(np.float32)
    eflux = np.full(flux.shape, 0.01)
    m = bank.match(flux, eflux, topk=3, npoly=4)
    keys = ("pars", "chisq", "fisher", "status", "niter", "at_bound", "err", "npix", "coef", "cont_status")
    one = fit.fit_joint_from_bank(flux, eflux, bank, npoly=4, topk=1)
    direct = [fit.fit_joint(flux, eflux, m["pars"][:, k], npoly=4, coef=m["coef"][:, k]) for k in range(3)]
    for key in keys:
        assert np.asarray(one[key]).tobytes() == np.asarray(direct[0][key]).tobytes(), key
    assert np.array_equal(one["start_index"], m["index"][:, 0]) and np.array_equal(one["start_chisq"], m["chisq"][:, 0]) and np.all(one["start_rank"] == 0)
    assert one["labels"] == direct[0]["labels"]
    three = fit.fit_joint_from_bank(flux, eflux, bank, npoly=4, topk=3)
    for s in range(N):
        valid = [k for k in range(3) if direct[k]["status"][s] not in (_lib.LMFIT_NAN, _lib.LMFIT_SINGULAR)]
        k = min(valid, key=lambda j: (direct[j]["chisq"][s], j)) if valid else 0
        assert three["start_rank"][s] == k and three["start_index"][s] == m["index"][s, k], (s, k, three["start_rank"][s])
        for key in keys:
            assert np.asarray(three[key][s]).tobytes() == np.asarray(direct[k][key][s]).tobytes(), (s, key)
    print("ranks kept with topk = 3: %s; statuses %s; coef %s" % (three["start_rank"].tolist(), three["status"].tolist(), three["coef"][0].tolist()))
    bank.close()
