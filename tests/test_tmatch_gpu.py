"""Template-bank chi^2 search on the device: payne_tmatch_* through the C ABI against the host emulator (bytes) and the long double
sum (the derived bound), thepayne_amd/fitting/tmatch.py's TemplateBank, and OptFit.fit_from_bank end to end.  The inputs, the
references and the bounds are tests/test_tmatch.py's, which checks on the CPU that the recovery pool yields its stars."""
import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import CONVERGED, DEFAULTS, RECOVERY_BMAX, g20, recovery_net, sigma_distance                      # noqa: F401
from test_lmfit_gpu import device_spectra
from test_tmatch import (CHUNK, SHAPE_N_PIX, SHAPE_N_STARS, U, bank_recovery_inputs, build_emulator, check_edge_case, check_lists, check_values,
                         edge_case, few_templates_case, match_case, shape_cases)

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
MAX_STARS, MAX_TEMPLATES = 70, 1000


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emulator(tmp_path_factory.mktemp("tmatch_emul_gpu"), sanitize=False)


@pytest.fixture(scope="module")
def handle(lib):
    import torch
    from thepayne_amd.fitting.tmatch import TMatchHandle
    h = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0))
    yield h
    h.close()


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def run_abi(lib, h, templates, flux, w, n, topk, want_all=True, expect=0):
    """payne_tmatch_match on host arrays with their own pitches -> (idx, chisq, all or None) on the host; untouched entries keep a
    sentinel."""
    import torch
    (M, ld_t), (N, ld_f) = templates.shape, flux.shape
    t_d, f_d, w_d = dev(templates.astype(np.float32)), dev(flux.astype(np.float32)), dev(w.astype(np.float64))
    idx = torch.full((N, topk), -9, dtype=torch.int32, device="cuda:0")
    chisq = torch.full((N, topk), SENTINEL, dtype=torch.float64, device="cuda:0")
    every = torch.full((N, M + 2), SENTINEL, dtype=torch.float64, device="cuda:0") if want_all else None
    rc = lib.payne_tmatch_match(h._h, t_d.data_ptr(), ld_t, M, f_d.data_ptr(), w_d.data_ptr(), ld_f, N, n, topk, idx.data_ptr(), chisq.data_ptr(),
                                every.data_ptr() if want_all else None, M + 2, None)
    assert rc == expect, (rc, lib.payne_last_error(None))
    torch.cuda.synchronize()
    if want_all:
        e = every.cpu().numpy()
        assert np.all(e[:, M:] == SENTINEL)
        return idx.cpu().numpy(), chisq.cpu().numpy(), np.ascontiguousarray(e[:, :M])
    return idx.cpu().numpy(), chisq.cpu().numpy(), None


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b) if x is not None and y is not None)


def check_call(lib, handle, emul, templates, flux, w, n, topk, what):
    """One call: the emulator's bytes; the bound; a second call, all_dev = NULL and the last star alone give the same bytes."""
    got = run_abi(lib, handle, templates, flux, w, n, topk)
    want = emul(templates, flux, w, n, topk)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (what, "lists differ from the emulator's")
    assert got[2].tobytes() == want[2].tobytes(), (what, "chi^2 differ from the emulator's", float(np.nanmax(np.abs(got[2] - want[2]))))
    ref, bound = check_values(got[2], templates, flux, w, n, what)
    differ = check_lists(got[0], got[1], got[2], ref, bound, what)
    assert same(run_abi(lib, handle, templates, flux, w, n, topk), got), (what, "a second call")
    assert same(run_abi(lib, handle, templates, flux, w, n, topk, want_all=False), got[:2]), (what, "all_dev NULL")
    N = flux.shape[0]
    if N > 1:
        alone = run_abi(lib, handle, templates, flux[N - 1:], w[N - 1:], n, topk)
        assert same(alone, [g[N - 1:] for g in got]), (what, "a star alone")
    return differ


# ---- 1. through the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPE_N_STARS)
@pytest.mark.parametrize("n", SHAPE_N_PIX)
def test_shapes_through_the_abi(lib, handle, emul, n, N):
    rng = np.random.default_rng(100 * n + N)
    differ = 0
    for M, topk in shape_cases(n, N):
        templates, flux, w = match_case(rng, N, M, n)
        differ += check_call(lib, handle, emul, templates, flux, w, n, topk, "device n=%d N=%d M=%d topk=%d" % (n, N, M, topk))
    assert differ == 0


def test_survey_length_spectra_through_the_abi(lib, handle, emul):
    rng = np.random.default_rng(3600)
    templates, flux, w = match_case(rng, 70, 1000, 3600, ld_t=3600, ld_f=3604)
    assert check_call(lib, handle, emul, templates, flux, w, 3600, 4, "device n=3600 N=70 M=1000 topk=4") == 0


def test_edge_cases_through_the_abi(lib, handle, emul):
    templates, flux, w, n, copies = edge_case()
    got = run_abi(lib, handle, templates, flux, w, n, 8)
    check_edge_case(*got, copies)
    assert same(got, emul(templates, flux, w, n, 8))
    a, b = few_templates_case()
    idx, chisq, every = run_abi(lib, handle, a[0], a[1], a[2], 5, 8)
    assert np.all(idx[:, :3] >= 0) and np.all(idx[:, 3:] == -1) and np.all(np.isinf(chisq[:, 3:])) and same((idx, chisq, every), emul(a[0], a[1], a[2], 5, 8))
    idx, chisq, every = run_abi(lib, handle, b[0], b[1], b[2], 5, 3)
    assert np.all(np.isnan(every)) and np.all(idx == -1) and np.all(chisq == np.inf)
    rng = np.random.default_rng(8)
    templates, flux, w = match_case(rng, 3, 17, 37)
    good = np.flatnonzero(w[0, :37] != 0.0)
    flux[0, good[1]] = np.nan
    w[1, good[2]] = np.nan
    idx, chisq, every = run_abi(lib, handle, templates, flux, w, 37, 3)
    assert np.all(np.isnan(every[:2])) and np.all(idx[:2] == -1) and np.all(np.isfinite(every[2])) and np.all(idx[2] >= 0)


def test_invalid_arguments_return_codes_and_touch_nothing(lib, handle):
    import ctypes as C
    assert lib.payne_tmatch_chunk() == CHUNK
    templates, flux, w = match_case(np.random.default_rng(9), 2, 3, 5)

    def call(h=handle._h, M=3, N=2, n=5, topk=1, ld_t=None, ld_f=None, ld_a=5, nulls=()):
        import torch
        t_d, f_d, w_d = dev(templates), dev(flux), dev(w)
        idx = torch.full((2, 8), -9, dtype=torch.int32, device="cuda:0")
        chisq = torch.full((2, 8), SENTINEL, dtype=torch.float64, device="cuda:0")
        every = torch.full((2, 5), SENTINEL, dtype=torch.float64, device="cuda:0")
        ptr = dict(t=t_d.data_ptr(), f=f_d.data_ptr(), w=w_d.data_ptr(), idx=idx.data_ptr(), chisq=chisq.data_ptr(), all=every.data_ptr())
        for k in nulls:
            ptr[k] = None
        rc = lib.payne_tmatch_match(h, ptr["t"], templates.shape[1] if ld_t is None else ld_t, M, ptr["f"], ptr["w"], flux.shape[1] if ld_f is None else ld_f,
                                    N, n, topk, ptr["idx"], ptr["chisq"], ptr["all"], ld_a, None)
        torch.cuda.synchronize()
        touched = bool((idx != -9).any().item() or (chisq != SENTINEL).any().item() or (every != SENTINEL).any().item())
        return rc, touched
    assert call() == (0, True)
    for kw in (dict(h=None), dict(topk=0), dict(topk=9), dict(M=MAX_TEMPLATES + 1), dict(N=MAX_STARS + 1), dict(N=-1), dict(M=-1), dict(ld_t=4),
               dict(ld_f=4), dict(n=0), dict(ld_a=2), dict(nulls=("t",)), dict(nulls=("f",)), dict(nulls=("w",)), dict(nulls=("idx",)),
               dict(nulls=("chisq",))):
        assert call(**kw) == (-1, False), kw
        assert len(lib.payne_last_error(None)) > 0
    assert call(N=0) == (0, False) and call(M=0) == (0, False)       # succeed and do nothing
    out = C.c_void_p()
    for a in ((0, 0, 10), (0, 10, 0)):
        assert lib.payne_tmatch_create(a[0], a[1], a[2], C.byref(out)) == -1 and not out.value
    assert lib.payne_tmatch_create(0, 1, 1, None) == -1
    lib.payne_tmatch_destroy(None)


# ---- 2. TemplateBank --------------------------------------------------------------------------------------------------------------------
def small_bank(g20, nobs=64, b_max=16, max_stars=4096):
    from thepayne_amd.fitting.tmatch import TemplateBank
    net, nntype = recovery_net(g20, "smlp")
    wave = net["wavelength"]
    width = wave[-1] - wave[0]
    obs_wave = np.linspace(wave[0] + 0.2 * width, wave[-1] - 0.2 * width, nobs)
    bank = TemplateBank(net, nntype, obs_wave, b_max=b_max, max_stars=max_stars)
    steps = (2, 2, 2, 1, 1)[:bank.n_labels]
    return net, nntype, obs_wave, bank.lattice(steps, vrad=(-30.0, 0.0, 30.0), vrot=(10.0,), inst_R=(20000.0,), inner=(0.1, 0.9))


def test_bank_is_predict_batch_and_finds_its_own_rows(g20):
    import torch
    net, nntype, obs_wave, bank = small_bank(g20, max_stars=7)      # 24 stars in blocks of 7
    M, nobs = len(bank), len(obs_wave)
    assert M == 24 and tuple(bank.templates.shape) == (M, nobs) and bank.templates.dtype == torch.float32
    eng = bank.predictor.anns.engine
    th = np.full((M, eng.ncols), np.nan)
    th[:, :8] = bank.theta
    tmpl = bank.templates.cpu().numpy()
    assert eng.predict_batch(th, stage=2).cpu().numpy().tobytes() == tmpl.tobytes()
    assert np.all(np.isfinite(tmpl)) and len(np.unique(tmpl, axis=0)) == M
    eflux = np.full((M, nobs), 0.01)
    res = bank.match(bank.templates, torch.as_tensor(eflux), topk=3, return_all=True)       # device tensors in
    t64 = tmpl.astype(np.float64)
    bound = (2 * nobs + 4) * U * 4.0 * (1e4 * t64 * t64).sum(axis=1)
    print("own rows: max |chi^2| / bound = %.3g" % float((np.abs(res["chisq"][:, 0]) / bound).max()))
    assert np.array_equal(res["index"][:, 0], np.arange(M)) and np.all(np.abs(res["chisq"][:, 0]) <= bound)
    assert np.all(res["chisq"][:, 1] > bound) and np.all(res["npix"] == nobs) and res["all"].shape == (M, M)
    assert np.array_equal(res["pars"][:, 0], bank.theta, equal_nan=True) and res["pars"].shape == (M, 3, 8)
    host = bank.match(tmpl, eflux, topk=3, return_all=True)          # host arrays in: the same bytes
    assert all(np.asarray(host[k]).tobytes() == np.asarray(res[k]).tobytes() for k in ("index", "chisq", "pars", "npix", "all"))
    # a flux that is not finite does not count; a star without a valid pixel matches everything with chi^2 = 0
    fl = tmpl.copy()
    fl[0, 3] = np.nan
    fl[1, :] = np.inf
    r2 = bank.match(fl, eflux, topk=1)
    assert r2["npix"][0] == nobs - 1 and r2["index"][0, 0] == 0 and r2["npix"][1] == 0 and r2["index"][1, 0] == 0 and r2["chisq"][1, 0] == 0.0
    bank.close()


# ---- 3. fit_from_bank -------------------------------------------------------------------------------------------------------------------
def test_fit_from_bank_is_fit_from_the_best_templates(g20):
    from thepayne_amd.fitting.optfit import OptFit
    net, nntype, obs_wave, bank = small_bank(g20)
    fit = OptFit(net, nntype, obs_wave, b_max=RECOVERY_BMAX)
    rng = np.random.default_rng(11)
    N, D = 5, bank.n_labels
    cols = [0, 1, 2, 3] + ([6] if D == 5 else [])
    truth = np.full((N, 8), np.nan)
    truth[:, cols] = net["xmin"] + (0.2 + 0.6 * rng.uniform(size=(N, D))) * (net["xmax"] - net["xmin"])
    truth[:, 4], truth[:, 5], truth[:, 7] = rng.choice([-30.0, 0.0, 30.0], N), 10.0, 20000.0
    flux = device_spectra(fit, truth)
    eflux = np.full(flux.shape, 0.01)
    m = bank.match(flux, eflux, topk=3)
    print("Vrad of the best template %s, of the truth %s" % (m["pars"][:, 0, 4].tolist(), truth[:, 4].tolist()))
    keys = ("pars", "chisq", "fisher", "status", "niter", "at_bound", "err", "npix")
    one = fit.fit_from_bank(flux, eflux, bank, topk=1)
    direct = [fit.fit(flux, eflux, m["pars"][:, k]) for k in range(3)]
    for key in keys:
        assert np.asarray(one[key]).tobytes() == np.asarray(direct[0][key]).tobytes(), key
    assert np.array_equal(one["start_index"], m["index"][:, 0]) and np.array_equal(one["start_chisq"], m["chisq"][:, 0]) and np.all(one["start_rank"] == 0)
    assert one["labels"] == direct[0]["labels"]
    three = fit.fit_from_bank(flux, eflux, bank, topk=3)
    for s in range(N):
        valid = [k for k in range(3) if direct[k]["status"][s] not in (_lib.LMFIT_NAN, _lib.LMFIT_SINGULAR)]
        k = min(valid, key=lambda j: (direct[j]["chisq"][s], j)) if valid else 0
        assert three["start_rank"][s] == k and three["start_index"][s] == m["index"][s, k], (s, k, three["start_rank"][s])
        for key in keys:
            assert np.asarray(three[key][s]).tobytes() == np.asarray(direct[k][key][s]).tobytes(), (s, key)
    print("ranks kept with topk = 3: %s; statuses %s" % (three["start_rank"].tolist(), three["status"].tolist()))
    with pytest.raises(ValueError):
        OptFit(net, nntype, obs_wave[:-1], b_max=RECOVERY_BMAX).fit_from_bank(flux[:, :-1], eflux[:, :-1], bank)
    bank.close()


def test_recovery_from_the_lattice(g20):
    """tests/test_tmatch.py's 16 stars: fit_from_bank ends CONVERGED within 1e-2 sigma of the fp64 reference loop's solution."""
    from thepayne_amd.fitting.optfit import OptFit
    from thepayne_amd.fitting.tmatch import TemplateBank
    case = bank_recovery_inputs(g20)
    assert len(case["kept"]) == 16
    net, nntype, cols = case["net"], case["nntype"], case["cols"]
    bank = TemplateBank(net, nntype, case["obs_wave"], b_max=64).build(case["theta"])
    fit = OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX)
    flux = device_spectra(fit, case["truth"])
    res = fit.fit_from_bank(flux, case["eflux"], bank, topk=1)
    d = [sigma_distance(res["pars"][i, cols], case["results"][i]["x"], case["results"][i]["A"]) for i in range(16)]
    print("templates: device %s, numpy %s; statuses %s; evaluations %s; worst distance from the reference %.3g sigma (bound 1e-2)"
          % (res["start_index"].tolist(), case["best"].tolist(), res["status"].tolist(), res["niter"].tolist(), max(d)))
    assert np.all(res["status"] == CONVERGED), res["status"]
    assert max(d) <= 1e-2, d
    bank.close()
