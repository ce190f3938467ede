"""The template-pair search on the device: payne_tmatch_match_pairs through the C ABI against the host emulator (bytes),
``TemplateBank.match_pairs`` and ``OptFit.fit_binary_from_bank`` end to end.  The inputs, the references and the bounds are
tests/test_tmatch_pair.py's, which checks the emulator against the long double reference and runs the end-to-end inputs' reference loop
on the CPU."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import CONVERGED, RECOVERY_BMAX, g20, sigma_distance                                              # noqa: F401
from test_tmatch import CHUNK, match_case
from test_tmatch_gpu import SENTINEL, dev, run_abi, same, small_bank
from test_tmatch_pair import (KEYS, ROWS, SHAPE_NK, SHAPE_N_PIX, binary_bank_inputs, build_pair_emulator, check_edge_case, edge_case, few_pairs_case,
                              pair_case, same_bytes, shape_cases)

pytestmark = pytest.mark.gpu
MAX_STARS, MAX_TEMPLATES, MAX_PRIMARIES = 70, 300, 16


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_pair_emulator(tmp_path_factory.mktemp("tmatch_pair_emul_gpu"), sanitize=False)


@pytest.fixture(scope="module")
def handle(lib):
    import torch
    from thepayne_amd.fitting.tmatch import TMatchHandle
    h = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0), max_primaries=MAX_PRIMARIES)
    yield h
    h.close()


def run_pairs(lib, h, templates, flux, w, n, cand, topk, want_all=True):
    """payne_tmatch_match_pairs on host arrays with their own pitches -> dict(idx_a, idx_b, chisq, amp, all or None) on the host; what
    the call must not touch keeps a sentinel."""
    import torch
    (M, ld_t), (N, ld_f), kA = templates.shape, flux.shape, cand.shape[1]
    t_d, f_d, w_d, c_d = dev(templates.astype(np.float32)), dev(flux.astype(np.float32)), dev(w.astype(np.float64)), dev(cand.astype(np.int32))
    idx_a = torch.full((N, topk), -9, dtype=torch.int32, device="cuda:0")
    idx_b = torch.full((N, topk), -9, dtype=torch.int32, device="cuda:0")
    chisq = torch.full((N, topk), SENTINEL, dtype=torch.float64, device="cuda:0")
    amp = torch.full((N, topk, 2), SENTINEL, dtype=torch.float64, device="cuda:0")
    every = torch.full((N * kA, M + 2), SENTINEL, dtype=torch.float64, device="cuda:0") if want_all else None
    rc = lib.payne_tmatch_match_pairs(h._h, t_d.data_ptr(), ld_t, M, f_d.data_ptr(), w_d.data_ptr(), ld_f, N, n, c_d.data_ptr(), kA, topk, idx_a.data_ptr(),
                                      idx_b.data_ptr(), chisq.data_ptr(), amp.data_ptr(), every.data_ptr() if want_all else None, M + 2, None)
    assert rc == 0, (rc, lib.payne_last_error(None))
    torch.cuda.synchronize()
    out = dict(idx_a=idx_a.cpu().numpy(), idx_b=idx_b.cpu().numpy(), chisq=chisq.cpu().numpy(), amp=amp.cpu().numpy(), all=None)
    if want_all:
        e = every.cpu().numpy()
        assert np.all(e[:, M:] == SENTINEL)
        out["all"] = np.ascontiguousarray(e[:, :M]).reshape(N, kA, M)
    return out


def check_call(lib, handle, emul, templates, flux, w, n, cand, topk, what):
    """One call: the emulator's bytes; a second call, all_dev = NULL and the last star alone give the same bytes."""
    got = run_pairs(lib, handle, templates, flux, w, n, cand, topk)
    want = emul(templates, flux, w, n, cand, topk)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, "differs from the emulator's")
    assert same_bytes(run_pairs(lib, handle, templates, flux, w, n, cand, topk), got), (what, "a second call")
    assert same_bytes(run_pairs(lib, handle, templates, flux, w, n, cand, topk, want_all=False), got), (what, "all_dev NULL")
    N = flux.shape[0]
    if N > 1:
        alone = run_pairs(lib, handle, templates, flux[N - 1:], w[N - 1:], n, cand[N - 1:], topk)
        assert same_bytes(alone, got, slice(N - 1, N)), (what, "a star alone")
    return got


# ---- 1. through the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NK", SHAPE_NK, ids=["N%d-kA%d" % nk for nk in SHAPE_NK])
@pytest.mark.parametrize("n", SHAPE_N_PIX)
def test_shapes_through_the_abi(lib, handle, emul, n, NK):
    """tests/test_tmatch_pair.py's shapes, on which it holds the emulator to the long double reference: the emulator's bytes."""
    assert lib.payne_tmatch_pair_rows() == ROWS and lib.payne_tmatch_pair_chunk() == CHUNK
    N, kA = NK
    rng = np.random.default_rng(1000 * n + 10 * N + kA)
    for M, topk in shape_cases(n, NK):
        templates, flux, w, cand, _ = pair_case(rng, N, M, n, kA)
        check_call(lib, handle, emul, templates, flux, w, n, cand, topk, "device n=%d N=%d kA=%d M=%d topk=%d" % (n, N, kA, M, topk))


def test_survey_length_spectra_through_the_abi(lib, handle, emul):
    rng = np.random.default_rng(3600)
    templates, flux, w, cand, truth = pair_case(rng, 70, 300, 3600, 4, ld_t=3600, ld_f=3604)
    got = check_call(lib, handle, emul, templates, flux, w, 3600, cand, 4, "device n=3600 N=70 kA=4 M=300 topk=4")
    pairs = np.sort(np.stack([got["idx_a"][:, 0], got["idx_b"][:, 0]], axis=1), axis=1)
    assert np.array_equal(pairs, np.sort(truth, axis=1))


def test_edge_cases_through_the_abi(lib, handle, emul):
    templates, flux, w, cand, n = edge_case()
    got = run_pairs(lib, handle, templates, flux, w, n, cand, 8)
    check_edge_case(got, cand)
    assert same_bytes(got, emul(templates, flux, w, n, cand, 8))
    assert same_bytes(run_pairs(lib, handle, templates, flux, w, n, cand, 8, want_all=False), got)
    assert same_bytes(run_pairs(lib, handle, templates, flux[5:], w[5:], n, cand[5:], 8), got, slice(5, 6))
    templates, flux, w, cand, n = few_pairs_case()
    got = run_pairs(lib, handle, templates, flux, w, n, cand, 8)
    assert np.all(got["idx_b"][:, 2:] == -1) and np.all(got["idx_a"][:, 2:] == -1) and np.all(np.isinf(got["chisq"][:, 2:])) and np.all(np.isnan(got["amp"][:, 2:]))
    assert same_bytes(got, emul(templates, flux, w, n, cand, 8))


def test_the_match_call_on_a_pairs_handle_gives_its_emulator_s_bytes(lib, handle, tmp_path_factory):
    from test_tmatch import build_emulator
    plain_emul = build_emulator(tmp_path_factory.mktemp("tmatch_emul_on_pairs"), sanitize=False)
    templates, flux, w = match_case(np.random.default_rng(10), 17, 2 * CHUNK + 3, 37)
    cand = np.zeros((17, 2), dtype=np.int32)
    cand[:, 1] = 1
    run_pairs(lib, handle, templates, flux, w, 37, cand, 3)
    assert same(run_abi(lib, handle, templates, flux, w, 37, 3), plain_emul(templates, flux, w, 37, 3))


def test_invalid_arguments_return_codes_and_touch_nothing(lib, handle):
    import torch
    from thepayne_amd.fitting.tmatch import TMatchHandle
    templates, flux, w, cand, _ = pair_case(np.random.default_rng(9), 2, 3, 5, 2)

    def call(h=handle._h, M=3, N=2, n=5, kA=2, topk=1, ld_t=None, ld_f=None, ld_a=5, nulls=()):
        t_d, f_d, w_d, c_d = dev(templates), dev(flux), dev(w), dev(cand)
        idx_a = torch.full((2, 8), -9, dtype=torch.int32, device="cuda:0")
        idx_b = torch.full((2, 8), -9, dtype=torch.int32, device="cuda:0")
        chisq = torch.full((2, 8), SENTINEL, dtype=torch.float64, device="cuda:0")
        amp = torch.full((2, 8, 2), SENTINEL, dtype=torch.float64, device="cuda:0")
        every = torch.full((4, 5), SENTINEL, dtype=torch.float64, device="cuda:0")
        ptr = dict(t=t_d.data_ptr(), f=f_d.data_ptr(), w=w_d.data_ptr(), cand=c_d.data_ptr(), idx_a=idx_a.data_ptr(), idx_b=idx_b.data_ptr(),
                   chisq=chisq.data_ptr(), amp=amp.data_ptr(), all=every.data_ptr())
        for k in nulls:
            ptr[k] = None
        rc = lib.payne_tmatch_match_pairs(h, ptr["t"], templates.shape[1] if ld_t is None else ld_t, M, ptr["f"], ptr["w"], flux.shape[1] if ld_f is None else ld_f,
                                          N, n, ptr["cand"], kA, topk, ptr["idx_a"], ptr["idx_b"], ptr["chisq"], ptr["amp"], ptr["all"], ld_a, None)
        torch.cuda.synchronize()
        touched = bool((idx_a != -9).any().item() or (idx_b != -9).any().item() or (chisq != SENTINEL).any().item() or (amp != SENTINEL).any().item()
                       or (every != SENTINEL).any().item())
        return rc, touched
    assert call() == (0, True)
    for kw in (dict(h=None), dict(kA=0), dict(kA=MAX_PRIMARIES + 1), dict(kA=-1), dict(topk=0), dict(topk=9), dict(M=MAX_TEMPLATES + 1), dict(N=MAX_STARS + 1),
               dict(N=-1), dict(M=-1), dict(ld_t=4), dict(ld_f=4), dict(n=0), dict(ld_a=2), dict(nulls=("t",)), dict(nulls=("f",)), dict(nulls=("w",)),
               dict(nulls=("cand",)), dict(nulls=("idx_a",)), dict(nulls=("idx_b",)), dict(nulls=("chisq",)), dict(nulls=("amp",))):
        assert call(**kw) == (-1, False), kw
        assert len(lib.payne_last_error(None)) > 0
    assert call(N=0) == (0, False) and call(M=0) == (0, False)       # succeed and do nothing
    out = C.c_void_p()
    for a in ((0, 0, 10, 4), (0, 10, 0, 4), (0, 10, 10, 0), (0, 10, 10, MAX_PRIMARIES + 1)):
        assert lib.payne_tmatch_create_pairs(a[0], a[1], a[2], a[3], C.byref(out)) == -1 and not out.value
    assert lib.payne_tmatch_create_pairs(0, 1, 1, 1, None) == -1
    # a handle of fewer primaries refuses more; a handle of payne_tmatch_create refuses match_pairs
    few = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0), max_primaries=1)
    old = TMatchHandle(MAX_STARS, MAX_TEMPLATES, torch.device("cuda", 0))
    assert call(h=few._h, kA=1) == (0, True) and call(h=few._h, kA=2) == (-1, False)
    assert call(h=old._h, kA=1) == (-1, False)
    few.close()
    old.close()
    with pytest.raises(ValueError):
        TMatchHandle(4, 4, torch.device("cuda", 0), max_poly=2, max_primaries=2)


# ---- 2. TemplateBank.match_pairs ----------------------------------------------------------------------------------------------------------
def test_bank_finds_the_pair_a_mixture_was_made_of(g20):
    import torch
    net, nntype, obs_wave, bank = small_bank(g20, max_stars=5)      # 12 stars in blocks of 5
    M, nobs = len(bank), len(obs_wave)
    tmpl = bank.templates.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(12)
    N = 12
    a = rng.integers(0, M, N)
    b = (a + 1 + rng.integers(0, M - 1, N)) % M
    c = rng.uniform(0.8, 1.6, N)
    flux = (c[:, None] * (0.7 * tmpl[a] + 0.3 * tmpl[b])).astype(np.float32)
    eflux = np.full(flux.shape, 0.01)
    res = bank.match_pairs(flux, eflux, topk=3, primaries=4, return_all=True)
    single = bank.match(flux, eflux, topk=4, npoly=1)
    assert np.array_equal(res["shortlist"], single["index"]) and np.array_equal(res["single_chisq"], single["chisq"][:, 0]) and np.all(res["npix"] == nobs)
    print("pairs found %s, planted %s; ratio %s; chi^2 %s against the single template's %s"
          % (list(zip(res["index_a"][:, 0].tolist(), res["index_b"][:, 0].tolist())), list(zip(a.tolist(), b.tolist())), np.round(res["ratio"][:, 0], 4).tolist(),
             res["chisq"][:, 0].tolist(), res["single_chisq"].tolist()))
    # the pair can be found where one of its templates is among the four primaries, which the single-template search decides
    has = ((res["shortlist"] == a[:, None]) | (res["shortlist"] == b[:, None])).any(axis=1)
    assert has.sum() >= N // 2, has
    assert np.array_equal(res["index_a"][has, 0], a[has]) and np.array_equal(res["index_b"][has, 0], b[has])          # A is the brighter
    assert np.all(np.abs(res["ratio"][has, 0] - 0.3) < 1e-3) and np.all(np.abs(res["scale"][has, 0] - c[has]) < 1e-3 * c[has])
    assert np.all(res["ratio"][res["index_a"] >= 0] <= 0.5) and np.all(res["index_a"][:, 0] >= 0)
    assert np.all(res["chisq"][:, 0] < res["single_chisq"]) and np.all(res["chisq"][:, :-1] <= res["chisq"][:, 1:])
    assert np.array_equal(res["pars_a"][:, 0], bank.theta[res["index_a"][:, 0]], equal_nan=True)
    assert np.array_equal(res["pars_b"][:, 0], bank.theta[res["index_b"][:, 0]], equal_nan=True)
    assert res["all"].shape == (N, 4, M) and res["pars_a"].shape == (N, 3, 8)
    # device tensors in, and one block of all the stars: the same bytes
    keys = ("index_a", "index_b", "chisq", "scale", "ratio", "pars_a", "pars_b", "npix", "shortlist", "single_chisq", "all")
    devres = bank.match_pairs(torch.as_tensor(flux).to("cuda:0"), torch.as_tensor(eflux).to("cuda:0"), topk=3, primaries=4, return_all=True)
    assert all(np.asarray(devres[k]).tobytes() == np.asarray(res[k]).tobytes() for k in keys)
    bank.close()
    bank.max_stars = 4096
    whole = bank.match_pairs(flux, eflux, topk=3, primaries=4, return_all=True)
    assert all(np.asarray(whole[k]).tobytes() == np.asarray(res[k]).tobytes() for k in keys)
    # a shortlist of the caller's: out of range and twice named become -1; the secondary alone as the primary finds the pair too
    sl = np.stack([b, b, np.full(N, M + 3)], axis=1)
    r2 = bank.match_pairs(flux, eflux, topk=1, primaries=3, shortlist=sl)
    assert np.array_equal(r2["shortlist"], np.stack([b, np.full(N, -1), np.full(N, -1)], axis=1))
    assert np.array_equal(r2["index_a"][:, 0], a) and np.array_equal(r2["index_b"][:, 0], b) and np.all(np.abs(r2["ratio"][:, 0] - 0.3) < 1e-3)
    # a star without a valid pixel lists nothing; the plain search on the bank still works beside the pairs' handle
    fl = flux.copy()
    fl[1, :] = np.inf
    r3 = bank.match_pairs(fl, eflux, topk=2)
    assert r3["npix"][1] == 0 and np.all(r3["index_a"][1] == -1) and np.all(r3["index_b"][1] == -1) and np.all(np.isinf(r3["chisq"][1])) and np.all(np.isnan(r3["ratio"][1]))
    assert np.all(np.isnan(r3["pars_a"][1])) and r3["index_a"][0, 0] == res["index_a"][0, 0] and np.isinf(r3["single_chisq"][1])
    with pytest.raises(ValueError):
        bank.match_pairs(flux, eflux, primaries=9)
    bank.close()
    assert bank._pair_handle is None


# ---- 3. fit_binary_from_bank ----------------------------------------------------------------------------------------------------------------
def test_fit_binary_from_bank_recovers_the_binaries(g20):
    """tests/test_tmatch_pair.py's binaries and lattice: fit_binary_from_bank(topk=1) is fit_binary from match_pairs' starts, byte for
    byte; it ends CONVERGED within 1e-2 sigma of the fp64 reference loop started from numpy's pair (carried on to its minimum); its chi^2 is below the single
    template's."""
    from thepayne_amd.fitting.optfit import OptFit
    from thepayne_amd.fitting.tmatch import TemplateBank
    case = binary_bank_inputs(g20)
    net, nntype, a = case["net"], case["nntype"], case["args"]
    cols, Ka, b_pos = a["cols"], a["Ka"], a["b_pos"]
    free_b = [k for k in range(Ka) if b_pos[k] >= Ka]
    bank = TemplateBank(net, nntype, case["obs_wave"], b_max=64).build(case["theta"])
    fit = OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX)
    kw = dict(tie=case["tie"], npoly=1, fit_vrad=True)
    flux, eflux, keep = case["flux"], case["eflux"], case["kept"]
    m = bank.match_pairs(flux, eflux, topk=1, primaries=4)
    print("device pairs %s, numpy %s; ratio %s; scale %s" % (list(zip(m["index_a"][:, 0].tolist(), m["index_b"][:, 0].tolist())), case["pairs"].tolist(),
                                                              m["ratio"][:, 0].tolist(), m["scale"][:, 0].tolist()))
    res = fit.fit_binary_from_bank(flux, eflux, bank, topk=1, primaries=4, **kw)
    direct = fit.fit_binary(flux, eflux, m["pars_a"][:, 0], m["pars_b"][:, 0], ratio=np.clip(m["ratio"][:, 0], 0.01, 0.99), coef=m["scale"][:, :1], **kw)
    for key in ("pars_a", "pars_b", "ratio", "coef", "chisq", "fisher", "status", "niter", "at_bound", "err", "npix"):
        assert np.asarray(res[key]).tobytes() == np.asarray(direct[key]).tobytes(), key
    assert res["labels"] == direct["labels"] and np.all(res["start_rank"] == 0) and np.array_equal(res["start_chisq"], m["chisq"][:, 0])
    assert np.array_equal(res["start_index_a"], m["index_a"][:, 0]) and np.array_equal(res["start_index_b"], m["index_b"][:, 0])
    assert np.array_equal(res["single_chisq"], m["single_chisq"])
    assert len(keep) >= len(flux) - 1                                # (tests/test_tmatch_pair.py says which binary is left out, and why)
    for i in keep:
        first, ref = case["results"][i], case["results"][i]["polished"]   # (the reference loop's end, and the same loop carried on to its minimum)
        z = np.concatenate([res["pars_a"][i, cols], res["pars_b"][i, [cols[k] for k in free_b]], [res["ratio"][i]], res["coef"][i]])
        d = sigma_distance(z, ref["x"], ref["A"])
        print("binary %d: status %d after %d evaluations (reference: %d), d = %.3g sigma (bound 1e-2; %.3g from the reference loop's end at the default xtol), "
              "q = %.5f, chi^2 %.4g against the single template's %.4g"
              % (i, res["status"][i], res["niter"][i], first["niter"], d, sigma_distance(z, first["x"], first["A"]), res["ratio"][i], res["chisq"][i], res["single_chisq"][i]))
        assert res["status"][i] == CONVERGED, (i, res["status"][i])
        assert d <= 1e-2, (i, d)
        assert res["chisq"][i] < res["single_chisq"][i]
    bank.close()
