"""Continuum polynomials on the device: payne_contfit_batch through the C ABI, thepayne_amd/fitting/contfit.py and
OptFit.fit_with_continuum end to end.  The inputs, the numpy fp64 oracle and the bounds (b), (c), (d) are tests/test_contfit.py's, which
holds the same arithmetic to the sums' bound (a) on the host, tile by tile; the ABI does not return the tile, so on the device (a) is
held through what follows from it: chi^2 inside (c), the polynomial inside (b), and every round's mask equal to the oracle's.

Yardstick of the alternation: tests/test_lmfit_gpu.py's for its noisy fits.  The distance d = max_k |x - x*| sqrt(F*_kk) of the
device's labels from the fp64 reference alternation's x* stays within max(10 xtol, 4 x the distance of the same numpy loop fed with
torch's CPU fp32 model and Jacobian, started at x*)."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import DEFAULTS, RECOVERY_BMAX, g20, recovery_net, sigma_distance                                   # noqa: F401
from test_contfit import (OK, NONPOSITIVE, TOO_FEW, SINGULAR, NAN, BAD_MODEL, SENTINEL, SHAPES, LONG, NCLIP, CLIP_N, MARGIN, ALT_P, ALT_ROUNDS, ALT_STARS,
                          aligned, unaligned, contfit_case, shape_cases, oracle, compare, clip_case, status_case, alternation_inputs,
                          alternation_reference, reference_alternation)

pytestmark = pytest.mark.gpu
XTOL = DEFAULTS["xtol"]
KEYS = ("coef", "chisq", "npix", "status", "rounds", "flux_out", "w_out")


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


class OnDevice(object):
    """A case's arrays on the device, uploaded once."""

    def __init__(self, case):
        self.case = case
        self.flux, self.w, self.model, self.x = dev(case["flux"]), dev(case["w"]), dev(case["model"]), dev(case["x"])
        self.index = None if case["index"] is None else dev(case["index"])


def run_abi(lib, d, nclip=0, kappa=(3.0, 3.0), rescale=False, drop_clipped=True, star=None, rows=True):
    """payne_contfit_batch on the case (or on its star `star` alone, through offset pointers) with every output pre-filled with the
    sentinel -> compare's dict.  The coefficients have a row of sentinels behind them."""
    import torch
    case = d.case
    n, P = case["n"], case["P"]
    ld_f, ld_m, ld_o = case["lds"]
    b0, N = (0, case["N"]) if star is None else (star, 1)
    M = d.model.shape[0]
    model, n_models = (d.model[b0:], M - b0) if d.index is None else (d.model, M)
    coef = torch.full((N + 1, P), SENTINEL, dtype=torch.float64, device="cuda:0")
    chisq = torch.full((N + 1,), SENTINEL, dtype=torch.float64, device="cuda:0")
    ints = torch.full((3, N + 1), -77, dtype=torch.int32, device="cuda:0")
    fo = torch.full((N, ld_o), SENTINEL, dtype=torch.float32, device="cuda:0")
    wo = torch.full((N, ld_o), SENTINEL, dtype=torch.float64, device="cuda:0")
    o = _lib.ContfitOpts(P=P, nclip=nclip, rescale=rescale, drop_clipped=drop_clipped, kappa_lo=kappa[0], kappa_hi=kappa[1])
    rc = lib.payne_contfit_batch(0, d.flux[b0:].data_ptr(), d.w[b0:].data_ptr(), ld_f, model.data_ptr(), ld_m, n_models,
                                 None if d.index is None else d.index[b0:].data_ptr(), d.x.data_ptr(), N, n, C.byref(o), coef.data_ptr(), chisq.data_ptr(),
                                 ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), fo.data_ptr() if rows else None, wo.data_ptr() if rows else None, ld_o, None)
    assert rc == 0, (rc, lib.payne_last_error(None))
    torch.cuda.synchronize()
    coef, chisq, ints = coef.cpu().numpy(), chisq.cpu().numpy(), ints.cpu().numpy()
    assert np.all(coef[N] == SENTINEL) and chisq[N] == SENTINEL and np.all(ints[:, N] == -77)
    return dict(coef=coef[:N], chisq=chisq[:N], npix=ints[0, :N], status=ints[1, :N], rounds=ints[2, :N], flux_out=fo.cpu().numpy(), w_out=wo.cpu().numpy())


def same_bytes(a, b, n, what, rows=slice(None)):
    for k in KEYS:
        x, y = a[k][rows], b[k]
        if k in ("flux_out", "w_out"):
            x, y = x[..., :n], y[..., :n]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, k)


def relaid(case, lds):
    """The same values in arrays of other leading dimensions."""
    n = case["n"]
    out = dict(case, lds=lds)
    for k, ld, fill in (("flux", lds[0], np.float32(1e30)), ("w", lds[0], 1e30), ("model", lds[1], np.float32(1e30))):
        a = np.full((case[k].shape[0], ld), fill, dtype=case[k].dtype)
        a[:, :n] = case[k][:, :n]
        out[k] = a
    return out


# ---- 1. the cases of the host tests through the ABI -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", SHAPES + [LONG])
def test_cases_through_the_abi(lib, n, P):
    ratios = {}
    cases = list(shape_cases(n, P)) if (n, P) != LONG else [contfit_case(np.random.default_rng(9), 2, P, n, unaligned(n))]
    nclip = 2 if (n, P) == LONG else 0
    for case in cases:
        orc = oracle(case, nclip=nclip)
        d = OnDevice(case)
        got = run_abi(lib, d, nclip=nclip)
        compare(case, got, orc, "ABI", nclip=nclip, ratios=ratios)
        same_bytes(got, run_abi(lib, d, nclip=nclip), n, "a second call")
        # the other instantiation (16-byte loads <-> element by element): the same bytes
        other = relaid(case, aligned(n) if case["lds"] == unaligned(n) else unaligned(n))
        d2 = OnDevice(other)
        same_bytes(got, run_abi(lib, d2, nclip=nclip), n, "the other load path")
        # a star alone: the bytes it has in the batch, through either path
        for b in sorted({0, case["N"] // 2, case["N"] - 1}):
            same_bytes(got, run_abi(lib, d, nclip=nclip, star=b), n, ("alone", b), rows=slice(b, b + 1))
            same_bytes(got, run_abi(lib, d2, nclip=nclip, star=b), n, ("alone, other path", b), rows=slice(b, b + 1))
        # without output rows: the same coefficients and statuses
        bare = run_abi(lib, d, nclip=nclip, rows=False)
        assert all(bare[k].tobytes() == got[k].tobytes() for k in KEYS[:5]) and np.all(bare["flux_out"] == np.float32(SENTINEL)) and np.all(bare["w_out"] == SENTINEL)
    print("n=%d P=%d: |dp| / bound (b) = %.3g, |dchi^2| / bound (c) = %.3g" % (n, P, ratios.get("b", 0), ratios.get("c", 0)))


# ---- 2. clipping ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", (False, True), ids=("unit", "rescale"))
@pytest.mark.parametrize("n", CLIP_N)
def test_clipping_masks_are_the_oracle_s_in_every_round(lib, n, rescale):
    """nclip = r stops after the oracle's round r, and the rows' zero weights are that round's mask: r = 0 .. NCLIP walks every round."""
    case, full = clip_case(n, rescale)
    assert min(o["margin"] for o in full) >= MARGIN
    for lds in (unaligned(n), aligned(n)):
        d = OnDevice(relaid(case, lds))
        for r in range(NCLIP + 1):
            orc = oracle(d.case, nclip=r, rescale=rescale)
            got = run_abi(lib, d, nclip=r, rescale=rescale)
            compare(d.case, got, orc, "ABI nclip=%d" % r, nclip=r)
            for s, o in enumerate(orc):
                counting = d.case["w"][s, :n] != 0
                assert np.array_equal(got["w_out"][s, :n] != 0, o["masks"][-1]) and got["npix"][s] == o["masks"][-1].sum() and got["rounds"][s] == o["rounds"]
                assert r == 0 or (counting & ~o["masks"][-1]).any()
            if r == NCLIP:
                kept = run_abi(lib, d, nclip=r, rescale=rescale, drop_clipped=False)
                compare(d.case, kept, orc, "ABI keep", nclip=r, drop_clipped=False)
                assert all(np.array_equal(kept["w_out"][s, :n] != 0, d.case["w"][s, :n] != 0) for s in range(d.case["N"]))
                assert all(kept[k].tobytes() == got[k].tobytes() for k in ("coef", "chisq", "npix", "status", "rounds", "flux_out"))


# ---- 3. statuses ----------------------------------------------------------------------------------------------------------------------
def test_statuses(lib):
    case = status_case()
    n = case["n"]
    for lds in (unaligned(n), aligned(n)):
        c1 = relaid(case, lds)
        got, orc = run_abi(lib, OnDevice(c1)), oracle(c1)
        assert list(got["status"]) == [OK, TOO_FEW, SINGULAR, NAN, OK, NAN, NONPOSITIVE]
        compare(c1, got, orc, "ABI")
        assert np.all(np.isfinite(got["coef"][6])) and got["npix"][1] == 3 and got["rounds"][1] == 0
        idx = np.arange(7, dtype=np.int32)
        idx[1], idx[4] = -1, 7
        c2 = dict(c1, index=idx)
        got2 = run_abi(lib, OnDevice(c2))
        assert list(got2["status"]) == [OK, BAD_MODEL, SINGULAR, NAN, BAD_MODEL, NAN, NONPOSITIVE]
        compare(c2, got2, oracle(c2), "ABI")
        for s in (0, 2, 3, 5, 6):                                     # the neighbours are as before
            same_bytes(got2, {k: got[k][s:s + 1] for k in KEYS}, n, ("neighbour", s), rows=slice(s, s + 1))
    # TOO_FEW after a clip (tests/test_contfit.py: test_too_few_after_a_clip_on_the_host)
    P = 4
    case = contfit_case(np.random.default_rng(3), 3, P, n, unaligned(n), noise=1e-4)
    w, f = case["w"], case["flux"]
    w[1, :n] = 0.0
    w[1, [3, 11, 19, 27, 35]] = 1e4
    f[1, [3, 11, 19, 27, 35]], case["model"][1, [3, 11, 19, 27, 35]] = 1.3, 1.0
    f[1, 11] += 5.0
    f[1, 27] -= 5.0
    got, orc = run_abi(lib, OnDevice(case), nclip=3, kappa=(0.5, 0.5)), oracle(case, nclip=3, kappa=(0.5, 0.5))
    assert orc[1]["status"] == TOO_FEW and orc[1]["rounds"] >= 1 and min(o["margin"] for o in orc) >= MARGIN
    compare(case, got, orc, "ABI", nclip=3)


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------------
def test_invalid_and_unsupported_arguments(lib):
    import torch
    N, n, P = 2, 8, 3
    inv, uns = _lib.E_INVALID, _lib.E_UNSUPPORTED
    bufs = dict(flux=dev(np.ones((N, n), dtype=np.float32)), w=dev(np.ones((N, n))), model=dev(np.ones((N, n), dtype=np.float32)), x=dev(np.linspace(-1, 1, n)),
                index=dev(np.zeros(N, dtype=np.int32)), coef=torch.full((N, P), SENTINEL, dtype=torch.float64, device="cuda:0"),
                chisq=torch.full((N,), SENTINEL, dtype=torch.float64, device="cuda:0"), npix=torch.full((N,), -77, dtype=torch.int32, device="cuda:0"),
                status=torch.full((N,), -77, dtype=torch.int32, device="cuda:0"), rounds=torch.full((N,), -77, dtype=torch.int32, device="cuda:0"),
                fo=torch.full((N, n), SENTINEL, dtype=torch.float32, device="cuda:0"), wo=torch.full((N, n), SENTINEL, dtype=torch.float64, device="cuda:0"))

    def call(N=N, n=n, ld_f=n, ld_m=n, ld_o=n, n_models=N, opts=True, null=(), **okw):
        p = {k: (None if k in null else v.data_ptr()) for k, v in bufs.items()}
        if "index" not in okw.pop("use", ("index",)):
            p["index"] = None
        o = _lib.ContfitOpts(**dict(dict(P=P), **okw))
        return lib.payne_contfit_batch(0, p["flux"], p["w"], ld_f, p["model"], ld_m, n_models, p["index"], p["x"], N, n, C.byref(o) if opts else None,
                                       p["coef"], p["chisq"], p["npix"], p["status"], p["rounds"], p["fo"], p["wo"], ld_o, None)
    assert call(opts=False) == inv                                                             # null opts
    assert call(P=0) == inv and call(P=16) == inv                                              # P outside 1 .. 15
    assert call(nclip=-1) == inv and call(nclip=17) == inv                                     # nclip outside 0 .. 16
    assert call(kappa_lo=0.0) == inv and call(kappa_hi=-1.0) == inv and call(kappa_lo=float("nan")) == inv   # a kappa that is not positive
    assert call(N=-1) == inv and call(n=0) == inv                                              # N < 0, n < 1
    assert call(ld_f=n - 1) == inv and call(ld_m=n - 1) == inv and call(ld_o=n - 1) == inv     # a leading dimension below n
    assert call(n_models=0) == inv and call(n_models=N - 1, use=()) == inv                     # n_models < 1; < N without an index
    for name in ("flux", "w", "model", "x", "coef", "chisq", "npix", "status", "rounds"):
        assert call(null=(name,)) == inv, name                                                 # a null pointer with N > 0
    assert call(n=_lib.CONTFIT_MAX_N + 1, ld_f=_lib.CONTFIT_MAX_N + 1, ld_m=_lib.CONTFIT_MAX_N + 1, ld_o=_lib.CONTFIT_MAX_N + 1) == uns
    assert b"262144" in lib.payne_last_error(None)
    torch.cuda.synchronize()
    for k in ("coef", "chisq", "fo", "wo"):
        assert np.all(bufs[k].cpu().numpy() == SENTINEL)                                       # none of the refused calls ran
    assert np.all(bufs["status"].cpu().numpy() == -77)
    assert call(N=0, null=tuple(bufs)) == 0                                                    # N == 0 succeeds and does nothing
    assert call(n_models=1) == 0 and call(null=("fo",)) == 0 and call(null=("wo",)) == 0 and call(null=("fo", "wo"), ld_o=0) == 0 and call(kappa_hi=float("inf")) == 0
    torch.cuda.synchronize()
    assert np.all(bufs["status"].cpu().numpy() == OK)


# ---- 5. ContinuumFit ------------------------------------------------------------------------------------------------------------------
def fit_inputs(n=1000, N=5, P=4, seed=5):
    case = contfit_case(np.random.default_rng(seed), N, P, n, (n, n, n))
    wave = 5000.0 + np.cumsum(np.random.default_rng(n).uniform(0.5, 1.5, n))
    eflux = np.where(case["w"] != 0, 1.0 / np.sqrt(np.where(case["w"] != 0, case["w"], 1.0)), 0.0)
    eflux[0, 7] = np.inf
    return case, wave, eflux


def test_fit_from_numpy_and_from_device_tensors_agree(lib):
    import torch
    from thepayne_amd.fitting.contfit import ContinuumFit
    from thepayne_amd.fitting import fitutils
    case, wave, eflux = fit_inputs()
    n, N = case["n"], case["N"]
    cf = ContinuumFit(wave, npoly=4, nclip=2)
    a = cf.fit(case["flux"], eflux, case["model"])
    b = cf.fit(dev(case["flux"]), dev(eflux), dev(case["model"]))
    assert all(isinstance(v, np.ndarray) for v in a.values()) and all(isinstance(v, torch.Tensor) for v in b.values())
    assert set(a) == {"coef", "chisq", "npix", "status", "rounds", "flux", "eflux", "weights"} == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].cpu().numpy().tobytes(), k
    mixed = cf.fit(case["flux"], eflux, dev(case["model"]))
    assert all(a[k].tobytes() == mixed[k].cpu().numpy().tobytes() for k in a)
    assert np.all(a["status"] == OK) and a["coef"].shape == (N, 4) and a["flux"].dtype == np.float32 and a["npix"][0] <= (eflux[0] != 0).sum() - 1
    wts = a["weights"]
    assert np.array_equal(a["eflux"] == 0, wts == 0) and np.allclose(a["eflux"][wts > 0], 1.0 / np.sqrt(wts[wts > 0]), rtol=1e-14) and a["eflux"][0, 7] == 0
    # the raw call on the same weights gives the same bytes
    w = np.where(np.isfinite(eflux) & (eflux != 0), 1.0 / np.where(eflux != 0, eflux, 1.0) ** 2, 0.0)
    raw = run_abi(lib, OnDevice(dict(case, w=w, x=cf.x)), nclip=2)
    assert raw["coef"].tobytes() == a["coef"].tobytes() and raw["flux_out"].tobytes() == a["flux"].tobytes() and raw["w_out"].tobytes() == a["weights"].tobytes()
    # polycalc's basis and abscissa
    for s in range(N):
        ok = (wts[s] != 0) & (case["flux"][s] != 0)
        p = fitutils.polycalc(a["coef"][s], wave)
        q = case["flux"][s][ok].astype(np.float64) / a["flux"][s][ok].astype(np.float64)
        assert np.all(np.abs(q - p[ok]) <= 2.0 ** -23 * np.abs(p[ok]))
    bare = cf.fit(case["flux"], eflux, case["model"], normalise=False)
    assert set(bare) == {"coef", "chisq", "npix", "status", "rounds"} and bare["coef"].tobytes() == a["coef"].tobytes()
    # [M, nobs] with an index, repeated and out of range
    idx = np.array([2, 2, 0, 9, -3])
    c = cf.fit(case["flux"], eflux, case["model"][:3], index=idx)
    g = cf.fit(case["flux"], eflux, case["model"][np.clip(idx, 0, 2)])
    assert list(c["status"][3:]) == [BAD_MODEL, BAD_MODEL] and all(c[k][:3].tobytes() == g[k][:3].tobytes() for k in c)
    assert np.all(np.isnan(c["coef"][3:])) and not c["eflux"][3:].any() and np.array_equal(c["flux"][3:], case["flux"][3:])


def small_bank(g20, nobs=64):
    from thepayne_amd.fitting.tmatch import TemplateBank
    net, nntype = recovery_net(g20, "smlp")
    wave = net["wavelength"]
    width = wave[-1] - wave[0]
    obs_wave = np.linspace(wave[0] + 0.2 * width, wave[-1] - 0.2 * width, nobs)
    bank = TemplateBank(net, nntype, obs_wave, b_max=16)
    return obs_wave, bank.lattice((2, 2, 2, 1, 1)[:bank.n_labels], vrad=(-30.0, 0.0, 30.0), vrot=(10.0,), inst_R=(20000.0,), inner=(0.1, 0.9))


def test_fit_to_bank_reads_the_templates_in_place(g20):
    import torch
    from thepayne_amd.fitting.contfit import ContinuumFit, abscissa
    from numpy.polynomial.chebyshev import chebvander
    obs_wave, bank = small_bank(g20)
    nobs, M, N = len(obs_wave), len(bank), 9
    rng = np.random.default_rng(8)
    tpl = bank.templates.cpu().numpy()
    pick = rng.integers(0, M, N)
    coef = np.concatenate([rng.uniform(0.9, 1.1, (N, 1)), rng.uniform(-0.02, 0.02, (N, 2))], axis=1)
    flux = (tpl[pick] * (chebvander(abscissa(obs_wave), 2) @ coef.T).T + 0.002 * rng.normal(0, 1, (N, nobs))).astype(np.float32)
    eflux = np.full((N, nobs), 0.002)
    cf = ContinuumFit(obs_wave, npoly=3)
    for rank in (0, 1):
        m = bank.match(flux, eflux, topk=2)
        m = dict(m, index=np.where(np.arange(N)[:, None] == 4, -1, m["index"]).astype(np.int32))     # star 4: no template
        res = cf.fit_to_bank(flux, eflux, bank, match=m, rank=rank)
        assert m["index"][4, rank] == -1 and res["status"][4] == BAD_MODEL and all(isinstance(v, np.ndarray) for v in res.values())
        idx = m["index"][:, rank]
        good = idx >= 0
        ref = cf.fit(flux[good], eflux[good], tpl[idx[good]])
        assert all(res[k][good].tobytes() == ref[k].tobytes() for k in ref), rank
        if rank == 0:
            own = cf.fit_to_bank(flux, eflux, bank)                    # runs the search itself
            assert all(own[k][good].tobytes() == res[k][good].tobytes() for k in res) and own["status"][4] == OK
            assert np.all(res["status"][good] == OK) and np.all(res["npix"][good] == nobs)
    with pytest.raises(ValueError):
        ContinuumFit(obs_wave[:-1], npoly=3).fit_to_bank(flux, eflux, bank)
    with pytest.raises(TypeError):
        cf.fit_to_bank(flux, eflux, object())
    out = cf.fit_to_bank(torch.as_tensor(flux), eflux, bank)
    assert isinstance(out["coef"], torch.Tensor)


# ---- 6. OptFit.fit_with_continuum -------------------------------------------------------------------------------------------------------
def test_fit_with_continuum_against_the_reference_alternation(g20):
    """The inputs of test_reference_alternation_recovers_the_truth: recovery stars times a P = 4 series.  The device's alternation
    stays within the yardstick of the fp64 reference alternation at the last round; plain OptFit.fit on the same un-normalised
    spectra ends at least 10 x that far from it (the factor found is printed)."""
    import torch
    from thepayne_amd.fitting.optfit import OptFit
    net, nntype, case, coef, flux, x = alternation_inputs(g20)
    refs = alternation_reference(g20)
    cols, S = case["cols"], ALT_STARS
    fit = OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX)
    f32 = flux.astype(np.float32)
    res = fit.fit_with_continuum(f32, case["eflux"][:S], case["start"][:S], npoly=ALT_P, rounds=ALT_ROUNDS)
    plain = fit.fit(f32, case["eflux"][:S], case["start"][:S])
    assert res["coef"].shape == (S, ALT_P) and res["chisq_rounds"].shape == (S, ALT_ROUNDS) and np.all(res["cont_status"] == OK)
    assert np.all(np.isfinite(res["chisq_rounds"])) and np.array_equal(res["chisq_rounds"][:, -1], res["chisq"])
    from numpy.polynomial.chebyshev import chebvander
    V = chebvander(x, ALT_P - 1)
    factors = []
    for i in range(S):
        r64, c64, _ = refs[i]
        r32, _, _ = reference_alternation(net, nntype, case, i, flux[i], x, rounds=3, dtype=torch.float32, start=r64["x"])
        d = sigma_distance(res["pars"][i, cols], r64["x"], r64["A"])
        d32 = sigma_distance(r32["x"], r64["x"], r64["A"])
        dplain = sigma_distance(plain["pars"][i, cols], r64["x"], r64["A"])
        bound = max(10.0 * XTOL, 4.0 * d32)
        factors.append(dplain / bound)
        print("star %d: d = %.3g sigma (bound %.3g; the fp32-fed loop's %.3g); plain fit %.3g sigma, %.3g x the bound; polynomial off the reference's by %.3g"
              % (i, d, bound, d32, dplain, dplain / bound, np.abs(V @ (res["coef"][i] - c64)).max()))
        assert d <= bound, (i, d, d32)
        assert dplain >= 10.0 * bound, (i, dplain, bound)
    print("plain OptFit.fit ends %.3g .. %.3g x the bound from the reference" % (min(factors), max(factors)))
    # a star whose spectrum is NaN at a counting pixel keeps cont_status NAN and NaN labels; its neighbours are as before
    bad = f32.copy()
    bad[1, 10] = np.nan
    res2 = fit.fit_with_continuum(bad, case["eflux"][:S], case["start"][:S], npoly=ALT_P, rounds=2)
    assert res2["cont_status"][1] == NAN and np.all(np.isnan(res2["pars"][1, cols])) and np.all(res2["cont_status"][[0, 2]] == OK)
    res3 = fit.fit_with_continuum(f32, case["eflux"][:S], case["start"][:S], npoly=ALT_P, rounds=2)
    assert all(np.asarray(res2[k])[[0, 2]].tobytes() == np.asarray(res3[k])[[0, 2]].tobytes() for k in ("pars", "chisq", "coef", "chisq_rounds"))
