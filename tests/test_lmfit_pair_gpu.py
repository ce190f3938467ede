"""Two-component spectra in one Levenberg-Marquardt fit on the device: payne_lmfit_update_pair through the C ABI and
OptFit.fit_binary end to end.  The inputs, the references and the bounds are tests/test_lmfit_pair.py's, which checks on the CPU that
the fp64 reference loop on the mixed model converges on the inputs fitted here.

Yardstick of fit_binary: d = max_k |x - x*| sqrt(A*_kk) over all K parameters, x* and A* the fp64 reference loop's, stays within 1e-2
(10 xtol, the project's bound for device fits); the same numpy loop fed with torch's CPU fp32 models and Jacobians is printed next to
it."""
import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import DEFAULTS, RUNNING, CONVERGED, STEP_TOL, RECOVERY_BMAX, RECOVERY_MAX_EVALS, g20, sigma_distance                          # noqa: F401
from test_lmfit_poly import BIG
from test_lmfit_poly_gpu import handle, dev, state_of, tile_of, relaid, x_on_device, lib                                                       # noqa: F401
from test_lmfit_pair import (SHAPES, SHAPE_IDS, LINEAR_N, BINARY_CASES, BINARY_PAIRS, pair_case, check_pair_tiles, pair_emul, start_of,       # noqa: F401
                             linear_case, check_linear, binary_inputs, binary_fit, binary_reference, STATE_CASES, STATE_IDS, state_case)

pytestmark = pytest.mark.gpu


def update_pair(lib, h, case, rows_a, rows_b, ld, flux, w, ld_f, x, b0=0):
    """payne_lmfit_update_pair on device tensors from star b0 on."""
    Kl = case["Kl"]
    ia, ib = np.ascontiguousarray(case["ia"], dtype=np.int32), np.ascontiguousarray(case["ib"], dtype=np.int32)
    return lib.payne_lmfit_update_pair(h._h, Kl, case["P"], ia.ctypes.data if Kl else None, ib.ctypes.data if Kl else None, rows_a[b0:].data_ptr(), case["Ka"],
                                       rows_b[b0:].data_ptr(), case["Kb"], ld, flux[b0:].data_ptr(), w[b0:].data_ptr(), ld_f,
                                       x.data_ptr() if case["P"] else None, case["n"], None)


# ---- 1. the sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ka,Kb,tied,P", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n", (5, 37, 1000))
def test_sums_through_the_abi(lib, Ka, Kb, tied, P, n):
    """The first evaluation is always accepted, so A, g and chi^2 are the tile.  Three stars against the einsum; 30 stars for the
    bytes: a second call, a star alone, the other load form."""
    import torch
    B = 30
    case = pair_case(np.random.default_rng(100000 * Ka + 1000 * Kb + 100 * P + n), B, Ka, Kb, tied, P, n, n + 3, n + 6)
    K = case["Kl"] + 1 + P
    x0, lo, hi = start_of(case)
    first = None
    for ld, ld_f, xoff in ((n + 3, n + 6, 1), ((n + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8, 0)):          # element by element; 16 bytes a lane
        ra_d, rb_d = dev(relaid(case["rows_a"], ld, n, np.float32(1e30))), dev(relaid(case["rows_b"], ld, n, np.float32(1e30)))
        flux_d, w_d = dev(relaid(case["flux"], ld_f, n, np.float32(1e30))), dev(relaid(case["w"], ld_f, n, 1e30))
        x_d = x_on_device(case["x"], xoff)
        h = handle(K, B)

        def run(b0=0, nb=B):
            h.begin(x0[b0:b0 + nb], lo, hi)
            assert update_pair(lib, h, case, ra_d, rb_d, ld, flux_d, w_d, ld_f, x_d, b0) == 0
            torch.cuda.synchronize()
            return state_of(h)
        st = run()
        G = tile_of(st, K)
        check_pair_tiles(G[:3], case, "ABI ld=%d" % ld, stars=range(3))
        assert np.array_equal(st["A"], np.swapaxes(st["A"], 1, 2)) and np.all(st["niter"] == 1)
        assert np.all(np.isfinite(G)) and np.all(G[:, K, K] > 0)                                     # (star 1 holds NaN under w == 0 only)
        again = run()
        assert all(again[k].tobytes() == st[k].tobytes() for k in st)                                # a second call: the same bytes
        for b in (0, 1, B // 2, B - 1):                                                              # a star alone: the same bytes as in the batch
            one = run(b, 1)
            assert all(one[k][0].tobytes() == st[k][b].tobytes() for k in st), (b,)
        if first is None:
            first = st
        else:
            assert all(first[k].tobytes() == st[k].tobytes() for k in st)                            # both load forms: the same bits
        h.close()


# ---- 2. against the emulator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ka,Kb,tied,P,n", STATE_CASES, ids=STATE_IDS)
def test_state_after_each_step_is_the_emulator_s(lib, pair_emul, Ka, Kb, tied, P, n):
    """Three updates on fresh random rows each: after every one the device's state is the emulator's -- status, evaluations, lambda and
    at_bound exactly, x_trial (whose entries from K_l on are the next update's ratio and coefficients) and x_best within STEP_TOL.
    The cases are tests/test_lmfit_pair.py's STATE_CASES, on which it shows without a GPU that two orders of the sums leave a step
    within a quarter of STEP_TOL."""
    import torch
    B = 3
    case, updates = state_case(Ka, Kb, tied, P, n)
    K = case["Kl"] + 1 + P
    x0, lo, hi = start_of(case)
    begin_e, Gs_e, states_e = pair_emul(x0, lo, hi, case, updates)
    h = handle(K, B)
    h.begin(x0, lo, hi)
    flux_d, w_d, x_d = dev(case["flux"]), dev(case["w"]), dev(case["x"])
    for t, (ra, rb) in enumerate(updates):
        ra_d, rb_d = dev(ra), dev(rb)
        assert update_pair(lib, h, case, ra_d, rb_d, n + 3, flux_d, w_d, n + 6, x_d) == 0
        torch.cuda.synchronize()
        st, se = state_of(h), states_e[t]
        for key in ("status", "niter", "at_bound", "lam"):
            assert np.array_equal(st[key], se[key]), (t, key, st[key], se[key])
        for b in range(B):
            assert np.all(np.isfinite(se["A"][b])) and np.all(np.diag(se["A"][b]) > 0)
            sig = 1.0 / np.sqrt(np.diag(se["A"][b]))
            err = np.abs(st["x_trial"][b] - se["x_trial"][b]) / sig
            errb = np.abs(st["x_best"][b] - se["x_best"][b]) / sig
            print("Kl=%d P=%d n=%d update %d star %d: status %d, |x_trial - emulator's| = %.3g sigma at most" % (case["Kl"], P, n, t, b, st["status"][b], err.max()))
            assert err.max() <= STEP_TOL and errb.max() <= STEP_TOL, (t, b, err.max(), errb.max())
    assert np.all(states_e[-1]["niter"] >= 1)
    h.close()


# ---- 3. a linear model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LINEAR_N)
def test_one_gauss_newton_step_solves_the_ratio(lib, n):
    """K = 1, lambda0 = lambda_min = 0: one update through LMHandle.update_pair from any q lands on q* within the CPU test's bound."""
    import torch
    case = linear_case(n)
    h = handle(1, case["B"], lambda0=0.0, lambda_min=0.0, xtol=0.0)
    h.begin(case["q"][:, None], np.array([-BIG]), np.array([BIG]))
    cut = lambda a: dev(np.ascontiguousarray(a[..., :n]))            # noqa: E731
    h.update_pair(cut(case["rows_a"]), cut(case["rows_b"]), cut(case["flux"]), cut(case["w"]), [], [])
    torch.cuda.synchronize()
    st = state_of(h)
    h.close()
    assert np.all(st["status"] == RUNNING) and np.all(st["lam"] == 0.0) and np.all(st["at_bound"] == 0)
    check_linear(case, st["x_trial"][:, 0], "device")


# ---- 4. OptFit.fit_binary -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nobs,tie,P", BINARY_CASES, ids=["n%d-tie%d-P%d" % (c[0], len(c[1]), c[2]) for c in BINARY_CASES])
def test_fit_binary_against_the_reference_loop(g20, nobs, tie, P):
    import torch
    from thepayne_amd.fitting.optfit import OptFit
    inp = binary_inputs(g20, nobs, tie, P)
    refs = binary_reference(g20, nobs, tie, P)
    S, a = BINARY_PAIRS, inp["args"]
    cols, Ka, Kl, b_pos = a["cols"], a["Ka"], a["Kl"], a["b_pos"]
    K = Kl + 1 + P
    free_b = [k for k in range(Ka) if b_pos[k] >= Ka]
    fit = OptFit(inp["net"], inp["nntype"], inp["obs_wave"], b_max=RECOVERY_BMAX)
    kw = dict(ratio=inp["q0"], tie=tie, npoly=P)

    def z_of(res, i):
        return np.concatenate([res["pars_a"][i, cols], res["pars_b"][i, [cols[k] for k in free_b]], [res["ratio"][i]], res["coef"][i]])
    res = fit.fit_binary(inp["flux"], inp["eflux"], inp["start_a"], inp["start_b"], **kw)
    assert res["pars_a"].shape == (S, 8) and res["pars_b"].shape == (S, 8) and res["ratio"].shape == (S,) and res["coef"].shape == (S, P)
    assert res["fisher"].shape == (S, K, K) and res["err"].shape == (S, K) and res["labels"] == a["names"] and np.all(res["npix"] == nobs)
    other = [c for c in range(8) if c not in cols]
    assert np.array_equal(res["pars_a"][:, other], inp["start_a"][:, other], equal_nan=True) and np.array_equal(res["pars_b"][:, other], inp["start_b"][:, other], equal_nan=True)
    tied_cols = [cols[k] for k in range(Ka) if b_pos[k] < Ka]
    assert np.array_equal(res["pars_b"][:, tied_cols], res["pars_a"][:, tied_cols]) and len(tied_cols) == len(tie)
    for i in range(S):
        r64 = refs[i]
        r32 = binary_fit(g20, i, nobs, tie, P, dtype=torch.float32)
        d, d32 = sigma_distance(z_of(res, i), r64["x"], r64["A"]), sigma_distance(r32["x"], r64["x"], r64["A"])
        print("nobs=%d tie=%s P=%d pair %d: status %d after %d evaluations (reference: %d), d = %.3g sigma (bound 1e-2; the fp32-fed loop's %.3g), q = %.6f"
              % (nobs, tie, P, i, res["status"][i], res["niter"][i], r64["niter"], d, d32, res["ratio"][i]))
        assert res["status"][i] == CONVERGED and res["niter"][i] <= RECOVERY_MAX_EVALS, (i, res["status"][i], res["niter"][i])
        assert d <= 1e-2, (i, d, d32)
        assert np.all(np.isfinite(res["err"][i])) and np.all(res["err"][i] >= 1.0 / np.sqrt(np.diag(res["fisher"][i])) * (1.0 - 1e-12))   # marginal >= conditional
    # b_max 16 holds one pair's rows: four pairs are four chunks, and each pair's bytes are those of the pair alone
    keys = ("pars_a", "pars_b", "ratio", "coef", "chisq", "fisher", "status", "niter", "at_bound", "err")
    for i in (0, S - 1):
        one = fit.fit_binary(inp["flux"][i:i + 1], inp["eflux"][i:i + 1], inp["start_a"][i:i + 1], inp["start_b"][i:i + 1], **dict(kw, ratio=inp["q0"][i:i + 1]))
        for key in keys:
            assert np.asarray(one[key][0]).tobytes() == np.asarray(res[key][i]).tobytes(), (i, key)
    big = OptFit(inp["net"], inp["nntype"], inp["obs_wave"], b_max=64)                             # three pairs a chunk: the same bytes again
    res_b = big.fit_binary(inp["flux"], inp["eflux"], inp["start_a"], inp["start_b"], **kw)
    assert all(np.asarray(res_b[key]).tobytes() == np.asarray(res[key]).tobytes() for key in keys)
    if (nobs, tie, P) in BINARY_CASES[:2]:
        # a spectrum that is NaN at a counting pixel: status NAN and NaN results, the neighbours as before (with and without a polynomial)
        bad = inp["flux"].copy()
        bad[1, 10] = np.nan
        res2 = fit.fit_binary(bad, inp["eflux"], inp["start_a"], inp["start_b"], **kw)
        assert res2["status"][1] == _lib.LMFIT_NAN and np.all(np.isnan(res2["pars_a"][1, cols])) and np.all(np.isnan(res2["pars_b"][1, cols])) and np.isnan(res2["ratio"][1])
        assert np.all(np.isnan(res2["coef"][1])) and np.all(np.isnan(res2["fisher"][1])) and np.all(np.isnan(res2["err"][1])) and np.isnan(res2["chisq"][1])
        assert all(np.asarray(res2[k])[[0, 2, 3]].tobytes() == np.asarray(res[k])[[0, 2, 3]].tobytes() for k in keys)
    if (nobs, tie, P) == BINARY_CASES[1]:
        # given coefficients: the same fit; the method's own ValueErrors
        from thepayne_amd.fitting.contfit import ContinuumFit
        q = torch.as_tensor(inp["q0"]).to("cuda:0")[:, None]
        sb = inp["start_b"].copy()
        mixed = ((1.0 - q) * fit.model_spectra(inp["start_a"]) + q * fit.model_spectra(sb)).to(torch.float32).contiguous()
        c0 = ContinuumFit(inp["obs_wave"], npoly=P).fit(inp["flux"], inp["eflux"], mixed, normalise=False)["coef"]
        given = fit.fit_binary(inp["flux"], inp["eflux"], inp["start_a"], inp["start_b"], coef=c0, **kw)
        assert all(np.asarray(given[k]).tobytes() == np.asarray(res[k]).tobytes() for k in keys)
        for badkw in (dict(npoly=5), dict(tie=("feh", "afe", "nope")), dict(ratio=0.995), dict(ratio_bounds=(0.0, 0.9)), dict(ratio_bounds=(0.1, 1.0))):
            with pytest.raises(ValueError):
                fit.fit_binary(inp["flux"], inp["eflux"], inp["start_a"], inp["start_b"], **dict(kw, **badkw))


# ---- 5. arguments ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_state_untouched(lib):
    import torch
    Ka, Kb, P, B, n = 2, 3, 2, 2, 8
    ia0, ib0 = np.array([0, 1, -1, 0], dtype=np.int32), np.array([-1, 2, 0, 1], dtype=np.int32)
    Kl = 4
    K = Kl + 1 + P
    inv = _lib.E_INVALID
    h = handle(K, 4)
    x0, lo, hi = dev(np.full((B, K), 0.5)), np.full(K, -10.0), np.full(K, 10.0)
    ra, rb = dev(np.ones((B, 1 + Ka, n), dtype=np.float32)), dev(np.full((B, 1 + Kb, n), 2.0, dtype=np.float32))
    flux, w, x = dev(np.ones((B, n), dtype=np.float32)), dev(np.ones((B, n))), dev(np.linspace(-1, 1, n))
    ptr = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())   # noqa: E731

    def update(h_=h._h, Kl=Kl, P=P, ia=ia0, ib=ib0, ra=ra, Ka=Ka, rb=rb, Kb=Kb, ld=n, flux=flux, w=w, ld_f=n, x=x, n=n):
        return lib.payne_lmfit_update_pair(h_, Kl, P, ptr(ia), ptr(ib), ptr(ra), Ka, ptr(rb), Kb, ld, ptr(flux), ptr(w), ld_f, ptr(x), n, None)
    h.begin(x0, lo, hi)
    torch.cuda.synchronize()
    before = state_of(h)
    assert update(h_=None) == inv                                                            # null handle
    assert update(n=0) == inv and update(ld=n - 1) == inv and update(ld_f=n - 1) == inv      # n < 1, ld < n, ld_f < n
    assert update(Kl=-1) == inv and update(P=-1) == inv and update(P=P + 1) == inv and update(Kl=Kl - 1) == inv   # Kl < 0, P < 0, Kl + 1 + P != K
    assert update(Ka=-1) == inv and update(Kb=-1) == inv and update(ia=None) == inv and update(ib=None) == inv    # Ka < 0, Kb < 0, null maps with Kl > 0
    assert update(Ka=1) == inv and update(Kb=2) == inv                                       # an index beyond its block
    assert update(ia=np.array([0, 1, -2, 0], dtype=np.int32)) == inv and update(ib=np.array([-1, 3, 0, 1], dtype=np.int32)) == inv
    assert update(ia=np.array([0, -1, -1, 0], dtype=np.int32), ib=np.array([-1, -1, 0, 1], dtype=np.int32)) == inv   # both -1 for parameter 1
    assert update(ra=None) == inv and update(rb=None) == inv and update(flux=None) == inv and update(w=None) == inv   # null pointers with B > 0
    assert update(x=None) == inv                                                             # null x_dev with P > 0 and B > 0
    torch.cuda.synchronize()
    after = state_of(h)
    assert all(np.array_equal(after[k], before[k]) for k in before) and np.all(after["niter"] == 0)   # none of the refused calls ran
    for bad in (dict(P=P + 1), dict(ia=ia0[:3]), dict(ia=np.array([0, 2, -1, 0])), dict(ia=np.array([0, -1, -1, 0]), ib=np.array([-1, -1, 0, 1])),
                dict(x=x[:-1]), dict(x=None), dict(rb=rb[:, :, :-1]), dict(flux=flux[:1]), dict(w=w.to(torch.float32))):
        kw = dict(dict(ra=ra, rb=rb, flux=flux, w=w, ia=ia0, ib=ib0, P=P, x=x), **bad)
        with pytest.raises(ValueError):
            h.update_pair(kw["ra"], kw["rb"], kw["flux"], kw["w"], kw["ia"], kw["ib"], kw["P"], kw["x"])
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 0)
    # B == 0 succeeds and does nothing; the valid call runs; P == 0 takes a null x_dev
    assert lib.payne_lmfit_begin(h._h, None, lo.ctypes.data, hi.ctypes.data, 0, None) == 0 and update(ra=None, rb=None, flux=None, w=None, x=None) == 0
    h.begin(x0, lo, hi)
    assert update() == 0
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 1)
    h.close()
    h = handle(Kl + 1, 4)
    h.begin(x0[:, :Kl + 1].contiguous(), lo[:Kl + 1], hi[:Kl + 1])
    assert update(h_=h._h, P=0, x=None) == 0
    torch.cuda.synchronize()
    assert np.all(state_of(h)["niter"] == 1)
    h.close()


# ---- 6. timing=True of the four fits --------------------------------------------------------------------------------------------
def timed_fit(g20, name):
    """(the OptFit, its stars, the rows a star needs, a call of fit `name` taking timing=): the smallest end-to-end inputs of each fit's
    own test, on a b_max that holds fewer rows than the stars need, so that they walk through the handle in at least two blocks."""
    from thepayne_amd.fitting.optfit import OptFit
    if name == "fit":                                                    # tests/test_lmfit_gpu.py's 37-pixel recovery of smlp
        from test_lmfit import recovery_inputs
        from test_lmfit_gpu import device_spectra
        net, nntype, case, _ = recovery_inputs(g20, "smlp", 37, False)
        fit, N = OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX), 5
        flux = device_spectra(fit, case["truth"][:N])
        return fit, N, 1 + 4, lambda **kw: fit.fit(flux, case["eflux"][:N], case["start"][:N], **kw)
    if name == "fit_joint":
        from test_contfit import ALT_STARS as S
        from test_lmfit_poly import JOINT_CASES, joint_inputs
        nobs, P, fit_vrad = JOINT_CASES[0]
        net, nntype, case, coef, flux, x = joint_inputs(g20, nobs)
        fit = OptFit(net, nntype, case["obs_wave"], b_max=RECOVERY_BMAX)
        f32 = flux.astype(np.float32)
        return fit, S, 1 + len(case["cols"]) + 3 * int(fit_vrad), lambda **kw: fit.fit_joint(f32, case["eflux"][:S], case["start"][:S], npoly=P, fit_vrad=fit_vrad, **kw)
    if name == "fit_specphot":
        from test_lmfit_phot import SP_CASES, specphot_inputs
        from test_lmfit_phot_gpu import fitters
        small = min(sorted(SP_CASES), key=lambda nm: (SP_CASES[nm]["which"] != "smlp") + SP_CASES[nm]["fit_vrad"] + len(SP_CASES[nm]["free"]) + SP_CASES[nm]["P"])   # the fewest parameters
        inp = specphot_inputs(g20, small)
        fit, sed = fitters(inp, small)
        cfg = inp["cfg"]
        return fit, len(inp["flux"]), 1 + inp["Km"] + 2 * int(cfg["fit_vrad"]), lambda **kw: fit.fit_specphot(
            inp["flux"], inp["eflux"], inp["mags"], inp["emags"], inp["start"], inp["phot_start"], sed, free_phot=cfg["free"], npoly=cfg["P"],
            fit_vrad=cfg["fit_vrad"], bounds=inp["bounds"], prior=inp["prior"], **kw)
    nobs, tie, P = BINARY_CASES[0]
    inp = binary_inputs(g20, nobs, tie, P)
    fit = OptFit(inp["net"], inp["nntype"], inp["obs_wave"], b_max=RECOVERY_BMAX)
    return fit, BINARY_PAIRS, 2 * (1 + inp["args"]["Ka"] + 2), lambda **kw: fit.fit_binary(inp["flux"], inp["eflux"], inp["start_a"], inp["start_b"], ratio=inp["q0"],
                                                                                           tie=tie, npoly=P, **kw)


@pytest.mark.parametrize("name", ("fit", "fit_joint", "fit_specphot", "fit_binary"))
def test_timing_changes_no_result_and_times_every_step(g20, name):
    """``timing=True`` puts event pairs round the steps of every iteration and sums them into ``fit.timing``: the arrays that come back
    are those of ``timing=False`` byte for byte, and every step of the fit has a time."""
    fit, N, rows, call = timed_fit(g20, name)
    assert N > max(1, RECOVERY_BMAX // rows)                                                       # at least two blocks
    plain = call(timing=False)
    assert fit.timing is None
    timed = call(timing=True)
    assert sorted(timed) == sorted(plain) and timed["labels"] == plain["labels"]
    for key in plain:
        if key != "labels":
            assert np.array_equal(np.asarray(timed[key]), np.asarray(plain[key]), equal_nan=True), (name, key)
    tm = fit.timing
    print("%s, %d stars: %s" % (name, N, tm))
    assert sorted(tm) == sorted(["network", "broadening", "update", "iterations"] + (["sed"] if name == "fit_specphot" else []))
    assert isinstance(tm["iterations"], int) and tm["iterations"] >= 1
    assert all(np.isfinite(tm[k]) and tm[k] > 0.0 for k in tm if k != "iterations"), tm
