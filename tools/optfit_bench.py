"""Least-squares label fits per second on one GPU: thepayne_amd.fitting.optfit.OptFit (payne_specjac_eval + payne_smooth_batch +
payne_lmfit_update an iteration) against scipy.optimize.least_squares around the numpy oracle's getspec on one CPU core.

    python tools/optfit_bench.py [--stars 4096] [--nobs 3600] [--b-max 2560] [--repeats 5] [--warmup 1] [--scipy-stars 8]
    python tools/optfit_bench.py --npoly 4 [--ref-stars 6] [--alt-rounds 3,10,20,40]     (OptFit.fit_joint: joint_mode below)

    python tools/optfit_bench.py --phot 7 [--npoly 4]                                       (OptFit.fit_specphot: phot_mode below)
    python tools/optfit_bench.py --binary [--npoly 4]                                       (OptFit.fit_binary: binary_mode below)

The workload: SMLP 4-256-256-256-4096 (synth.make_torch_net), 3600 observed pixels, stars drawn in the inner half of the label box
with their own Vrad / Vrot / inst_R, spectra from the model itself plus seeded noise at S/N 100, starts 10 % of the box off the
truth.  A timed unit is one whole ``fit`` (uploads, every iteration, the results back on the host) between two host clocks with a
device synchronisation; the figure is the median of `repeats` fits after `warmup` untimed ones.  The split per iteration comes
from one more fit with event pairs on the stream around the three steps (``fit(timing=True)``).  The update kernel alone is
timed with every star RUNNING (a fresh ``begin`` before each launch, outside the event pair); its bytes are the rows, flux and
weights it reads once, (1 + K) n 4 + n 4 + n 8 a star, against the 8 TB/s HBM peak of the MI355X.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def workload(stars, nobs, seed=3):
    from thepayne_amd import synth
    net = synth.make_torch_net("SMLP", npix=4096, H=(256, 256, 256), seed=22)
    rng = np.random.default_rng(seed)
    span = net["xmax"] - net["xmin"]
    truth = np.full((stars, 8), np.nan)
    truth[:, :4] = net["xmin"] + (0.5 + rng.uniform(-0.25, 0.25, (stars, 4))) * span
    truth[:, 4], truth[:, 5], truth[:, 7] = rng.uniform(-30, 30, stars), rng.uniform(3, 30, stars), rng.uniform(15000.0, 30000.0, stars)
    start = truth.copy()
    start[:, :4] += 0.1 * span * rng.choice([-1.0, 1.0], (stars, 4))
    return net, synth.obs_grid(net["wavelength"], nobs), truth, start, rng


def scipy_side(net, obs_wave, flux, eflux, start, n):
    """scipy.optimize.least_squares (trf, 2-point differences, the same box) around the numpy oracle's getspec: seconds a star."""
    from scipy.optimize import least_squares
    import oracle.payne_oracle as PO
    secs, nfev = [], []
    for i in range(n):
        fixed = start[i]
        ok = np.isfinite(flux[i])

        def resid(x):
            m = PO.getspec(net, Teff=x[0], logg=x[1], feh=x[2], afe=x[3], rad_vel=fixed[4], rot_vel=fixed[5], inst_R=float(fixed[7]), outwave=obs_wave)[1]
            return np.where(ok & np.isfinite(m), (flux[i] - m) / eflux[i], 0.0)
        t0 = time.perf_counter()
        r = least_squares(resid, start[i, :4], bounds=(net["xmin"], net["xmax"]), x_scale=net["xmax"] - net["xmin"])
        secs.append(time.perf_counter() - t0)
        nfev.append(int(r.nfev))
    return float(np.median(secs)), nfev


def event_ms(torch, before, timed, repeats, warmup):
    """Median ms of `timed()` between an event pair on the stream, `before()` run outside the pair, after `warmup` untimed calls."""
    ms = []
    for r in range(repeats + warmup):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        timed()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def joint_reference(net, obs_wave, flux, eflux, start, x, P, n):
    """The fp64 joint Levenberg-Marquardt loop of tests/test_lmfit_poly.py (numpy, the oracle's getspec chain) on the first n stars:
    [(x*, A*) or None where it does not end CONVERGED inside the box within 25 evaluations]."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from numpy.polynomial.chebyshev import chebvander
    from test_lmfit import OracleModel, lm_reference, CONVERGED
    from test_contfit import oracle_star
    V = chebvander(x, P - 1)
    out = []
    for i in range(n):
        om = OracleModel(net, "SMLP", obs_wave, start[i])
        f, w = flux[i].astype(np.float64), 1.0 / eflux[i] ** 2
        o = oracle_star(flux[i], w, om(start[i, :4])[0].astype(np.float32), x, P)

        def fun(z):
            m, J = om(z[:4])
            p = V @ z[4:]
            return m * p, np.concatenate([J * p[None, :], m[None, :] * V.T], axis=0)
        r = lm_reference(fun, np.concatenate([start[i, :4], o["coef"]]), np.concatenate([net["xmin"], np.full(P, -1e30)]),
                         np.concatenate([net["xmax"], np.full(P, 1e30)]), f, w)
        out.append((r["x"], r["A"]) if r["status"] == CONVERGED and r["at_bound"] == 0 and r["niter"] <= 25 else None)
    return out


def distances(refs, pars, coef):
    """Per compared star: (max over all K parameters of |x - x*| sqrt(A*_kk), max over the labels of |x - x*| in marginal sigma)."""
    cond, marg = [], []
    for i, ref in enumerate(refs):
        if ref is None:
            continue
        xs, A = ref
        dz = np.abs(np.concatenate([pars[i, :4], coef[i]]) - xs)
        cond.append(float(np.max(dz * np.sqrt(np.diag(A)))))
        marg.append(float(np.max(dz[:4] / np.sqrt(np.diag(np.linalg.inv(A)))[:4])))
    return cond, marg


def joint_mode(args):
    """--npoly P: the workload multiplied by a Chebyshev series of P coefficients per star (c_0 in [0.5, 2], |c_j| <= 0.1, the errors
    scaled with it).  (a) ``fit_joint`` stars/s and its distance from the fp64 joint reference loop on the first --ref-stars stars,
    against ``fit_with_continuum`` at each of --alt-rounds; (b) the update alone for one block of stars, event pairs on the stream:
    payne_lmfit_update at K = 4 (what the added rows cost), payne_lmfit_update_poly at K = 4 + P, and the route without it -- the
    4 + P + 1 rows built by torch in fp32 and handed to payne_lmfit_update at K = 4 + P; (c) payne_lmfit_update_poly's compulsory
    bytes, (1 + 4) n 4 + n 4 + n 8 a star and x once, against the HBM peak."""
    import torch
    from numpy.polynomial.chebyshev import chebvander
    from thepayne_amd.fitting.optfit import OptFit, LMHandle
    from thepayne_amd.fitting.contfit import abscissa
    P, N, n = args.npoly, args.stars, args.nobs
    net, obs_wave, truth, start, rng = workload(N, n)
    fit = OptFit(net, "SMLP", obs_wave, b_max=args.b_max)
    eng = fit.predictor.anns.engine
    clean = fit.model_spectra(truth).cpu().numpy().astype(np.float64)
    x = abscissa(obs_wave)
    ctrue = np.concatenate([rng.uniform(0.5, 2.0, (N, 1)), rng.uniform(-0.1, 0.1, (N, P - 1))], axis=1)
    poly = np.ascontiguousarray((chebvander(x, P - 1) @ ctrue.T).T)
    flux = ((clean + rng.normal(0, 0.01, (N, n))) * poly).astype(np.float32)
    eflux = 0.01 * poly

    def clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    for _ in range(args.warmup):
        clock(lambda: fit.fit_joint(flux, eflux, start, npoly=P))
    secs = []
    for _ in range(args.repeats):
        s, res = clock(lambda: fit.fit_joint(flux, eflux, start, npoly=P))
        secs.append(s)
    clock(lambda: fit.fit_joint(flux, eflux, start, npoly=P, timing=True))
    tm = fit.timing
    refs = joint_reference(net, obs_wave, flux, eflux, start, x, P, args.ref_stars) if args.ref_stars > 0 else []
    cond, marg = distances(refs, res["pars"], res["coef"])
    out = {"mode": "npoly", "npoly": P, "stars": N, "nobs": n, "b_max": args.b_max, "fit_joint_s_median": float(np.median(secs)), "fit_joint_s_min": float(np.min(secs)),
           "fit_joint_stars_per_s": N / float(np.median(secs)), "status_counts": np.bincount(res["status"], minlength=6).tolist(),
           "evaluations_median": float(np.median(res["niter"])), "evaluations_max": int(res["niter"].max()), "block_iterations": tm["iterations"],
           "ms_per_iteration": {k: tm[k] / tm["iterations"] for k in ("network", "broadening", "update")},
           "reference_stars_compared": len(cond), "fit_joint_sigma_all_parameters": cond, "fit_joint_marginal_sigma_labels": marg, "alternation": []}
    clock(lambda: fit.fit_with_continuum(flux[:args.b_max], eflux[:args.b_max], start[:args.b_max], npoly=P, rounds=1))
    for rounds in args.alt_rounds:
        s, alt = clock(lambda: fit.fit_with_continuum(flux, eflux, start, npoly=P, rounds=rounds))
        _, m = distances(refs, alt["pars"], alt["coef"])
        out["alternation"].append({"rounds": rounds, "s": s, "stars_per_s": N / s, "marginal_sigma_labels": m,
                                   "status_counts": np.bincount(alt["status"], minlength=6).tolist()})
    # (b) the update alone, every star RUNNING (a fresh begin before each launch, outside the event pair)
    Km, B, dev = 4, min(N, max(1, args.b_max // 5)), eng.device
    K = Km + P
    rows = torch.randn((B, 1 + Km, n), dtype=torch.float32, device=dev)
    rows[:, 0] = 1.0 + 0.1 * rows[:, 0]
    flux_d, w_d = torch.as_tensor(flux[:B]).to(dev), torch.as_tensor(1.0 / eflux[:B] ** 2).to(dev)
    x_d = torch.as_tensor(x).to(dev)
    T32 = torch.as_tensor(chebvander(x, P - 1).T.copy()).to(dev).to(torch.float32)               # [P, n]
    lo, hi = np.concatenate([net["xmin"], np.full(P, -1e30)]), np.concatenate([net["xmax"], np.full(P, 1e30)])
    x0 = np.concatenate([start[:B, :4], ctrue[:B]], axis=1)
    h4, hK = LMHandle(Km, B, dev), LMHandle(K, B, dev)
    big = torch.empty((B, 1 + K, n), dtype=torch.float32, device=dev)

    def torch_route():
        c32 = hK.trial()[:, Km:].to(torch.float32)
        p = c32 @ T32                                                                             # [B, n]
        big[:, 0] = rows[:, 0] * p
        big[:, 1:1 + Km] = rows[:, 1:] * p[:, None, :]
        big[:, 1 + Km:] = rows[:, :1] * T32[None, :, :]
        hK.update(big, flux_d, w_d)
    ms_plain = event_ms(torch, lambda: h4.begin(x0[:, :Km], lo[:Km], hi[:Km]), lambda: h4.update(rows, flux_d, w_d), args.repeats * 4, args.warmup + 2)
    ms_poly = event_ms(torch, lambda: hK.begin(x0, lo, hi), lambda: hK.update_poly(rows, flux_d, w_d, x_d, P), args.repeats * 4, args.warmup + 2)
    ms_torch = event_ms(torch, lambda: hK.begin(x0, lo, hi), torch_route, args.repeats * 4, args.warmup + 2)
    h4.close()
    hK.close()
    nbytes = B * ((1 + Km) * n * 4 + n * 4 + n * 8) + n * 8
    out.update({"stars_per_block": B, "update_ms_K4": ms_plain, "update_poly_ms": ms_poly, "torch_rows_plus_update_ms": ms_torch,
                "update_poly_over_update_K4": ms_poly / ms_plain, "torch_route_over_update_poly": ms_torch / ms_poly,
                "update_poly_bytes": nbytes, "update_poly_bytes_per_s": nbytes / (ms_poly * 1e-3), "update_poly_fraction_of_hbm_peak": nbytes / (ms_poly * 1e-3) / HBM_PEAK,
                "repeats": args.repeats, "warmup": args.warmup})
    print(json.dumps(out), flush=True)


def phot_mode(args):
    """--phot F: the --npoly workload (P = 4 unless --npoly says otherwise) with F magnitudes a star from random per-filter nets with
    colour (synth.make_phot_nets, w1 x 3, w3 x 30, width 64), 0.02 mag errors, logR and Av free and starting 10 % of their box off,
    the distance fixed.  (a) ``fit_specphot`` stars/s and the per-iteration split network / broadening / SED Jacobian / update, next to
    ``fit_joint`` on the spectra alone in the same process; (b) the update alone for one block of stars, event pairs on the stream,
    every star RUNNING: payne_lmfit_update_phot at K = 4 + 2 + P against payne_lmfit_update_poly at the same K (six model rows: it
    streams two more rows a star) and at K = 4 + P (the same rows)."""
    import torch
    from numpy.polynomial.chebyshev import chebvander
    from thepayne_amd import synth
    from thepayne_amd.fitting import SEDFit
    from thepayne_amd.fitting.optfit import OptFit, LMHandle
    from thepayne_amd.fitting.contfit import abscissa
    F, P, N, n = args.phot, args.npoly or 4, args.stars, args.nobs
    net, obs_wave, truth, start, rng = workload(N, n)
    fit = OptFit(net, "SMLP", obs_wave, b_max=args.b_max)
    eng = fit.predictor.anns.engine
    clean = fit.model_spectra(truth).cpu().numpy().astype(np.float64)
    x = abscissa(obs_wave)
    ctrue = np.concatenate([rng.uniform(0.5, 2.0, (N, 1)), rng.uniform(-0.1, 0.1, (N, P - 1))], axis=1)
    poly = np.ascontiguousarray((chebvander(x, P - 1) @ ctrue.T).T)
    flux = ((clean + rng.normal(0, 0.01, (N, n))) * poly).astype(np.float32)
    eflux = 0.01 * poly
    phot = synth.make_phot_nets(filters=["f%03d" % i for i in range(F)], H=64, seed=1)
    phot["w1"], phot["w3"] = (phot["w1"] * np.float32(3.0)).astype(np.float32), (phot["w3"] * np.float32(30.0)).astype(np.float32)
    phot["hiav"] = np.zeros((F, 5))
    sed = SEDFit(usebands=phot["filters"], nnpath=phot, device=eng.device)
    box = {"logR": (-1.0, 2.0), "Av": (0.0, 4.5)}
    ptruth = np.column_stack([rng.uniform(-0.3, 1.5, N), rng.uniform(100.0, 3000.0, N), rng.uniform(0.1, 2.0, N)])
    pstart = ptruth.copy()
    for c, nm in ((0, "logR"), (2, "Av")):
        pstart[:, c] = np.clip(ptruth[:, c] + 0.1 * (box[nm][1] - box[nm][0]) * rng.choice([-1.0, 1.0], N), *box[nm])
    mags = sed.grad(np.concatenate([truth[:, :4], ptruth], axis=1))[0] + rng.normal(0, 0.02, (N, F))
    emags = np.full((N, F), 0.02)

    def clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def both(**kw):
        return fit.fit_specphot(flux, eflux, mags, emags, start, pstart, sed, free_phot=("logR", "Av"), npoly=P, bounds=box, **kw)
    out = {"mode": "phot", "filters": F, "npoly": P, "stars": N, "nobs": n, "b_max": args.b_max, "repeats": args.repeats, "warmup": args.warmup}
    for name, call in (("fit_specphot", both), ("fit_joint", lambda **kw: fit.fit_joint(flux, eflux, start, npoly=P, **kw))):
        for _ in range(args.warmup):
            clock(call)
        secs = []
        for _ in range(args.repeats):
            s, res = clock(call)
            secs.append(s)
        clock(lambda: call(timing=True))
        tm = fit.timing
        out[name] = {"s_median": float(np.median(secs)), "s_min": float(np.min(secs)), "stars_per_s": N / float(np.median(secs)),
                     "status_counts": np.bincount(res["status"], minlength=6).tolist(), "evaluations_median": float(np.median(res["niter"])),
                     "evaluations_max": int(res["niter"].max()), "block_iterations": tm["iterations"],
                     "ms_per_iteration": {k: tm[k] / tm["iterations"] for k in tm if k != "iterations"}}
    # (b) the update alone, every star RUNNING (a fresh begin before each launch, outside the event pair)
    Km, Kp, B, dev = 4, 2, min(N, max(1, args.b_max // 5)), eng.device
    K = Km + Kp + P
    rows = torch.randn((B, 1 + Km + Kp, n), dtype=torch.float32, device=dev)
    rows[:, 0] = 1.0 + 0.1 * rows[:, 0]
    rows4 = rows[:, :1 + Km].contiguous()
    flux_d, w_d, x_d = torch.as_tensor(flux[:B]).to(dev), torch.as_tensor(1.0 / eflux[:B] ** 2).to(dev), torch.as_tensor(x).to(dev)
    prow = torch.as_tensor(np.concatenate([start[:B, :4], pstart[:B]], axis=1)).to(dev)
    m_d, dm_d = sed.grad_device(prow)
    obs_d, pw_d = torch.as_tensor(mags[:B]).to(dev), torch.as_tensor(1.0 / emags[:B] ** 2).to(dev)
    sed_col = np.array([0, 1, 2, 3, 4, 6] + [-1] * P, dtype=np.int32)
    lo = np.concatenate([net["xmin"], [box["logR"][0], box["Av"][0]], np.full(P, -1e30)])
    hi = np.concatenate([net["xmax"], [box["logR"][1], box["Av"][1]], np.full(P, 1e30)])
    x0 = np.concatenate([start[:B, :4], pstart[:B][:, [0, 2]], ctrue[:B]], axis=1)
    sel = [0, 1, 2, 3] + list(range(6, K))
    hK, h4 = LMHandle(K, B, dev), LMHandle(Km + P, B, dev)
    ms_phot = event_ms(torch, lambda: hK.begin(x0, lo, hi), lambda: hK.update_phot(rows4, flux_d, w_d, x_d, P, Kp, sed_col, m_d, dm_d, obs_d, pw_d),
                       args.repeats * 4, args.warmup + 2)
    ms_poly_K = event_ms(torch, lambda: hK.begin(x0, lo, hi), lambda: hK.update_poly(rows, flux_d, w_d, x_d, P), args.repeats * 4, args.warmup + 2)
    ms_poly_4 = event_ms(torch, lambda: h4.begin(x0[:, sel], lo[sel], hi[sel]), lambda: h4.update_poly(rows4, flux_d, w_d, x_d, P), args.repeats * 4, args.warmup + 2)
    ms_sed = event_ms(torch, lambda: None, lambda: sed.grad_device(prow), args.repeats * 4, args.warmup + 2)
    hK.close()
    h4.close()
    out.update({"stars_per_block": B, "K": K, "update_phot_ms": ms_phot, "update_poly_ms_same_K": ms_poly_K, "update_poly_ms_same_rows": ms_poly_4, "sed_jac_ms": ms_sed,
                "update_phot_over_update_poly_same_K": ms_phot / ms_poly_K, "update_phot_over_update_poly_same_rows": ms_phot / ms_poly_4,
                "fit_specphot_over_fit_joint_time": out["fit_specphot"]["s_median"] / out["fit_joint"]["s_median"]})
    print(json.dumps(out), flush=True)


def binary_mode(args):
    """--binary: the --npoly workload (P = 4 unless --npoly says otherwise) with a second component a star -- another star's Teff and
    log(g), the primary's [Fe/H] and [a/Fe] (tied in the fit), its Vrad 40 km/s off, light ratio q = 0.3; the starts 10 % of the box
    off in every label, 1 km/s in both Vrad, q = 0.4.  (a) ``fit_binary`` stars/s, status counts and the per-iteration split;
    (b) the update alone for one block of stars, event pairs on the stream, every star RUNNING: payne_lmfit_update_pair at
    K = 5 + 3 + 1 + P against payne_lmfit_update_poly at the same K (it streams 1 + K - P rows a star where the pair update streams
    2 + 5 + 5) and against the route without it -- torch forms the K + 1 mixed rows in fp32 and payne_lmfit_update sums them;
    (c) payne_lmfit_update_pair's compulsory bytes, 12 n 4 + n 4 + n 8 a star and x once, against the HBM peak."""
    import torch
    from numpy.polynomial.chebyshev import chebvander
    from thepayne_amd.fitting.optfit import OptFit, LMHandle, check_binary_args
    from thepayne_amd.fitting.contfit import abscissa
    P, N, n, q_true, tie = args.npoly or 4, args.stars, args.nobs, 0.3, ("feh", "afe")
    net, obs_wave, truth, start, rng = workload(N, n)
    fit = OptFit(net, "SMLP", obs_wave, b_max=args.b_max)
    eng = fit.predictor.anns.engine
    perm = np.roll(np.arange(N), 1)
    truth_b, start_b = truth[perm].copy(), start[perm].copy()
    for t, s in ((truth_b, truth), (start_b, start)):
        t[:, 2:4], t[:, 7] = s[:, 2:4], s[:, 7]
    truth_b[:, 4] = truth[:, 4] + 40.0
    start_a = start.copy()
    start_a[:, 4], start_b[:, 4] = truth[:, 4] + 1.0, truth_b[:, 4] - 1.0
    clean = ((1.0 - q_true) * fit.model_spectra(truth) + q_true * fit.model_spectra(truth_b)).cpu().numpy().astype(np.float64)
    x = abscissa(obs_wave)
    ctrue = np.concatenate([rng.uniform(0.5, 2.0, (N, 1)), rng.uniform(-0.1, 0.1, (N, P - 1))], axis=1)
    poly = np.ascontiguousarray((chebvander(x, P - 1) @ ctrue.T).T)
    flux = ((clean + rng.normal(0, 0.01, (N, n))) * poly).astype(np.float32)
    eflux = 0.01 * poly

    def clock(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def call(**kw):
        return fit.fit_binary(flux, eflux, start_a, start_b, ratio=0.4, tie=tie, npoly=P, **kw)
    for _ in range(args.warmup):
        clock(call)
    secs = []
    for _ in range(args.repeats):
        s, res = clock(call)
        secs.append(s)
    clock(lambda: call(timing=True))
    tm = fit.timing
    done = res["status"] == 1
    out = {"mode": "binary", "npoly": P, "stars": N, "nobs": n, "b_max": args.b_max, "repeats": args.repeats, "warmup": args.warmup,
           "fit_binary_s_median": float(np.median(secs)), "fit_binary_s_min": float(np.min(secs)), "fit_binary_stars_per_s": N / float(np.median(secs)),
           "status_counts": np.bincount(res["status"], minlength=6).tolist(), "evaluations_median": float(np.median(res["niter"])),
           "evaluations_max": int(res["niter"].max()), "block_iterations": tm["iterations"],
           "ms_per_iteration": {k: tm[k] / tm["iterations"] for k in ("network", "broadening", "update")},
           "ratio_median_converged": float(np.median(res["ratio"][done])) if done.any() else None,
           "ratio_err_median_converged": float(np.median(res["err"][done][:, res["labels"].index("ratio")])) if done.any() else None}
    # (b) the update alone, every star RUNNING (a fresh begin before each launch, outside the event pair)
    a = check_binary_args(flux[:1], eflux[:1], start_a[:1], start_b[:1], n, 4, net["xmin"], net["xmax"], ratio=0.4, tie=tie, npoly=P)
    Ka, Kl, ia, ib, lo, hi = a["Ka"], a["Kl"], a["ia"], a["ib"], a["lo"], a["hi"]
    K, B, dev = Kl + 1 + P, min(N, max(1, args.b_max // 5)), eng.device
    rows_a = torch.randn((B, 1 + Ka, n), dtype=torch.float32, device=dev)
    rows_b = torch.randn((B, 1 + Ka, n), dtype=torch.float32, device=dev)
    rows_a[:, 0], rows_b[:, 0] = 1.0 + 0.1 * rows_a[:, 0], 1.0 + 0.1 * rows_b[:, 0]
    rows_poly = torch.randn((B, 1 + K - P, n), dtype=torch.float32, device=dev)
    rows_poly[:, 0] = rows_a[:, 0]
    flux_d, w_d, x_d = torch.as_tensor(flux[:B]).to(dev), torch.as_tensor(1.0 / eflux[:B] ** 2).to(dev), torch.as_tensor(x).to(dev)
    T32 = torch.as_tensor(chebvander(x, P - 1).T.copy()).to(dev).to(torch.float32)               # [P, n]
    free_b = [k for k in range(Ka) if a["b_pos"][k] >= Ka]
    x0 = np.concatenate([start_a[:B][:, a["cols"]], start_b[:B][:, [a["cols"][k] for k in free_b]], np.full((B, 1), 0.4), ctrue[:B]], axis=1)
    lo_p, hi_p = lo.copy(), hi.copy()
    hK = LMHandle(K, B, dev)
    big = torch.empty((B, 1 + K, n), dtype=torch.float32, device=dev)
    sel_a = torch.as_tensor(np.where(ia >= 0, 1 + ia, 0)).to(dev)
    sel_b = torch.as_tensor(np.where(ib >= 0, 1 + ib, 0)).to(dev)
    has_a = torch.as_tensor((ia >= 0).astype(np.float32)).to(dev)[None, :, None]
    has_b = torch.as_tensor((ib >= 0).astype(np.float32)).to(dev)[None, :, None]

    def torch_route():
        xt = hK.trial()
        q = xt[:, Kl].to(torch.float32)[:, None]
        p = xt[:, Kl + 1:].to(torch.float32) @ T32                                                # [B, n]
        mix = (1.0 - q) * rows_a[:, 0] + q * rows_b[:, 0]
        big[:, 0] = mix * p
        big[:, 1:1 + Kl] = ((1.0 - q)[:, None] * has_a * rows_a.index_select(1, sel_a) + q[:, None] * has_b * rows_b.index_select(1, sel_b)) * p[:, None, :]
        big[:, 1 + Kl] = (rows_b[:, 0] - rows_a[:, 0]) * p
        big[:, 2 + Kl:] = mix[:, None, :] * T32[None, :, :]
        hK.update(big, flux_d, w_d)
    ms_pair = event_ms(torch, lambda: hK.begin(x0, lo, hi), lambda: hK.update_pair(rows_a, rows_b, flux_d, w_d, ia, ib, P, x_d), args.repeats * 4, args.warmup + 2)
    ms_poly = event_ms(torch, lambda: hK.begin(x0, lo_p, hi_p), lambda: hK.update_poly(rows_poly, flux_d, w_d, x_d, P), args.repeats * 4, args.warmup + 2)
    ms_torch = event_ms(torch, lambda: hK.begin(x0, lo, hi), torch_route, args.repeats * 4, args.warmup + 2)
    hK.close()
    nbytes = B * ((2 + 2 * Ka) * n * 4 + n * 4 + n * 8) + n * 8
    out.update({"stars_per_block": B, "K": K, "update_pair_ms": ms_pair, "update_poly_ms_same_K": ms_poly, "torch_rows_plus_update_ms": ms_torch,
                "update_pair_over_update_poly_same_K": ms_pair / ms_poly, "torch_route_over_update_pair": ms_torch / ms_pair,
                "update_pair_bytes": nbytes, "update_pair_bytes_per_s": nbytes / (ms_pair * 1e-3), "update_pair_fraction_of_hbm_peak": nbytes / (ms_pair * 1e-3) / HBM_PEAK,
                "update_poly_bytes_same_K": B * ((1 + K - P) * n * 4 + n * 4 + n * 8) + n * 8})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=4096)
    ap.add_argument("--nobs", type=int, default=3600)
    ap.add_argument("--b-max", type=int, default=2560)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-stars", type=int, default=8)
    ap.add_argument("--npoly", type=int, default=0, help="fit a continuum polynomial of this many coefficients along (fit_joint)")
    ap.add_argument("--ref-stars", type=int, default=6, help="--npoly: stars compared with the fp64 joint reference loop")
    ap.add_argument("--alt-rounds", type=lambda s: [int(v) for v in s.split(",")], default=[3, 10, 20, 40], help="--npoly: fit_with_continuum's rounds")
    ap.add_argument("--phot", type=int, default=0, help="fit this many magnitudes a star along with the spectrum, logR and Av free (fit_specphot)")
    ap.add_argument("--binary", action="store_true", help="fit two components a star, [Fe/H] and [a/Fe] tied, with a light ratio (fit_binary)")
    args = ap.parse_args()
    if args.binary:
        return binary_mode(args)
    if args.phot:
        return phot_mode(args)
    if args.npoly:
        return joint_mode(args)
    import torch
    from thepayne_amd.fitting.optfit import OptFit, LMHandle
    net, obs_wave, truth, start, rng = workload(args.stars, args.nobs)
    fit = OptFit(net, "SMLP", obs_wave, b_max=args.b_max)
    P, eng = fit.predictor, fit.predictor.anns.engine
    P._bind(obs_wave)
    th = np.full((args.stars, eng.ncols), np.nan)
    th[:, :8] = truth
    clean = torch.cat([eng.smooth_batch(P._jacobian().eval(truth[s:s + 512, :4])[0], th[s:s + 512], stage=2) for s in range(0, args.stars, 512)])
    flux = (clean.cpu().numpy().astype(np.float64) + rng.normal(0, 0.01, (args.stars, args.nobs))).astype(np.float32)
    eflux = np.full(flux.shape, 0.01)

    def one(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fit.fit(flux, eflux, start, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    for _ in range(args.warmup):
        one()
    secs = []
    for _ in range(args.repeats):
        s, res = one()
        secs.append(s)
    _, res_t = one(timing=True)
    tm = fit.timing
    # the update kernel alone, every star RUNNING
    K, B, n = 4, min(args.stars, max(1, args.b_max // 5)), args.nobs
    h = LMHandle(K, B, eng.device)
    rows = torch.randn((B, 1 + K, n), dtype=torch.float32, device=eng.device)
    flux_d, w_d = torch.as_tensor(flux[:B]).to(eng.device), torch.full((B, n), 1e4, dtype=torch.float64, device=eng.device)
    x0 = start[:B, :4]
    ms = []
    for r in range(args.repeats + args.warmup):
        h.begin(x0, net["xmin"], net["xmax"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.update(rows, flux_d, w_d)
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    h.close()
    bytes_update = B * ((1 + K) * n * 4 + n * 4 + n * 8)
    out = {"stars": args.stars, "nobs": args.nobs, "b_max": args.b_max, "stars_per_block": B, "fit_s_median": float(np.median(secs)), "fit_s_min": float(np.min(secs)),
           "stars_per_s": args.stars / float(np.median(secs)), "status_counts": np.bincount(res["status"], minlength=6).tolist(),
           "evaluations_median": float(np.median(res["niter"])), "evaluations_max": int(res["niter"].max()), "block_iterations": tm["iterations"],
           "ms_per_iteration": {k: tm[k] / tm["iterations"] for k in ("network", "broadening", "update")},
           "update_kernel_ms_median": float(np.median(ms)), "update_kernel_bytes": bytes_update,
           "update_kernel_bytes_per_s": bytes_update / (float(np.median(ms)) * 1e-3), "update_kernel_fraction_of_hbm_peak": bytes_update / (float(np.median(ms)) * 1e-3) / HBM_PEAK,
           "repeats": args.repeats, "warmup": args.warmup}
    if args.scipy_stars > 0:
        s, nfev = scipy_side(net, obs_wave, flux.astype(np.float64), eflux, start, args.scipy_stars)
        out.update(scipy_s_per_star_median=s, scipy_stars_per_s=1.0 / s, scipy_nfev=nfev, gpu_over_scipy=(args.stars / float(np.median(secs))) * s)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
