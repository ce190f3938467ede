"""SED fits for many stars on one GPU: thepayne_amd.fitting.sedfit (payne_sedfit_run, the whole Levenberg-Marquardt fit in one
launch) against the routes it replaces.

    python tools/sedfit_bench.py [--stars 1048576] [--filters 7,12] [--width 64] [--repeats 5] [--warmup 2] [--no-sedopt]

The workload: seeded nets with colour (synth.make_phot_nets with w1 x 3 and w3 x 30), truths uniform in Teff 4000-9000, logg 1-5,
FeH -2..0.3, aFe 0..0.4, logR -0.3..1.5, Dist 100-3000, Av 0.1-2, the model's own magnitudes plus 0.02 mag noise, starts 10 % of the
box off in every free parameter.  Two fits: free = (Teff, logR, Av), and (Teff, logR, Dist, Av) with a 5 % prior on Dist.  A timed
unit is one SEDFit.run call on device tensors between two events on the stream, warm; the figure is the median of `repeats` calls.
Beside the fit: one evaluation (the same call with maxiter = 1), payne_sedfit_jac, and
  (a) payne_sed_batch on (1 + Kn) x N rows, the forward cost of the same tile rows without tangents (timed on at most 2^19 rows and
      scaled to the row count);
  (b) the route without the fused loop, per iteration: payne_sedfit_jac, then torch fp64 batched normal equations, cholesky_ex,
      cholesky_solve and a host look at the result; its fit is that times the fused fit's mean number of evaluations;
  (c) SEDopt (Nelder-Mead on the host through one-row payne_sed_batch calls) on one star, Teff fixed as its own test has it.
Floors of one evaluation: the fp64 matrix instructions of both layers at the card's 78.6 TFLOP/s, and the weights every workgroup
streams from L2 at 8 TB/s (HBM's rate: L2 is faster, so this floor is generous).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12
HBM_PEAK = 8.0e12
NAMES = ("Teff", "logg", "FeH", "aFe", "logR", "Dist", "Av")
TRUTH = {"Teff": (4000.0, 9000.0), "logg": (1.0, 5.0), "FeH": (-2.0, 0.3), "aFe": (0.0, 0.4), "logR": (-0.3, 1.5), "Dist": (100.0, 3000.0), "Av": (0.1, 2.0)}
BOX = {"Teff": (3000.0, 10000.0), "logg": (0.0, 5.5), "FeH": (-2.5, 0.5), "aFe": (-0.2, 0.6), "logR": (-1.0, 2.0), "Dist": (50.0, 5000.0), "Av": (0.0, 4.5)}


def nets(F, H, seed=1):
    from thepayne_amd import synth
    phot = synth.make_phot_nets(filters=["f%03d" % i for i in range(F)], H=H, seed=seed)
    phot["w1"] = (phot["w1"] * np.float32(3.0)).astype(np.float32)
    phot["w3"] = (phot["w3"] * np.float32(30.0)).astype(np.float32)
    return phot


def timed(torch, fn, repeats, warmup):
    ms = []
    for r in range(repeats + warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), out


def torch_iteration(torch, fit, pars, obs, w, cols, lo, hi, iv, mu, lam=1e-3):
    """One iteration of the unfused route: the Jacobian is written, read back, and the host looks at the factorisation's flags."""
    m, J = fit.grad_device(pars)
    Jf = J[:, :, cols]
    r = obs - m
    x = pars[:, cols]
    A = torch.einsum("nfi,nf,nfj->nij", Jf, w, Jf) + torch.diag_embed(iv)
    g = torch.einsum("nfi,nf,nf->ni", Jf, w, r) + (mu - x) * iv
    d = torch.diagonal(A, dim1=1, dim2=2)
    L, info = torch.linalg.cholesky_ex(A + lam * torch.diag_embed(d))
    step = torch.cholesky_solve(g[:, :, None], L)[:, :, 0]
    out = pars.clone()
    out[:, cols] = torch.minimum(torch.maximum(x + step, lo), hi)
    bad = int((info != 0).sum().item())                                 # (the host decides what to do next: a synchronisation)
    return out, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=1 << 20)
    ap.add_argument("--filters", default="7,12")
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sedopt", action="store_true")
    args = ap.parse_args()
    import torch
    from thepayne_amd.fitting.sedfit import SEDFit, LM_DEFAULTS
    if not torch.cuda.is_available():
        raise SystemExit("sedfit_bench needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    N, H = args.stars, args.width
    Hp = (H + 15) & ~15
    out = {"stars": N, "width": H, "repeats": args.repeats, "warmup": args.warmup, "fp64_matrix_peak": FP64_MATRIX_PEAK, "hbm_peak": HBM_PEAK, "runs": []}
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.rand((N, 7), dtype=torch.float64, device=dev, generator=g)
    t_lo, t_hi = (torch.tensor([TRUTH[n][i] for n in NAMES], dtype=torch.float64, device=dev) for i in (0, 1))
    truth = t_lo + (t_hi - t_lo) * u
    for F in [int(v) for v in args.filters.split(",")]:
        phot = nets(F, H)
        fit = SEDFit(usebands=phot["filters"], nnpath=phot)
        model, _ = fit.grad_device(truth.contiguous())
        obs = (model + 0.02 * torch.randn(model.shape, dtype=torch.float64, device=dev, generator=g)).contiguous()
        w = torch.full_like(obs, 1.0 / 0.02 ** 2)
        for free in (("Teff", "logR", "Av"), ("Teff", "logR", "Dist", "Av")):
            cols = [NAMES.index(f) for f in free]
            K, Kn = len(cols), sum(1 for c in cols if c < 4 or c == 6)
            S = 48 // (1 + Kn)
            lo, hi = np.array([BOX[f][0] for f in free]), np.array([BOX[f][1] for f in free])
            lo_d, hi_d = torch.as_tensor(lo).to(dev), torch.as_tensor(hi).to(dev)
            sign = torch.where(torch.rand((N, K), dtype=torch.float64, device=dev, generator=g) < 0.5, -1.0, 1.0)
            start = truth.clone()
            start[:, cols] = torch.minimum(torch.maximum(truth[:, cols] + 0.1 * (hi_d - lo_d) * sign, lo_d), hi_d)
            start = start.contiguous()
            mu = sigma = None
            iv, mu_b = torch.zeros((N, K), dtype=torch.float64, device=dev), torch.zeros((N, K), dtype=torch.float64, device=dev)
            if "Dist" in free:
                k = free.index("Dist")
                mu, sigma = torch.zeros((N, K), dtype=torch.float64, device=dev), torch.full((N, K), float("inf"), dtype=torch.float64, device=dev)
                mu[:, k], sigma[:, k] = truth[:, 5], 0.05 * truth[:, 5]
                iv[:, k], mu_b[:, k] = 1.0 / sigma[:, k] ** 2, mu[:, k]
            ms, ms_min, res = timed(torch, lambda: fit.run(obs, w, start, cols, lo, hi, mu, sigma), args.repeats, args.warmup)
            niter = res["niter"].double()
            status = res["status"].cpu().numpy()
            d_sigma = ((res["pars"][:, cols] - truth[:, cols]).abs() * torch.sqrt(torch.diagonal(res["fisher"], dim1=1, dim2=2))).max(dim=1).values
            ms1, _, _ = timed(torch, lambda: fit.run(obs, w, start, cols, lo, hi, mu, sigma, dict(LM_DEFAULTS, maxiter=1)), args.repeats, args.warmup)
            msj, _, _ = timed(torch, lambda: fit.grad_device(start), args.repeats, args.warmup)
            tiles = (N + S - 1) // S
            mfma_flop = tiles * F * 2.0 * 48 * Hp * (Hp + 8)
            l2_bytes = tiles * F * (Hp * Hp * 4.0 + 8 * Hp * 4.0 + 5 * Hp * 8.0 + 3 * Hp * 4.0)
            run = {"filters": F, "free": list(free), "K": K, "Kn": Kn, "stars_per_tile": S, "fit_ms_median": ms, "fit_ms_min": ms_min, "stars_per_s": N / (ms * 1e-3),
                   "evaluations_mean": float(niter.mean().item()), "evaluations_max": int(niter.max().item()),
                   "status_counts": {str(k): int((status == k).sum()) for k in np.unique(status)},
                   "median_distance_from_truth_in_conditional_sigma": float(d_sigma.median().item()),
                   "one_evaluation_ms": ms1, "jac_ms": msj, "jac_stars_per_s": N / (msj * 1e-3),
                   "evaluation_matrix_floor_ms": mfma_flop / FP64_MATRIX_PEAK * 1e3, "evaluation_weights_floor_ms": l2_bytes / HBM_PEAK * 1e3}
            # (a) the forward pass alone on as many rows as the tiles hold
            from thepayne_amd.predict.predictsed import FastPayneSEDPredict
            rows_n = (1 + Kn) * N
            timed_rows = min(rows_n, 1 << 19)
            fwd = FastPayneSEDPredict(usebands=phot["filters"], nnpath=phot, device=0, b_max=1 << 15)
            th = truth.repeat((timed_rows + N - 1) // N, 1)[:timed_rows]
            rows9 = torch.stack([torch.log10(th[:, 0]), th[:, 1], th[:, 2], th[:, 3], th[:, 6], torch.full_like(th[:, 0], 3.1),
                                 2.0 * th[:, 4] + 4.0 * (torch.log10(th[:, 0]) - np.log10(5770.0)), th[:, 5], torch.full_like(th[:, 0], float("nan"))], dim=1).contiguous()
            msa, _, _ = timed(torch, lambda: fwd.sed_batch(rows9), args.repeats, args.warmup)
            run.update(sed_batch_rows_timed=int(rows9.shape[0]), sed_batch_ms_timed=msa, sed_batch_ms_for_tile_rows=msa * rows_n / rows9.shape[0],
                       one_evaluation_over_sed_batch=ms1 / (msa * rows_n / rows9.shape[0]))
            # (b) the unfused route, per iteration
            msb, _, (_, bad) = timed(torch, lambda: torch_iteration(torch, fit, start, obs, w, cols, lo_d, hi_d, iv, mu_b), max(3, args.repeats // 2), 1)
            run.update(unfused_iteration_ms=msb, unfused_fit_ms_estimate=msb * run["evaluations_mean"], unfused_over_fused=msb * run["evaluations_mean"] / ms,
                       unfused_bad_factorisations=bad)
            out["runs"].append(run)
            del fwd
        if not args.no_sedopt and "sedopt_one_star_s" not in out:
            # (c) SEDopt on one star (scaled parametrisation, Teff fixed: a simplex on Teff runs to its 1e5 iterations)
            try:
                from thepayne_amd.fitting.fitutils import SEDopt
                t0 = truth[0].cpu().numpy()
                logA = 1.0
                fs = SEDFit(usebands=phot["filters"], nnpath=phot, photscale=True)
                m0 = fs.grad(np.array([[t0[0], t0[1], t0[2], t0[3], logA, t0[6]]]))[0][0]
                inputphot = {f: (float(m), 0.02) for f, m in zip(phot["filters"], m0)}
                so = SEDopt(inputphot=inputphot, photANNpath=phot, fixedpars={"Teff": float(t0[0]), "logg": float(t0[1]), "aFe": float(t0[3])},
                            initpars={"Teff": float(t0[0]), "FeH": 0.0, "logg": float(t0[1]), "aFe": float(t0[3]), "logA": 1.5, "Av": 0.5})
                tic = time.perf_counter()
                x = so()[0]
                out["sedopt_one_star_s"] = time.perf_counter() - tic
                out["sedopt_filters"] = F
                out["sedopt_fitted"] = list(so.fitpars)
                out["sedopt_error"] = [float(v) for v in (np.asarray(x) - np.array([t0[2], logA, t0[6]]))]
            except ImportError as e:                                    # scipy is SEDopt's own requirement
                out["sedopt_one_star_s"] = None
                out["sedopt_note"] = str(e)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
