"""Least-squares label fits per second on one GPU: thepayne_amd.fitting.optfit.OptFit (payne_specjac_eval + payne_smooth_batch +
payne_lmfit_update an iteration) against scipy.optimize.least_squares around the numpy oracle's getspec on one CPU core.

    python tools/optfit_bench.py [--stars 4096] [--nobs 3600] [--b-max 2560] [--repeats 5] [--warmup 1] [--scipy-stars 8]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=4096)
    ap.add_argument("--nobs", type=int, default=3600)
    ap.add_argument("--b-max", type=int, default=2560)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-stars", type=int, default=8)
    args = ap.parse_args()
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
