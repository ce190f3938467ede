"""Continuum polynomials for many stars on one GPU: thepayne_amd.fitting.contfit (payne_contfit_batch) against torch's own fp64 route on
the same card and numpy's lstsq on one CPU core.

    python tools/contfit_bench.py [--stars 4096] [--nobs 3600] [--npoly 4,8] [--nclip 0,3] [--repeats 7] [--warmup 2] [--numpy-stars 16]

The workload: seeded spectra, a model of order one with 10 % structure times a Chebyshev series (c_0 in [0.5, 2], |c_j| <= 0.1) plus
noise at S/N 100, cosmic rays (+0.2 .. 2) on 3 % of the pixels and dips (x 0.3 .. 0.8) on 3 %, errors of 0.01, a tenth of the pixels
without weight.  A timed unit is one ContinuumFit.run call (one launch, with the normalised rows written) on device tensors between
two events on the stream, warm; the figure is the median of `repeats` calls.  Compulsory bytes: 16 n a star for every pass that reads
flux, weights and model (one per solve and one per residual pass, counted from the `rounds` the call returns), 12 n read and 12 n
written by the output pass; their rate is set against the 8 TB/s HBM peak.  The sums pass also issues n / 4 fp64 matrix instructions a
star: its floor at the card's 78.6 TFLOP/s is reported beside the bytes' floor, and the larger of the two is the bound.
torch's route on the same tensors: B = m T [N, n, P] in fp64, the normal equations by einsum, torch.linalg.cholesky_ex and
cholesky_solve, chi^2 by a second einsum; with clipping, the same loop with a 0 / 1 mask on the weights, nclip + 1 solves.  numpy:
lstsq on sqrt(w) m T for `numpy-stars` stars, one thread, the same clipping loop.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
from numpy.polynomial.chebyshev import chebvander

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
FP64_MATRIX_PEAK = 78.6e12


def workload(N, n, P, seed=0):
    rng = np.random.default_rng(seed)
    wave = 5150.0 + np.cumsum(rng.uniform(0.02, 0.04, n))
    from thepayne_amd.fitting.contfit import abscissa
    x = abscissa(wave)
    model = (1.0 + 0.1 * rng.normal(0, 1, (N, n))).astype(np.float32)
    coef = np.concatenate([rng.uniform(0.5, 2.0, (N, 1)), rng.uniform(-0.1, 0.1, (N, P - 1))], axis=1)
    flux = model.astype(np.float64) * (chebvander(x, P - 1) @ coef.T).T + 0.01 * rng.normal(0, 1, (N, n))
    hit = rng.uniform(size=(N, n))
    flux[hit < 0.03] += rng.uniform(0.2, 2.0, int((hit < 0.03).sum()))
    dip = (hit >= 0.03) & (hit < 0.06)
    flux[dip] *= rng.uniform(0.3, 0.8, int(dip.sum()))
    w = np.full((N, n), 1e4)
    w[rng.uniform(size=(N, n)) < 0.1] = 0.0
    return wave, x, flux.astype(np.float32), w, model


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


def torch_route(torch, f, w, m, T, nclip, kappa=3.0, block=512):
    """coef [N, P] by batched normal equations in fp64, stars in blocks (B is block x n x P doubles)."""
    out = []
    for s in range(0, f.shape[0], block):
        fb, wb = f[s:s + block].double(), w[s:s + block]
        B = m[s:s + block].double()[:, :, None] * T[None]
        keep = (wb != 0).double()
        for r in range(nclip + 1):
            wk = wb * keep
            A = torch.einsum("spi,sp,spj->sij", B, wk, B)
            b = torch.einsum("spi,sp,sp->si", B, wk, fb)
            L, _info = torch.linalg.cholesky_ex(A)
            c = torch.cholesky_solve(b[:, :, None], L)[:, :, 0]
            if r < nclip:
                z = torch.sqrt(wb) * (fb - torch.einsum("spi,si->sp", B, c))
                keep = ((wb != 0) & (z >= -kappa) & (z <= kappa)).double()
        out.append(c)
    return torch.cat(out)


def numpy_route(f, w, m, x, P, nclip, kappa=3.0):
    V = chebvander(x, P - 1) * m.astype(np.float64)[:, None]
    sw, fz = np.sqrt(w), f.astype(np.float64)
    counting = w != 0
    keep = counting.copy()
    for r in range(nclip + 1):
        c = np.linalg.lstsq(sw[keep, None] * V[keep], sw[keep] * fz[keep], rcond=None)[0]
        if r < nclip:
            z = sw * (fz - V @ c)
            new = counting & (z >= -kappa) & (z <= kappa)
            if np.array_equal(new, keep):
                break
            keep = new
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=4096)
    ap.add_argument("--nobs", type=int, default=3600)
    ap.add_argument("--npoly", default="4,8")
    ap.add_argument("--nclip", default="0,3")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-stars", type=int, default=16)
    args = ap.parse_args()
    import torch
    from thepayne_amd.fitting.contfit import ContinuumFit
    if not torch.cuda.is_available():
        raise SystemExit("contfit_bench needs a GPU: a timing taken elsewhere says nothing")
    N, n = args.stars, args.nobs
    out = {"stars": N, "nobs": n, "repeats": args.repeats, "warmup": args.warmup, "hbm_peak": HBM_PEAK, "fp64_matrix_peak": FP64_MATRIX_PEAK, "runs": []}
    for P in [int(v) for v in args.npoly.split(",")]:
        wave, x, flux, w, model = workload(N, n, P)
        f_d, w_d, m_d = (torch.as_tensor(a).to("cuda:0") for a in (flux, w, model))
        T_d = torch.as_tensor(chebvander(x, P - 1)).to("cuda:0")
        for nclip in [int(v) for v in args.nclip.split(",")]:
            cf = ContinuumFit(wave, npoly=P, nclip=nclip)
            ms, ms_min, res = timed(torch, lambda: cf.run(f_d, w_d, m_d), args.repeats, args.warmup)
            rounds = res["rounds"].cpu().numpy().astype(np.int64)
            passes = rounds + np.minimum(rounds, nclip)
            nbytes = float(n * (16.0 * passes.sum() + 24.0 * N))
            mfma_flop = float(rounds.sum()) * (n / 4.0) * 2.0 * 16 * 16 * 4
            floor_hbm, floor_mfma = nbytes / HBM_PEAK, mfma_flop / FP64_MATRIX_PEAK
            run = {"npoly": P, "nclip": nclip, "ms_median": ms, "ms_min": ms_min, "stars_per_s": N / (ms * 1e-3), "solves_mean": float(rounds.mean()),
                   "passes_mean": float(passes.mean()) + 1.0, "compulsory_bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
                   "fraction_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK, "hbm_floor_ms": floor_hbm * 1e3, "matrix_floor_ms": floor_mfma * 1e3,
                   "bound": "fp64 matrix instruction" if floor_mfma > floor_hbm else "HBM", "fraction_of_bound": max(floor_hbm, floor_mfma) / (ms * 1e-3),
                   "status_ok": int((res["status"] == 0).sum().item())}
            bare_ms, _, _ = timed(torch, lambda: cf.run(f_d, w_d, m_d, normalise=False), args.repeats, args.warmup)
            run["ms_median_without_rows"] = bare_ms
            t_ms, t_min, t_c = timed(torch, lambda: torch_route(torch, f_d, w_d, m_d, T_d, nclip), max(3, args.repeats // 2), 1)
            V = T_d
            dp = (torch.einsum("pj,sj->sp", V, res["coef"]) - torch.einsum("pj,sj->sp", V, t_c)).abs().max().item()
            run.update(torch_ms_median=t_ms, torch_ms_min=t_min, torch_stars_per_s=N / (t_ms * 1e-3), torch_over_kernel_time=t_ms / ms, max_abs_dpoly_vs_torch=float(dp))
            if args.numpy_stars > 0:
                t0 = time.perf_counter()
                for s in range(args.numpy_stars):
                    numpy_route(flux[s], w[s], model[s], x, P, nclip)
                sec = time.perf_counter() - t0
                run.update(numpy_stars_per_s=args.numpy_stars / sec, kernel_over_numpy=(N / (ms * 1e-3)) / (args.numpy_stars / sec))
            out["runs"].append(run)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
