"""Template-bank chi^2 search on one GPU: thepayne_amd.fitting.tmatch (payne_tmatch_match) against torch's own fp64 matrix form on
the same card and numpy's direct sum on one CPU core.

    python tools/tmatch_bench.py [--stars 4096] [--nobs 3600] [--templates 4096,65536] [--topk 4] [--repeats 5] [--warmup 1] [--numpy-stars 8]
                                 [--npoly P] [--pairs [--primaries 4]]

The workload: tools/optfit_bench.py's SMLP 4-256-256-256-4096, 3600 observed pixels, stars drawn in the inner half of the label box,
spectra from the model itself plus seeded noise at S/N 100.  The bank: a lattice of the four labels (4 per label for 4096 templates,
8 per label for 65 536) times 16 radial velocities, one Vrot and Inst_R.  A timed unit is one payne_tmatch_match call (both
launches) on device tensors between two events on the stream, warm; the figure is the median of `repeats` calls.  The share of the
fp64 matrix rate counts 4 N M n flop (two multiply-adds a pixel and pair) against the card's 78.6 TFLOP/s.  `build` is the wall
time of TemplateBank.lattice (the forward pass of every template), synchronised.
torch's form on the same tensors: (w f) @ (-2 m).T + w @ (m m).T + c0 in fp64, then torch.topk, in template blocks as large as
half of the free memory allows (its fp64 operand copies and N x block buffers are counted and reported), block lists merged by a
second topk.  numpy: sum w (f - m)^2 for `numpy-stars` stars against at most 4096 templates, one thread.  Prints one JSON line.

`--npoly P` (1 .. 8) also times payne_tmatch_match_poly on the same arrays with P Chebyshev coefficients minimised out of every pair
(the stars are the same spectra times the series 1.3, 0.25, -0.12, 0.06), beside the plain match of the same run: ms, star x
templates / s, the share of the fp64 matrix rate over 2 n (3 P - 1) flop a pair, the ratio to the plain match and the yardstick
(3 P - 1) / 2.  torch's route on the same card: the 3 P - 1 products as two fp64 matmuls in template blocks that fit half of the free
memory, A from S by a gather, linalg.cholesky_ex, cholesky_solve, the quadratic form and topk (`--torch-repeats` calls).

`--pairs` also times payne_tmatch_match_pairs (`--primaries` per star, the single-template-with-scale search's best) on binaries mixed
from the same clean spectra, 0.7 of star s and 0.3 of star s + 1, with the same noise: the call's ms between two events, star x pairs / s
over N kA M pairs, and the share of the fp64 matrix rate over 2 n flop per (row, template) -- of the whole call, so a lower bound of the
cross launch's own (a kernel trace splits the call into its three launches).  torch's route on the same card: the moments and the cross
term as fp64 matmuls (the gathered operand w m_a materialised), the 2 x 2 algebra elementwise with the same rules, topk over each star's
kA M pairs; its buffers are counted and reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12


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


def torch_form(torch, templates, f, w, topk, budget):
    """(idx, chisq, bytes of its buffers): the expanded form on torch's fp64 matmul, templates in blocks."""
    N, n = f.shape
    M = templates.shape[0]
    per_template = 2 * n * 8 + 3 * N * 8                            # -2 m and m^2 in fp64; two products and their sum
    block = int(max(1, min(M, budget // per_template)))
    a1 = w * f.double()
    c0 = (a1 * f.double()).sum(dim=1, keepdim=True)
    best_c, best_i = None, None
    for s in range(0, M, block):
        m = templates[s:s + block].double()
        chi = a1 @ (-2.0 * m).T + w @ (m * m).T + c0
        c, i = torch.topk(chi, min(topk, chi.shape[1]), dim=1, largest=False)
        i = i + s
        if best_c is None:
            best_c, best_i = c, i
        else:
            cc, ii = torch.cat([best_c, c], dim=1), torch.cat([best_i, i], dim=1)
            best_c, pick = torch.topk(cc, topk, dim=1, largest=False)
            best_i = torch.gather(ii, 1, pick)
    return best_i, best_c, block * per_template + 2 * N * n * 8, block


def torch_poly_form(torch, templates, f, w, x, P, topk, budget):
    """(idx, chisq, template block): the search with the polynomial minimised out on torch's fp64 matmul, cholesky_ex and topk."""
    N, n = f.shape
    M, Q = templates.shape[0], 2 * P - 1
    T = [torch.ones_like(x), x]
    for q in range(2, Q):
        T.append(2.0 * x * T[-1] - T[-2])
    T = torch.stack(T[:Q])                                           # [2 P - 1, n]
    a1 = w * f.double()
    c0 = (a1 * f.double()).sum(dim=1, keepdim=True)
    star_b = (a1[:, None, :] * T[None, :P]).reshape(N * P, n)
    star_s = (w[:, None, :] * T[None]).reshape(N * Q, n)
    jj, kk = torch.meshgrid(torch.arange(P, device=x.device), torch.arange(P, device=x.device), indexing="ij")
    per_template = 2 * n * 8 + N * 8 * (2 * (3 * P - 1) + 4 * P * P + 4 * P + 4)
    block = int(max(1, min(M, budget // per_template)))
    best_c, best_i = None, None
    for s in range(0, M, block):
        m = templates[s:s + block].double()
        nb = m.shape[0]
        b = (star_b @ m.T).reshape(N, P, nb).permute(0, 2, 1)
        S = (star_s @ (m * m).T).reshape(N, Q, nb).permute(0, 2, 1)
        A = 0.5 * (S[:, :, jj + kk] + S[:, :, (jj - kk).abs()])
        L, info = torch.linalg.cholesky_ex(A)
        c = torch.cholesky_solve(b[..., None], L)[..., 0]
        chi = c0 + (c * ((A @ c[..., None])[..., 0] - 2.0 * b)).sum(dim=-1)
        chi = torch.where((info == 0) & torch.isfinite(chi), chi, torch.full_like(chi, float("inf")))
        cc, i = torch.topk(chi, min(topk, nb), dim=1, largest=False)
        i = i + s
        if best_c is None:
            best_c, best_i = cc, i
        else:
            cc, ii = torch.cat([best_c, cc], dim=1), torch.cat([best_i, i], dim=1)
            best_c, pick = torch.topk(cc, topk, dim=1, largest=False)
            best_i = torch.gather(ii, 1, pick)
    return best_i, best_c, block


def torch_pair_form(torch, templates, f, w, cand, topk):
    """(flat idx [N, topk] = j M + b, chisq, bytes of its buffers): the pair search on torch's fp64 matmul, elementwise algebra and topk."""
    N, n = f.shape
    M, kA = templates.shape[0], cand.shape[1]
    m = templates.double()
    a1 = w * f.double()
    c0 = (a1 * f.double()).sum(dim=1)
    B, S = a1 @ m.T, w @ (m * m).T
    ok = cand >= 0
    a = cand.clamp(min=0).long()
    G = (w[:, None, :] * m[a]).reshape(N * kA, n)
    X = (G @ m.T).reshape(N, kA, M)
    Sa, Ba = torch.gather(S, 1, a)[:, :, None], torch.gather(B, 1, a)[:, :, None]
    Sb, Bb = S[:, None, :], B[:, None, :]
    SS = Sa * Sb
    D = SS - X * X
    al, be = (Ba * Sb - Bb * X) / D, (Bb * Sa - Ba * X) / D
    chi = c0[:, None, None] + al * (Sa * al + X * be - 2.0 * Ba) + be * (X * al + Sb * be - 2.0 * Bb)
    cols = torch.arange(M, device=f.device)[None, None, :]
    earlier = torch.zeros_like(chi, dtype=torch.bool)
    for j in range(1, kA):
        earlier[:, j] = (cols[:, 0] == a[:, :j, None]).any(dim=1)
    good = ok[:, :, None] & (cols != a[:, :, None]) & ~earlier & (Sa > 0) & (Sb > 0) & (D > SS / 1048576.0) & (al > 0) & (be > 0) & torch.isfinite(chi)
    chi = torch.where(good, chi, torch.full_like(chi, float("inf")))
    c, i = torch.topk(chi.reshape(N, kA * M), topk, dim=1, largest=False)
    nbytes = 8 * (m.numel() + a1.numel() + G.numel() + 2 * B.numel() + 6 * X.numel()) + 2 * X.numel()
    return i, c, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=4096)
    ap.add_argument("--nobs", type=int, default=3600)
    ap.add_argument("--templates", default="4096,65536")
    ap.add_argument("--topk", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--numpy-stars", type=int, default=8)
    ap.add_argument("--b-max", type=int, default=512)
    ap.add_argument("--npoly", type=int, default=0)
    ap.add_argument("--torch-repeats", type=int, default=2)
    ap.add_argument("--pairs", action="store_true")
    ap.add_argument("--primaries", type=int, default=4)
    args = ap.parse_args()
    import torch
    from optfit_bench import workload
    from thepayne_amd.fitting.optfit import OptFit
    from thepayne_amd.fitting.tmatch import TemplateBank, TMatchHandle
    net, obs_wave, truth, start, rng = workload(args.stars, args.nobs)
    fit = OptFit(net, "SMLP", obs_wave, b_max=args.b_max)
    P, eng = fit.predictor, fit.predictor.anns.engine
    P._bind(obs_wave)
    th = np.full((args.stars, eng.ncols), np.nan)
    th[:, :8] = truth
    clean = torch.cat([eng.smooth_batch(P._jacobian().eval(truth[s:s + 512, :4])[0], th[s:s + 512], stage=2) for s in range(0, args.stars, 512)])
    flux = (clean.cpu().numpy().astype(np.float64) + rng.normal(0, 0.01, (args.stars, args.nobs))).astype(np.float32)
    dev = eng.device
    f_d = torch.as_tensor(flux).to(dev)
    w_d = torch.full(flux.shape, 1e4, dtype=torch.float64, device=dev)
    N, n = flux.shape
    if args.npoly:
        from thepayne_amd.fitting.contfit import abscissa
        x_d = torch.as_tensor(abscissa(obs_wave)).to(dev)
        fp_d = (f_d.double() * (1.3 + 0.25 * x_d - 0.12 * (2.0 * x_d * x_d - 1.0) + 0.06 * (4.0 * x_d ** 3 - 3.0 * x_d))).float()
    out = {"stars": N, "nobs": n, "topk": args.topk, "npoly": args.npoly, "repeats": args.repeats, "warmup": args.warmup, "fp64_matrix_peak": FP64_MATRIX_PEAK, "runs": []}
    for M in [int(v) for v in args.templates.split(",")]:
        steps = int(round((M / 16.0) ** 0.25))
        bank = TemplateBank(net, "SMLP", obs_wave, b_max=args.b_max, max_stars=N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank.lattice(steps, vrad=np.linspace(-30.0, 30.0, 16), vrot=(10.0,), inst_R=(20000.0,))
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        M = len(bank)
        h = TMatchHandle(N, M, dev, max_poly=args.npoly)
        ms, ms_min, (idx, chisq, _) = timed(torch, lambda: h.match(bank.templates, f_d, w_d, args.topk, n=n), args.repeats, args.warmup)
        flop = 4.0 * N * M * n
        run = {"templates": M, "lattice_steps": steps, "build_s": build_s, "template_values_not_finite": int((~torch.isfinite(bank.templates)).sum().item()), "match_ms_median": ms, "match_ms_min": ms_min,
               "star_templates_per_s": N * M / (ms * 1e-3), "flop_per_s": flop / (ms * 1e-3), "fraction_of_fp64_matrix_peak": flop / (ms * 1e-3) / FP64_MATRIX_PEAK}
        free, _total = torch.cuda.mem_get_info(dev)
        t_ms, t_min, (t_idx, t_c, t_bytes, t_block) = timed(torch, lambda: torch_form(torch, bank.templates, f_d, w_d, args.topk, free // 2), args.repeats, args.warmup)
        run.update(torch_ms_median=t_ms, torch_ms_min=t_min, torch_buffer_bytes=int(t_bytes), torch_template_block=int(t_block),
                   torch_star_templates_per_s=N * M / (t_ms * 1e-3), torch_over_kernel_time=t_ms / ms,
                   top1_agree_with_torch=float((t_idx[:, 0] == idx[:, 0].long()).double().mean().item()),
                   max_abs_dchisq_top1=float((t_c[:, 0] - chisq[:, 0]).abs().max().item()))
        if args.numpy_stars > 0:
            tm = bank.templates[:4096].cpu().numpy().astype(np.float64)
            ww = np.full(n, 1e4)
            t0 = time.perf_counter()
            for s in range(args.numpy_stars):
                d = flux[s].astype(np.float64)[None, :] - tm
                (ww[None, :] * d * d).sum(axis=1)
            sec = time.perf_counter() - t0
            run.update(numpy_star_templates_per_s=args.numpy_stars * len(tm) / sec, kernel_over_numpy=(N * M / (ms * 1e-3)) / (args.numpy_stars * len(tm) / sec))
        if args.npoly:
            Pn = args.npoly
            p_ms, p_min, (p_idx, p_chisq, p_coef, p_flags, _) = timed(torch, lambda: h.match_poly(bank.templates, fp_d, w_d, x_d, Pn, args.topk, n=n),
                                                                       args.repeats, args.warmup)
            p_flop = 2.0 * n * (3 * Pn - 1) * N * M
            run.update(poly_ms_median=p_ms, poly_ms_min=p_min, poly_star_templates_per_s=N * M / (p_ms * 1e-3),
                       poly_fraction_of_fp64_matrix_peak=p_flop / (p_ms * 1e-3) / FP64_MATRIX_PEAK, poly_over_plain_time=p_ms / ms,
                       yardstick_ratio=(3 * Pn - 1) / 2.0, poly_positive_top1=float((p_flags[:, 0] & 1).double().mean().item()),
                       poly_top1_is_plain_top1_on_the_clean_stars=float((p_idx[:, 0] == idx[:, 0]).double().mean().item()))
            free, _total = torch.cuda.mem_get_info(dev)
            tp_ms, tp_min, (tp_idx, tp_c, tp_block) = timed(torch, lambda: torch_poly_form(torch, bank.templates, fp_d, w_d, x_d, Pn, args.topk, free // 2),
                                                            args.torch_repeats, 1)
            run.update(torch_poly_ms_median=tp_ms, torch_poly_ms_min=tp_min, torch_poly_template_block=int(tp_block), torch_poly_over_kernel_time=tp_ms / p_ms,
                       poly_top1_agree_with_torch=float((tp_idx[:, 0] == p_idx[:, 0].long()).double().mean().item()),
                       poly_max_abs_dchisq_top1=float((tp_c[:, 0] - p_chisq[:, 0]).abs().max().item()))
        if args.pairs:
            kA = args.primaries
            fb_d = (0.7 * clean + 0.3 * torch.roll(clean, -1, dims=0) + (f_d - clean)).float().contiguous()
            h1 = TMatchHandle(N, M, dev, max_poly=1)
            x1 = torch.zeros(n, dtype=torch.float64, device=dev)
            s_ms, _, (cand, s_chisq, _, _, _) = timed(torch, lambda: h1.match_poly(bank.templates, fb_d, w_d, x1, 1, kA, n=n), args.repeats, args.warmup)
            h1.close()
            hp = TMatchHandle(N, M, dev, max_primaries=kA)
            q_ms, q_min, (ia, ib, q_chisq, amp, _) = timed(torch, lambda: hp.match_pairs(bank.templates, fb_d, w_d, cand, args.topk, n=n), args.repeats, args.warmup)
            hp.close()
            q_flop = 2.0 * n * N * kA * M
            ratio = amp[:, 0].min(dim=1).values / amp[:, 0].sum(dim=1)
            run.update(pairs_primaries=kA, pairs_shortlist_ms_median=s_ms, pairs_ms_median=q_ms, pairs_ms_min=q_min, pairs_star_pairs_per_s=N * kA * M / (q_ms * 1e-3),
                       pairs_cross_flop_over_call_time_fraction_of_fp64_matrix_peak=q_flop / (q_ms * 1e-3) / FP64_MATRIX_PEAK,
                       pairs_workspace_bytes=int(16 * N * M + 8 * N + 28 * 8 * N * kA * ((M + 127) // 128)), pairs_listed_top1=float((ib[:, 0] >= 0).double().mean().item()),
                       pairs_chisq_below_single=float((q_chisq[:, 0] < s_chisq[:, 0]).double().mean().item()), pairs_median_ratio_top1=float(ratio.nanmedian().item()))
            tq_ms, tq_min, (tq_i, tq_c, tq_bytes) = timed(torch, lambda: torch_pair_form(torch, bank.templates, fb_d, w_d, cand, args.topk), args.torch_repeats, 1)
            j_of = (cand[:, :, None] == ia[:, None, :1]).float().argmax(dim=1)[:, 0]
            run.update(torch_pairs_ms_median=tq_ms, torch_pairs_ms_min=tq_min, torch_pairs_buffer_bytes=int(tq_bytes), torch_pairs_over_kernel_time=tq_ms / q_ms,
                       pairs_top1_agree_with_torch=float((tq_i[:, 0] == j_of * M + ib[:, 0].long()).double().mean().item()),
                       pairs_max_abs_dchisq_top1=float((tq_c[:, 0] - q_chisq[:, 0]).abs().max().item()))
            del fb_d, cand, ia, ib, q_chisq, amp, tq_i, tq_c
            torch.cuda.empty_cache()
        out["runs"].append(run)
        h.close()
        bank.close()
        del bank, h
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
