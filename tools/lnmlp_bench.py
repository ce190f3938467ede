"""Rows per second of the photometric LayerNorm + SiLU network on one GPU: payne_lnmlp_kernel (csrc/k_lnmlp.hip) through
Payne.predict.photANN_new against torch.nn eager on the same card.

    python tools/lnmlp_bench.py [--n 1048576] [--nntype MLP_v0] [--repeats 20] [--warmup 3]

The default network (6, 256, 256, 256, 8) from synth.phot_mlp; x is fp64 [N, 6] on the device.  Every call is timed by an event
pair on the current stream after `warmup` untimed calls; the figure is the median of `repeats` calls.  The eager side is a
torch.nn.Sequential of the same layers in fp32 on x.float() (the conversion is inside the timed region, as the kernel reads
fp64 too).  FLOP = 2 x multiply-adds of the Linear layers only; the fraction is of the fp32 matrix rate of the MI355X,
157.3 TFLOP/s.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MATRIX_PEAK = 157.3e12


def median_ms(fn, repeats, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--nntype", default="MLP_v0")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from thepayne_amd import synth
    from thepayne_amd.predict.photANN_new import ANN
    arrs = synth.phot_mlp(nntype=args.nntype, seed=5)
    A = ANN(nnpath=arrs, nntype=args.nntype)
    x = torch.as_tensor(np.random.default_rng(1).normal(0.0, 1.5, (args.n, A.model.D_in))).to("cuda:0")
    mods, macs = [], 0
    for W, b, g, be in A.model.layers:
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = torch.as_tensor(W.copy()), torch.as_tensor(b.copy())
        mods.append(lin)
        macs += W.size
        if g is not None:
            ln = torch.nn.LayerNorm(W.shape[0])
            ln.weight.data, ln.bias.data = torch.as_tensor(g.copy()), torch.as_tensor(be.copy())
            mods += [ln, torch.nn.SiLU()]
    eager = torch.nn.Sequential(*mods).eval().to("cuda:0")
    with torch.no_grad():
        y_k = A.eval(x)
        y_e = eager(x.float())
        diff = float((y_k - y_e).abs().max())
        k_ms, k_min = median_ms(lambda: A.eval(x), args.repeats, args.warmup)
        e_ms, e_min = median_ms(lambda: eager(x.float()), args.repeats, args.warmup)
    flop = 2.0 * macs * args.n
    print(json.dumps({
        "nntype": args.nntype, "dims": [A.model.D_in, A.model.H1, A.model.H2, A.model.H3, A.model.D_out], "n": args.n,
        "macs_per_row": macs, "kernel_ms_median": k_ms, "kernel_ms_min": k_min, "kernel_rows_per_s": args.n / (k_ms * 1e-3),
        "kernel_tflops": flop / (k_ms * 1e-3) / 1e12, "kernel_fraction_of_fp32_matrix_peak": flop / (k_ms * 1e-3) / FP32_MATRIX_PEAK,
        "eager_ms_median": e_ms, "eager_ms_min": e_min, "eager_rows_per_s": args.n / (e_ms * 1e-3),
        "eager_tflops": flop / (e_ms * 1e-3) / 1e12, "kernel_over_eager": e_ms / k_ms, "max_abs_kernel_minus_eager": diff,
        "repeats": args.repeats, "warmup": args.warmup}))


if __name__ == "__main__":
    main()
