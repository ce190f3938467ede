"""Spectra with their label Jacobians per second on one GPU: payne_specjac_eval (csrc/k_specjac.hip) against torch eager computing
the same Jacobian in fp32 with D_in jvp calls, and against (1 + D_in) forward passes alone through payne_specmlp_train_predict,
all on the same card.

    python tools/specjac_bench.py [--stars 512 65536] [--max-rows 8192] [--repeats 7] [--warmup 2] [--min-ms 120]

Three shapes: SMLP 4-256-256-256-4096, LinNet 4-300x5-4096 (H1 = H2 = H3 = 300) and YST1 4-300-300-4096, initialised as TrainMod
initialises them; the labels fp64 on the device, every output buffer allocated before the clock starts.  N above --max-rows is
evaluated in chunks inside the one call.  One timed unit is `calls` consecutive calls between an event pair on the current stream
(a call is two launches a chunk and no host synchronisation); `calls` is chosen per side from a trial unit so that a unit holds at
least --min-ms of work; the figure is the median of `repeats` units after `warmup` untimed ones, divided by `calls`.  FLOP = 2 x
multiply-adds of the Linear layers x (1 + D_in) rows a star -- the primal and the D_in tangents; the first layer's tangent rows
are counted although they cost nothing -- and the fraction is of the fp32 matrix rate of the MI355X, 157.3 TFLOP/s.  The forward
comparison is one payne_specmlp_train_predict call of N rows, its time multiplied by 1 + D_in.  Prints one JSON line per shape
and N."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MATRIX_PEAK = 157.3e12
SHAPES = [("SMLP", "SMLP", (4, 256, 256, 256, 4096)), ("LinNet", "LinNet", (4, 300, 300, 300, 4096)), ("YST1", "SMLP", (4, 300, 300, 4096))]


def unit_ms(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, repeats, warmup, min_ms):
    """(median, min) milliseconds per call of fn, and the calls per timed unit.  A trial unit sizes `calls`; a side that speeds up
    once warm (eager's first calls) is sized again until its median unit holds min_ms."""
    import torch
    unit_ms(fn, 3)
    torch.cuda.synchronize()
    calls = max(2, int(np.ceil(1.25 * min_ms / (unit_ms(fn, 3) / 3.0))))
    while True:
        for _ in range(warmup):
            unit_ms(fn, calls)
        ms = [unit_ms(fn, calls) for _ in range(repeats)]
        if np.median(ms) >= min_ms:
            return float(np.median(ms)) / calls, float(np.min(ms)) / calls, calls
        calls = int(np.ceil(1.25 * calls * min_ms / np.median(ms)))


def layers_of(kind, nntype, dims):
    from thepayne_amd.train import trainspec as ts
    if kind == "YST1":                                                  # three Linear layers, LeakyReLU between them
        rng = np.random.default_rng(5)
        return [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.float32(np.sqrt(i)), rng.uniform(-1, 1, o).astype(np.float32) / np.float32(np.sqrt(i)))
                for i, o in zip(dims[:-1], dims[1:])]
    d_in, H1, H2, H3, d_out = dims
    return ts.arrays_to_layers(ts.defmod(d_in, H1, H2, H3, d_out, NNtype=nntype, seed=5), nntype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, nargs="+", default=[512, 65536])
    ap.add_argument("--max-rows", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=120.0)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    import torch
    from thepayne_amd import _lib
    from thepayne_amd.predict._spec import SpecJacobian
    from thepayne_amd.train import trainspec as ts
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for kind, nntype, dims in SHAPES:
        layers = layers_of(kind, nntype, dims)
        d_in, d_out = dims[0], dims[-1]
        macs = sum(W.size for W, b in layers)
        act = _lib.ACT_LRELU if nntype == "SMLP" else _lib.ACT_SIGMOID
        net = {"layers": [(W, b, act if i + 1 < len(layers) else _lib.ACT_NONE) for i, (W, b) in enumerate(layers)],
               "xmin": np.full(d_in, -0.5), "xmax": np.full(d_in, 0.5)}
        jac = SpecJacobian(net, max_rows=args.max_rows, device=0)
        trainer = ts.Trainer(layers, NNtype=nntype, max_rows=args.max_rows, device="cuda:0")
        mods = []
        for i, (W, b) in enumerate(layers):
            lin = torch.nn.Linear(W.shape[1], W.shape[0])
            lin.weight.data, lin.bias.data = torch.as_tensor(W.copy()), torch.as_tensor(b.copy())
            mods.append(lin)
            if i + 1 < len(layers):
                mods.append(torch.nn.LeakyReLU() if nntype == "SMLP" else torch.nn.Sigmoid())
        eager = torch.nn.Sequential(*mods).eval().to(dev)
        for N in args.stars:
            rng = np.random.default_rng(1)
            x64 = torch.as_tensor(rng.uniform(-0.5, 0.5, (N, d_in))).to(dev)
            x32 = x64.to(torch.float32)
            y = torch.empty((N, d_out), dtype=torch.float32, device=dev)
            J = torch.empty((N, d_in, d_out), dtype=torch.float32, device=dev)

            def ours():
                rc = lib.payne_specjac_eval(jac._h, x64.data_ptr(), d_in, N, y.data_ptr(), d_out, J.data_ptr(), d_out, 0, stream())
                assert rc == 0, rc

            def forward():
                rc = lib.payne_specmlp_train_predict(trainer._handle, x32.data_ptr(), d_in, N, y.data_ptr(), d_out, stream())
                assert rc == 0, rc
            k_ms, k_min, k_calls = median_ms(ours, args.repeats, args.warmup, args.min_ms)
            f_ms, f_min, f_calls = median_ms(forward, args.repeats, args.warmup, args.min_ms)
            flop = 2.0 * macs * (1 + d_in) * N
            out = {"kind": kind, "dims": list(dims), "stars": N, "max_rows": args.max_rows, "macs_per_row": macs, "rows_per_star": 1 + d_in,
                   "call_ms_median": k_ms, "call_ms_min": k_min, "calls_per_unit": k_calls, "stars_per_s": N / (k_ms * 1e-3),
                   "tflops": flop / (k_ms * 1e-3) / 1e12, "fraction_of_fp32_matrix_peak": flop / (k_ms * 1e-3) / FP32_MATRIX_PEAK,
                   "forward_ms_median": f_ms, "forward_x_rows_ms": (1 + d_in) * f_ms, "forward_x_rows_stars_per_s": N / ((1 + d_in) * f_ms * 1e-3),
                   "forward_x_rows_fraction_of_fp32_matrix_peak": flop / ((1 + d_in) * f_ms * 1e-3) / FP32_MATRIX_PEAK,
                   "forward_x_rows_over_call": (1 + d_in) * f_ms / k_ms, "repeats": args.repeats, "warmup": args.warmup, "min_ms": args.min_ms}
            if not args.no_eager:
                vs = []
                for k in range(d_in):
                    v = torch.zeros_like(x32)
                    v[:, k] = 1.0
                    vs.append(v)

                def theirs():
                    for k in range(d_in):
                        yy, jv = torch.autograd.functional.jvp(eager, x32, vs[k])
                        J[:, k, :] = jv
                e_ms, e_min, e_calls = median_ms(theirs, args.repeats, args.warmup, args.min_ms)
                out.update(eager_ms_median=e_ms, eager_ms_min=e_min, eager_calls_per_unit=e_calls, eager_stars_per_s=N / (e_ms * 1e-3),
                           eager_fraction_of_fp32_matrix_peak=flop / (e_ms * 1e-3) / FP32_MATRIX_PEAK, eager_over_call=e_ms / k_ms)
            print(json.dumps(out), flush=True)
            del x64, x32, y, J
        jac.close()
        trainer.close()


if __name__ == "__main__":
    main()
