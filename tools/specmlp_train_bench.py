"""Training steps per second of the spectral networks on one GPU: payne_specmlp_train_step (csrc/k_specmlp_train.hip) through
thepayne_amd.train.trainspec.Trainer against torch eager (autograd + torch.optim.RAdam) on the same card.

    python tools/specmlp_train_bench.py [--batch 512] [--repeats 7] [--warmup 2] [--min-ms 120]

Two shapes: SMLP 4-256-256-256-4096 and LinNet 4-300x5-4096 (H1 = H2 = H3 = 300), initialised as TrainMod initialises them; x
(encoded rows), t fp32 on the device.  One timed unit is `steps` consecutive steps on the same batch between an event pair on
the current stream (a step is five launches and no host synchronisation, so single steps would time the launch path only);
`steps` is chosen per side from a trial unit so that a unit holds at least --min-ms of work; the figure is the median of
`repeats` units after `warmup` untimed ones, divided by `steps`.  The forward alone (payne_specmlp_train_loss: launches 1 and 2)
is timed the same way.  The eager side: the reference's loop body (trainspec.py:425-444) on a torch.nn.Sequential of the same
layers, without its loss.item().  FLOP = 6 x multiply-adds of the Linear layers (forward, dA, dW) per row; the fraction is of
the fp32 matrix rate of the MI355X, 157.3 TFLOP/s.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MATRIX_PEAK = 157.3e12
SHAPES = [("SMLP", (4, 256, 256, 256, 4096)), ("LinNet", (4, 300, 300, 300, 4096))]


def unit_ms(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, repeats, warmup, min_ms):
    """(median, min) milliseconds per call of fn, and the calls per timed unit."""
    import torch
    unit_ms(fn, 3)
    torch.cuda.synchronize()
    steps = max(10, int(np.ceil(1.25 * min_ms / (unit_ms(fn, 10) / 10.0))))
    for _ in range(warmup):
        unit_ms(fn, steps)
    ms = [unit_ms(fn, steps) for _ in range(repeats)]
    assert np.median(ms) >= min_ms, (np.median(ms), min_ms)
    return float(np.median(ms)) / steps, float(np.min(ms)) / steps, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=120.0)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    import torch
    from thepayne_amd.train import trainspec as ts
    for nntype, (d_in, H1, H2, H3, d_out) in SHAPES:
        layers = ts.arrays_to_layers(ts.defmod(d_in, H1, H2, H3, d_out, NNtype=nntype, seed=5), nntype)
        trainer = ts.Trainer(layers, NNtype=nntype, max_rows=args.batch, device="cuda:0")
        rng = np.random.default_rng(1)
        x = torch.as_tensor(rng.uniform(-0.5, 0.5, (args.batch, d_in)).astype(np.float32)).to("cuda:0")
        t = torch.as_tensor((1.0 + 0.1 * rng.normal(0.0, 1.0, (args.batch, d_out))).astype(np.float32)).to("cuda:0")
        loss_d = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        macs = sum(W.size for W, b in layers)
        k_ms, k_min, k_steps = median_ms(lambda: trainer.step(x, t, loss_d), args.repeats, args.warmup, args.min_ms)
        f_ms, f_min, f_steps = median_ms(lambda: trainer.loss(x, t, loss_d), args.repeats, args.warmup, args.min_ms)
        flop = 6.0 * macs * args.batch
        out = {"nntype": nntype, "dims": [W.shape[0] for W, b in layers], "d_in": d_in, "batch": args.batch, "macs_per_row": macs,
               "step_ms_median": k_ms, "step_ms_min": k_min, "steps_per_s": 1e3 / k_ms, "steps_per_unit": k_steps,
               "step_tflops": flop / (k_ms * 1e-3) / 1e12, "step_fraction_of_fp32_matrix_peak": flop / (k_ms * 1e-3) / FP32_MATRIX_PEAK,
               "forward_ms_median": f_ms, "forward_fraction_of_fp32_matrix_peak": flop / 3.0 / (f_ms * 1e-3) / FP32_MATRIX_PEAK,
               "steps_taken": trainer.steps, "repeats": args.repeats, "warmup": args.warmup, "min_ms": args.min_ms}
        if not args.no_eager:
            mods = []
            for i, (W, b) in enumerate(layers):
                lin = torch.nn.Linear(W.shape[1], W.shape[0])
                lin.weight.data, lin.bias.data = torch.as_tensor(W.copy()), torch.as_tensor(b.copy())
                mods.append(lin)
                if i + 1 < len(layers):
                    mods.append(torch.nn.LeakyReLU() if nntype == "SMLP" else torch.nn.Sigmoid())
            eager = torch.nn.Sequential(*mods).train().to("cuda:0")
            opt = torch.optim.RAdam(eager.parameters(), lr=1e-4)
            loss_fn = torch.nn.MSELoss(reduction='sum')

            def theirs():
                loss = loss_fn(eager(x), t)
                opt.zero_grad()
                loss.backward()
                opt.step()
            e_ms, e_min, e_steps = median_ms(theirs, args.repeats, args.warmup, args.min_ms)
            out.update(eager_step_ms_median=e_ms, eager_step_ms_min=e_min, eager_steps_per_unit=e_steps, step_over_eager=e_ms / k_ms)
        print(json.dumps(out), flush=True)
        trainer.close()


if __name__ == "__main__":
    main()
