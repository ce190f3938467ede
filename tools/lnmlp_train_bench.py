"""Training steps per second of the photometric LayerNorm + SiLU network on one GPU: payne_lnmlp_train_step
(csrc/k_lnmlp_train.hip) through thepayne_amd.train.trainphot.Trainer against torch eager (autograd + torch.optim.RAdam) on the
same card.

    python tools/lnmlp_train_bench.py [--batch 2048] [--nntype MLP_v0] [--steps 50] [--repeats 7] [--warmup 2]

The default network (6, 256, 256, 256, 8) initialised as TrainMod initialises it, the type's own dropout; x, t fp32 on the
device.  One timed unit is `steps` consecutive steps on the same batch between an event pair on the current stream (a step is
three launches and no host synchronisation, so single steps would time the launch path only); the figure is the median of
`repeats` units after `warmup` untimed ones, divided by `steps`.  The eager side: the reference's loop body
(trainphot.py:428-443) on a torch.nn.Sequential of the same layers with nn.Dropout, without its loss.item().
FLOP = 6 x multiply-adds of the Linear layers (forward, dA, dW) per row; the fraction is of the fp32 matrix rate of the MI355X,
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
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--nntype", default="MLP_v0")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    from thepayne_amd.train import trainphot as tp
    model = tp.defmod(6, 256, 256, 256, 8, NNtype=args.nntype, seed=5)
    block, p = tp.DROPOUT[args.nntype]
    drop = [p if i == block else 0.0 for i in range(len(model.layers) - 1)]
    trainer = tp.Trainer(model.layers, drop, max_rows=args.batch, device="cuda:0")
    rng = np.random.default_rng(1)
    x = torch.as_tensor(rng.normal(0.0, 1.0, (args.batch, 6)).astype(np.float32)).to("cuda:0")
    t = torch.as_tensor(rng.normal(0.0, 1.0, (args.batch, 8)).astype(np.float32)).to("cuda:0")
    loss_d = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    mods, macs = [], 0
    for i, (W, b, g, be) in enumerate(model.layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = torch.as_tensor(W.copy()), torch.as_tensor(b.copy())
        mods.append(lin)
        macs += W.size
        if g is not None:
            ln = torch.nn.LayerNorm(W.shape[0])
            ln.weight.data, ln.bias.data = torch.as_tensor(g.copy()), torch.as_tensor(be.copy())
            mods += [ln, torch.nn.SiLU()] + ([torch.nn.Dropout(drop[i])] if drop[i] > 0 else [])
    eager = torch.nn.Sequential(*mods).train().to("cuda:0")
    opt = torch.optim.RAdam(eager.parameters(), lr=1e-3)
    loss_fn = torch.nn.MSELoss(reduction='mean')

    def ours():
        for _ in range(args.steps):
            trainer.step(x, t, loss_d)

    def theirs():
        for _ in range(args.steps):
            loss = loss_fn(eager(x), t)
            opt.zero_grad()
            loss.backward()
            opt.step()
    k_ms, k_min = median_ms(ours, args.repeats, args.warmup)
    e_ms, e_min = median_ms(theirs, args.repeats, args.warmup)
    k_ms, k_min, e_ms, e_min = (v / args.steps for v in (k_ms, k_min, e_ms, e_min))
    flop = 6.0 * macs * args.batch
    print(json.dumps({
        "nntype": args.nntype, "dims": [model.D_in, model.H1, model.H2, model.H3, model.D_out], "batch": args.batch,
        "macs_per_row": macs, "step_ms_median": k_ms, "step_ms_min": k_min, "steps_per_s": 1e3 / k_ms,
        "step_tflops": flop / (k_ms * 1e-3) / 1e12, "step_fraction_of_fp32_matrix_peak": flop / (k_ms * 1e-3) / FP32_MATRIX_PEAK,
        "eager_step_ms_median": e_ms, "eager_step_ms_min": e_min, "step_over_eager": e_ms / k_ms, "final_loss": loss_d.item(),
        "steps_per_unit": args.steps, "repeats": args.repeats, "warmup": args.warmup}))
    trainer.close()


if __name__ == "__main__":
    main()
