#!/usr/bin/env python
"""Freeze one training step and a short RAdam trajectory of the reference's photometric networks (Payne/train/NNmodels_new.py:
MLP_v0, MLP_v1) as tests/golden/g19_trainphot.npz.

Run where the unmodified reference is present (it is imported through oracle.ref_shim, as tools/freeze_quicklook_golden.py does):

    python tools/freeze_trainphot_golden.py

The file holds data only.  Per network ("v0": MLP_v0(5, 40, 72, 33, 3), "v1": MLP_v1(6, 64, 32, 96, 8), the shapes of
g18_lnmlp.npz), the module in train() mode with its d1.p set to 0 and every LayerNorm gain and bias perturbed by N(0, 0.3):
    <name>/model/mlp.<key>     the initial state dict (fp32)
    <name>/t                   the targets, fp32 [257, D_out]  (x, fp32 [257, 6], is shared; MLP_v0 reads its first five columns)
    <name>/loss64              MSELoss(reduction='mean') at N = 257 with the module in .double() on those fp32 values
    <name>/grad64/mlp.<key>    every parameter's gradient of that loss, fp64
    <name>/grad_dev            torch fp32's pooled deviation of the gradients: max over tensors of max|g32 - g64| / max|g64|
    <name>/traj_loss64         the losses before each of 12 full-batch torch.optim.RAdam(lr=1e-3) steps, fp64
    <name>/traj_final64/mlp.<key>   the parameters after the 12 steps, fp64
    <name>/traj_par_dev        torch fp32's pooled deviation of those parameters
    <name>/traj_loss_dev       torch fp32's max|L32 - L64| / max L64 over the 12 losses
The script asserts the conditions the tests rely on (tests/test_trainphot.py, tests/test_trainphot_gpu.py) and writes nothing
when one fails.
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim as rs  # noqa: E402

rs.install()
import torch  # noqa: E402
from Payne.train import NNmodels_new as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g19_trainphot.npz")
N, STEPS, LR = 257, 12, 1e-3
NETS = {"v0": (ref.MLP_v0, (5, 40, 72, 33, 3)), "v1": (ref.MLP_v1, (6, 64, 32, 96, 8))}


def pooled(a, b64):
    """max over the tensors of max|a - b64| / max|b64|"""
    return max(float((a[k].double() - b64[k]).abs().max() / b64[k].abs().max()) for k in b64)


def grads(model, x, t):
    model.zero_grad()
    loss = torch.nn.MSELoss(reduction='mean')(model(x), t)
    loss.backward()
    return loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def trajectory(model, x, t):
    opt = torch.optim.RAdam(model.parameters(), lr=LR)
    losses = []
    for _ in range(STEPS):
        loss = torch.nn.MSELoss(reduction='mean')(model(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses), {k: p.detach().clone() for k, p in model.named_parameters()}


def main():
    torch.manual_seed(19)
    torch.set_num_threads(1)
    rng = np.random.default_rng(19)
    out = {"x": rng.normal(0.0, 1.5, (N, 6)).astype(np.float32)}
    for name, (cls, dims) in NETS.items():
        m32 = cls(*dims)
        m32.train()
        m32.mlp.d1.p = 0.0
        with torch.no_grad():
            for k, p in m32.named_parameters():
                if ".ln" in k:
                    p.add_(torch.as_tensor(rng.normal(0.0, 0.3, tuple(p.shape)), dtype=torch.float32))
        x = torch.as_tensor(out["x"][:, :dims[0]].copy())
        t = torch.as_tensor(rng.normal(0.0, 1.0, (N, dims[-1])).astype(np.float32))
        for k, v in m32.state_dict().items():
            out["%s/model/%s" % (name, k)] = v.numpy().copy()
        out[name + "/t"] = t.numpy().copy()
        m64 = copy.deepcopy(m32).double()
        assert m32.training and m64.training and m64.mlp.d1.p == 0.0
        l32, g32 = grads(m32, x, t)
        l64, g64 = grads(m64, x.double(), t.double())
        out[name + "/loss64"] = np.float64(l64)
        for k, g in g64.items():
            out["%s/grad64/%s" % (name, k)] = g.numpy().copy()
        out[name + "/grad_dev"] = np.float64(pooled(g32, g64))
        L32, p32 = trajectory(copy.deepcopy(m32), x, t)
        L64, p64 = trajectory(copy.deepcopy(m64), x.double(), t.double())
        out[name + "/traj_loss64"] = L64
        for k, p in p64.items():
            out["%s/traj_final64/%s" % (name, k)] = p.numpy().copy()
        out[name + "/traj_par_dev"] = np.float64(pooled(p32, p64))
        out[name + "/traj_loss_dev"] = np.float64(np.abs(L32 - L64).max() / L64.max())
        # what the tests rely on
        assert abs(L64[0] - l64) <= 1e-15 * l64
        assert 1e-9 < out[name + "/grad_dev"] < 1e-5 and 1e-9 < out[name + "/traj_par_dev"] < 1e-5, name
        assert 1e-10 < out[name + "/traj_loss_dev"] < 1e-5, name
        assert L64[-1] < L64[0], name                               # the steps descend
        assert all(float(g.abs().max()) > 0 for g in g64.values()), name
        print("%s: loss64 %.6f, grad_dev %.3g, traj_par_dev %.3g, traj_loss_dev %.3g, loss %.4f -> %.4f" % (
            name, l64, out[name + "/grad_dev"], out[name + "/traj_par_dev"], out[name + "/traj_loss_dev"], L64[0], L64[-1]))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
