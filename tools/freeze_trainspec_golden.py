#!/usr/bin/env python
"""Freeze one training step and a short RAdam trajectory of the reference's spectral networks (Payne/train/NNmodels.py: SMLP,
LinNet) as tests/golden/g20_trainspec.npz.

Run where the unmodified reference is present (it is imported through oracle.ref_shim, as tools/freeze_trainphot_golden.py does):

    python tools/freeze_trainspec_golden.py [seed]

The file holds data only.  Per network ("smlp": SMLP(5, 40, 72, 33, 150), "linnet": LinNet(4, 48, 40, 56, 150)), the module in
train() mode with xmin = -0.5, xmax = 0.5, so that its own encode() ((x - xmin) / (xmax - xmin) - 0.5 in fp64, cast to fp32)
returns the encoded rows as they are given:
    x                          the encoded rows [130, 5] in [-0.5, 0.5)  (LinNet reads the first four columns)
    t                          the targets [130, 150] = 1 + 0.1 N(0, 1), shared by both networks; x and t are values fp16 holds
                               exactly, stored as fp16 and given to the networks as fp32
    <name>/model/<key>         the initial state dict (fp32), stored as byte planes (planes32() below)
    <name>/loss64              MSELoss(reduction='sum') at N = 130 with the module in .double() on those fp32 values
    <name>/grad64/<key>        every parameter's gradient of that loss, fp64, stored as byte planes (planes() below)
    <name>/grad_dev            torch fp32's pooled deviation of the gradients: max over tensors of max|g32 - g64| / max|g64|
    <name>/traj_loss64         the losses before each of 12 full-batch torch.optim.RAdam(lr=1e-4) steps, fp64
    <name>/traj_final64/<key>  the parameters after the 12 steps, fp64, stored as byte planes of its bits XOR the initial parameter's
    <name>/traj_par_dev        torch fp32's pooled deviation of those parameters
    <name>/traj_loss_dev       torch fp32's max|L32 - L64| / max L64 over the 12 losses
The script asserts the conditions the tests rely on (tests/test_trainspec.py, tests/test_trainspec_gpu.py) and writes nothing
when one fails: the deviations lie in (1e-10, 1e-5), the losses descend, every gradient is nonzero, and for SMLP no hidden
pre-activation of the fp64 run, over all 12 steps, lies within 1e-5 max|z| of zero (a LeakyReLU kink crossed by rounding would
otherwise decide a comparison); choose another seed if that fails.
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
from Payne.train import NNmodels as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g20_trainspec.npz")
N, STEPS, LR, D_OUT = 130, 12, 1e-4, 150
NETS = {"smlp": (ref.SMLP, (5, 40, 72, 33, D_OUT)), "linnet": (ref.LinNet, (4, 48, 40, 56, D_OUT))}
MAX_BYTES = 531648                               # the largest fixture committed so far
KINK = 1e-5


def planes(a, base=None):
    """An fp64 array as its eight byte planes, uint8 [8, *shape]: the sign and exponent bytes lie together and compress, the
    values are kept exactly.  With `base` (the fp32 array the values started from) the bits are stored XOR those of base in
    fp64, which clears the leading bytes as well.  tests/test_trainspec.py's g20_array() puts them together again."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if base is not None:
        a = (a.view(np.uint64) ^ np.ascontiguousarray(base, dtype=np.float64).view(np.uint64)).view(np.float64)
    return np.ascontiguousarray(np.moveaxis(a.view(np.uint8).reshape(a.shape + (8,)), -1, 0))


def planes32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.ascontiguousarray(np.moveaxis(a.view(np.uint8).reshape(a.shape + (4,)), -1, 0))


def data(seed):
    """x and t, rounded to values fp16 holds exactly and stored as fp16 (half the bytes; the networks are given them as fp32)."""
    rng = np.random.default_rng(seed)
    return {"x": rng.uniform(-0.5, 0.5, (N, 5)).astype(np.float16), "t": (1.0 + 0.1 * rng.normal(0.0, 1.0, (N, D_OUT))).astype(np.float16)}


def pooled(a, b64):
    """max over the tensors of max|a - b64| / max|b64|"""
    return max(float((a[k].double() - b64[k]).abs().max() / b64[k].abs().max()) for k in b64)


def grads(model, x, t):
    model.zero_grad()
    loss = torch.nn.MSELoss(reduction='sum')(model(x), t)
    loss.backward()
    return loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def kink_margin(model, x):
    """SMLP: min over the hidden Linear layers of min|z| / max|z| at the current parameters."""
    worst, a = np.inf, model.encode(x).to(next(model.parameters()).dtype)
    for m in model.features:
        a = m(a)
        if isinstance(m, torch.nn.Linear) and m is not model.features[-1]:
            worst = min(worst, float(a.abs().min() / a.abs().max()))
    return worst


def trajectory(model, x, t, watch=None):
    opt = torch.optim.RAdam(model.parameters(), lr=LR)
    losses, margin = [], np.inf
    for _ in range(STEPS):
        if watch is not None:
            with torch.no_grad():
                margin = min(margin, watch(model, x))
        loss = torch.nn.MSELoss(reduction='sum')(model(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses), {k: p.detach().clone() for k, p in model.named_parameters()}, margin


def main(seed):
    torch.manual_seed(seed)
    torch.set_num_threads(1)
    out = data(seed)
    assert out["x"].min() >= -0.5 and out["x"].max() < 0.5
    for name, (cls, dims) in NETS.items():
        d_in = dims[0]
        m32 = cls(*dims, np.full(d_in, -0.5), np.full(d_in, 0.5))
        m32.train()
        x = torch.as_tensor(out["x"][:, :d_in].astype(np.float32))
        t = torch.as_tensor(out["t"].astype(np.float32))
        assert np.array_equal(m32.encode(x).numpy(), x.numpy())         # the rows are their own encoding
        for k, v in m32.state_dict().items():
            out["%s/model/%s" % (name, k)] = planes32(v.numpy())
        m64 = copy.deepcopy(m32).double()
        m64.encode = lambda xx: xx                                      # (the module's own casts to fp32; the values are the same)
        l32, g32 = grads(m32, x, t)
        l64, g64 = grads(m64, x.double(), t.double())
        out[name + "/loss64"] = np.float64(l64)
        for k, g in g64.items():
            out["%s/grad64/%s" % (name, k)] = planes(g.numpy())
        out[name + "/grad_dev"] = np.float64(pooled(g32, g64))
        L32, p32, _ = trajectory(copy.deepcopy(m32), x, t)
        L64, p64, margin = trajectory(copy.deepcopy(m64), x.double(), t.double(), kink_margin if name == "smlp" else None)
        out[name + "/traj_loss64"] = L64
        for k, p in p64.items():
            out["%s/traj_final64/%s" % (name, k)] = planes(p.numpy(), base=m32.state_dict()[k].numpy())
        out[name + "/traj_par_dev"] = np.float64(pooled(p32, p64))
        out[name + "/traj_loss_dev"] = np.float64(np.abs(L32 - L64).max() / L64.max())
        # what the tests rely on
        assert abs(L64[0] - l64) <= 1e-15 * l64
        for k in ("/grad_dev", "/traj_par_dev", "/traj_loss_dev"):
            assert 1e-10 < out[name + k] < 1e-5, (name, k, out[name + k])
        assert L64[-1] < L64[0], name                                   # the steps descend
        assert all(float(g.abs().max()) > 0 for g in g64.values()), name
        assert margin > KINK, (name, margin)
        print("%s: loss64 %.6f, grad_dev %.3g, traj_par_dev %.3g, traj_loss_dev %.3g, loss %.4f -> %.4f, kink margin %.3g" % (
            name, l64, out[name + "/grad_dev"], out[name + "/traj_par_dev"], out[name + "/traj_loss_dev"], L64[0], L64[-1], margin))
    tmp = OUT + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    size = os.path.getsize(tmp)
    if size > MAX_BYTES:
        os.remove(tmp)
        raise SystemExit("the fixture would be %d bytes, above %d" % (size, MAX_BYTES))
    os.replace(tmp, OUT)
    print("wrote %s (%d bytes)" % (OUT, size))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 355)
