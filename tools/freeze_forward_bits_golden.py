#!/usr/bin/env python
"""Freeze the bits of the forward pass as the host code of csrc/payne_hip.hip wires it up (run_net: the first launch with its riders,
the hidden layers or their chain, the output layer) as tests/golden/g23_forward_bits.npz: per case of the table below, the sha256 of
every result's bytes and its fp64 sum (for a readable failure message), obtained through the public ABI only
(PayneEngine.predict_batch(stage=0) and lnlike_batch).  tests/golden/g22_out_bits.npz pins the output layer's kernels; this table
pins the hidden side and what rides in the first launch.

Run on the MI355X with PAYNE_HIP_LIB pointing at a library built from a known-good commit (the one named on the command line):

    PAYNE_HIP_LIB=/path/to/known-good/libpayne_hip.so python tools/freeze_forward_bits_golden.py <commit hash> [out.npz]

tests/test_forward_bits_gpu.py runs the same table (CASES, run_case) on the tree's library, demands equal digests and checks through
kernels_used() that every call launched the hidden-layer, output-layer and photometric kernels the case names.  The inputs come from
synth's and np.random.default_rng's seeds alone.  The shapes are the smallest that reach every arm of run_net:
    B = 33 / 64        a ragged second 32-row block of the hidden-layer tiles / two whole ones
    npix = 200         the output layer's second 128-column tile is ragged; 150 observed pixels
    LinNet 300 x 5     the second layer on fp16 pairs, layers 3 .. 5 on planes handed on (variant 0, V_HID_WAVES4), in one launch
                       (V_HID_CHAIN) or all in fp32 (V_HID_F32)
    300 x 2            the net of the flagship workload: no hidden layer past the second
    64, 48, 32         hidden widths that differ: the generic tile kernel for the output layer, no operand planes
    two layers         the output layer is the first launch (label encoding and first layer fused into the generic kernel)
    continuum          a second network through the same path, multiplied in pixel by pixel
    photometry         a joint likelihood: the photometric nets ride in the first launch, or get their own (V_SED_OWN_LAUNCH)
    V_NO_PREP          no records from the first launch: the post kernel derives them itself
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g23_forward_bits.npz")

V_NO_PREP, V_SED_OWN, V_HID_F32, V_HID_CHAIN, V_HID_WAVES4 = 16, 8192, 2097152, 4194304, 8388608     # (thepayne_amd/_lib.py: V_*)
NPIX, NOBS = 200, 150

HK_FIRST, HK_NEXT, CHAIN = "payne_dense_hidden_kernel<true, 4>", "payne_dense_hidden_kernel<false, 4>", "payne_dense_chain_kernel"
D2HH, GENERIC, SED = "payne_dense_dma2hh_kernel<5>", "payne_dense_kernel<BM, BN, BK, FUSE>", "payne_sed_kernel"


def _cases():
    """(net, keywords): `batches` = the batch sizes run on one context; `kernels` = (hidden, out, sed) every call must report, or
    {call: (hidden, out, sed)} where the calls differ."""
    out = []
    for v, hid in ((0, HK_NEXT), (V_HID_CHAIN, CHAIN), (V_HID_WAVES4, HK_NEXT), (V_HID_F32, HK_NEXT)):
        out.append(("linnet", dict(variant=v, batches=(33, 64), kernels=(hid, D2HH, ""))))
    out.append(("h300x2", dict(variant=0, batches=(33,), kernels=(HK_FIRST, D2HH, ""))))
    out.append(("widths", dict(variant=0, batches=(33,), kernels=(HK_NEXT, GENERIC, ""))))
    out.append(("two-layer", dict(variant=0, batches=(33,), kernels=("", GENERIC, ""))))
    # (the continuum network runs after the spectral one in a likelihood call, and alone for stage 4: its kernels are the last)
    out.append(("continuum", dict(variant=0, batches=(33,), kernels={"rows": (HK_FIRST, D2HH, ""), "lnl": (HK_FIRST, GENERIC, ""),
                                                                       "cont": (HK_FIRST, GENERIC, "")})))
    out.append(("photometry", dict(variant=0, batches=(33,), kernels=(HK_FIRST, D2HH, ""))))
    out.append(("photometry", dict(variant=V_SED_OWN, batches=(33,), kernels={"rows": (HK_FIRST, D2HH, ""), "lnl": (HK_FIRST, D2HH, SED)})))
    out.append(("h300x2", dict(variant=V_NO_PREP, batches=(33,), kernels=(HK_FIRST, D2HH, ""))))
    return out


CASES = _cases()


def case_id(case):
    return "%s/variant=%d" % (case[0], case[1]["variant"])


def _seed(case):
    return int.from_bytes(hashlib.sha256(case_id(case).encode()).digest()[:4], "little")


def _net(name):
    from thepayne_amd import _lib, nnio, synth
    if name == "linnet":
        raw = synth.make_torch_net("LinNet", npix=NPIX, H=(300, 300, 300), seed=3)
        return nnio.normalize_spec_net(raw, "LinNet")
    if name == "widths":
        raw = synth.make_torch_net("SMLP", npix=NPIX, H=(64, 48, 32), seed=4)
        return nnio.normalize_spec_net(raw, "SMLP")
    net = nnio.normalize_spec_net(synth.make_yst_net(npix=NPIX, H=300, seed=5, line_depth=0.2))
    if name == "two-layer":                                  # labels -> 300 -> npix
        (W0, b0, a0), _, (W2, b2, a2) = net["layers"]
        net["layers"] = [(W0, b0, a0), (W2, b2, _lib.ACT_NONE)]
    return net


def _theta(rng, net, B, eng):
    th = np.full((B, eng.ncols), np.nan)
    th[:, 0:4] = net["xmin"][:4] + rng.uniform(0.05, 0.95, size=(B, 4)) * (net["xmax"][:4] - net["xmin"][:4])
    th[:, 4] = rng.uniform(9.0, 11.0, B)
    th[:, 5] = rng.uniform(0.5, 5.0, B)
    th[:, 7] = rng.uniform(25000.0, 30000.0, B)
    if eng.phot is not None:
        th[:, eng.phot_off] = rng.uniform(-1.0, 1.0, B)          # log(A)
        th[:, eng.phot_off + 2] = rng.uniform(0.0, 1.0, B)       # Av
    return th


def run_case(case):
    """({result name: ndarray}, {result name: ((hidden, out, sed) launched, expected)}) of one case of CASES on the library the
    package loads."""
    from thepayne_amd import nnio, synth
    from thepayne_amd.engine import PayneEngine
    name, kw = case
    rng = np.random.default_rng(_seed(case))
    net = _net(name)
    w = synth.obs_grid(net["wavelength"], NOBS, inset=0.5)
    obs = (w, 1.0 + rng.normal(0, 0.01, NOBS), np.full(NOBS, 0.01))
    phot = obs_phot = None
    if name == "photometry":
        phot = synth.make_phot_nets()
        obs_phot = synth.c3_obs_phot(phot["filters"])
    b_max = max(kw["batches"])
    eng = PayneEngine(net, obs=obs, phot=phot, obs_phot=obs_phot, photscale=phot is not None, b_max=b_max, variant=kw["variant"])
    res, kernels = {}, {}
    try:
        if name == "continuum":
            wl = net["wavelength"]
            cnet = synth.make_cont_net(npix=60, lam_lo=wl[0] - 1.0, lam_hi=wl[-1] + 1.0, H=32)
            eng.set_continuum(nnio.normalize_spec_net(cnet, rescale_teff=False))
        th = _theta(rng, net, b_max, eng)
        calls = (("rows", lambda t: eng.predict_batch(t, stage=0)), ("lnl", eng.lnlike_batch))
        if name == "continuum":
            calls += (("cont", lambda t: eng.predict_batch(t, stage=4)),)
        for B in kw["batches"]:
            for call, fn in calls:
                key = "%s/B=%d" % (call, B)
                res[key] = fn(th[:B].copy()).cpu().numpy()
                used = eng.kernels_used()
                want = kw["kernels"][call] if isinstance(kw["kernels"], dict) else kw["kernels"]
                kernels[key] = ((used["hidden"], used["out"], used["sed"]), want)
    finally:
        eng.close()
    return res, kernels


def digests():
    """(keys, sha256 hex digests, fp64 sums, every kernel as named) over all of CASES, in order."""
    keys, sha, sums, named = [], [], [], True
    for case in CASES:
        res, kernels = run_case(case)
        for key, (got, want) in kernels.items():
            print("%-30s %-12s %s%s" % (case_id(case), key, got, "" if got == want else "   EXPECTED %s" % (want,)), flush=True)
            named = named and got == want
        for name, a in res.items():
            keys.append(case_id(case) + "::" + name)
            sha.append(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
            sums.append(float(np.nansum(a, dtype=np.float64)))
            assert np.isfinite(a).sum() >= 0.9 * a.size, (keys[-1], "mostly not finite")
    return keys, sha, sums, named


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch
    if len(sys.argv) < 2 or not os.environ.get("PAYNE_HIP_LIB"):
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    keys, sha, sums, named = digests()
    assert len(set(keys)) == len(keys) and all(np.isfinite(sums)), "duplicate keys or non-finite sums"
    assert named, "a call launched another kernel than its case names"
    np.savez_compressed(out, keys=np.array(keys), sha256=np.array(sha), sums=np.array(sums, dtype=np.float64),
                        parent_commit=np.array(sys.argv[1]), rocm_version=np.array(str(torch.version.hip)))
    print("%d digests of %d cases from %s (commit %s, ROCm %s) -> %s" % (len(keys), len(CASES), os.environ["PAYNE_HIP_LIB"], sys.argv[1],
                                                                          torch.version.hip, out))
