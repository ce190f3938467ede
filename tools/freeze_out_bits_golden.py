#!/usr/bin/env python
"""Freeze the bits of the output layer's plane-operand kernels (csrc/dense_kernels.hpp, csrc/out_tile.hpp) as
tests/golden/g22_out_bits.npz: per case of the table below, the sha256 of every result's bytes and its fp64 sum (for a readable
failure message), obtained through the public ABI only (PayneEngine.predict_batch(stage=0) for pixel rows, lnlike_batch for
contexts whose rows go out in the frequency domain or as rows of the resampled grid).

Run on the MI355X with PAYNE_HIP_LIB pointing at a library built from a known-good commit (the one named on the command line):

    PAYNE_HIP_LIB=/path/to/known-good/libpayne_hip.so python tools/freeze_out_bits_golden.py <commit hash> [out.npz]

tests/test_out_bits_gpu.py runs the same table (CASES, run_case) on the tree's library, demands equal digests and checks through
kernels_used()["out"] that every case ran the kernel it names (a fall-back would otherwise hide one).  The inputs come from
synth.make_yst_net's and np.random.default_rng's seeds alone.  The shapes are the smallest that reach every branch:
    B = 64 / 65        a whole 64-row tile (the epilogue's scalar-base stores) / a second row tile with one real row (row clamp,
                       checked stores); npix = 200: the second 128-column tile is ragged (column clamp, col < N)
    H = 300 / 100      320 padded columns, the k-steps counted at compile time, the last stage cut at 300 / 128 padded columns,
                       k-steps counted at run time, the tail cut at the seventh 16-deep step
    variants           which of the kernels a shape gets (plan_out, csrc/out_plan.hpp); V_OUT_F32 (and V_OUT_BK64) for the fp32 ring
    npix = 1024 + obs  rows in the frequency domain (the restated weights, no bias shift)
    512 x 4224         8 x 33 = 264 tiles of 64 x 128: more than the 256 compute units, and 4224 is no multiple of 256 -- the
                       kernels for a compute unit that works through several tiles
    512 x 32768, H 100 4 x 128 whole 128 x 256 tiles: payne_dense_big3_kernel; 500 rows of the same context fall back by themselves
    npix = 700 + obs   rows of the resampled grid (n1 = 1024): a batch whose candidates all rotate, and one with a candidate that
                       does not -- the device-side switch to the pixel weights (the `sel` word), both outcomes
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g22_out_bits.npz")

V_BK64, V_F32, V_PLANES, V_BF16X3, V_WHOLE = 1024, 4096, 524288, 1048576, 16777216     # (thepayne_amd/_lib.py: V_OUT_*)
MANY_TILES = 264                                     # 64 x 128 tiles of the 512 x 4224 cases: they need a device with fewer compute units

D2HH, D2H_64, D2H_10, D2H_0 = ("payne_dense_dma2hh_kernel<5>", "payne_dense_dma2h_kernel<5, 64>", "payne_dense_dma2h_kernel<10, 32>",
                               "payne_dense_dma2h_kernel<0, 32>")
D3F, D3_10, D3_0, D3_PLAIN = ("payne_dense_dma3f_kernel<10>", "payne_dense_dma3_kernel<10, 4, true>", "payne_dense_dma3_kernel<0, 4, true>",
                              "payne_dense_dma3_kernel<0, 2, false>")
BIG_H2, BIG = "payne_dense_big3_kernel<true>", "payne_dense_big3_kernel<false>"


DMA = "payne_dense_dma_kernel<WN, BK, NK, NS, PIPE>"   # (launched from a template: all its instantiations report the template's name)


def _cases():
    """(kind, keywords); `runs` = ((batch label, B, kernel the launch must report), ...)."""
    out = []
    both = lambda k: (("B=64", 64, k), ("B=65", 65, k))
    for H, table in ((300, ((0, D2HH), (V_WHOLE, D2H_64), (V_BF16X3, D3F), (V_PLANES, D3_10))),
                     (100, ((0, D2H_0), (V_BF16X3, D3_0)))):
        for v, k in table:
            out.append(("pixels", dict(H=H, npix=200, variant=v, runs=both(k))))
            out.append(("frequency", dict(H=H, npix=1024, nobs=900, variant=v, runs=(("B=65", 65, k),))))
            out.append(("resampled", dict(H=H, npix=700, nobs=600, variant=v, runs=(("rotate", 24, k), ("one does not", 24, k)))))
    for H in (300, 100):
        for v in (V_F32, V_F32 | V_BK64):
            out.append(("pixels", dict(H=H, npix=200, variant=v, runs=both(DMA))))
    for v, k in ((0, D2H_10), (V_BF16X3, D3_PLAIN), (V_F32, DMA)):
        out.append(("pixels", dict(H=300, npix=4224, variant=v, runs=(("B=512", 512, k),), tiles=MANY_TILES)))
    for v, k, kf in ((0, BIG_H2, D2H_0), (V_BF16X3, BIG, D3_PLAIN)):
        out.append(("pixels", dict(H=100, npix=32768, variant=v, runs=(("B=512", 512, k), ("B=500", 500, kf)))))
    return out


CASES = _cases()


def case_id(case):
    kind, kw = case
    return "%s/H=%d,npix=%d,variant=%d" % (kind, kw["H"], kw["npix"], kw["variant"])


def _seed(case):
    return int.from_bytes(hashlib.sha256(case_id(case).encode()).digest()[:4], "little")


def _theta(rng, net, B, ncols):
    th = np.full((B, ncols), np.nan)
    th[:, 0:4] = net["xmin"][:4] + rng.uniform(0.05, 0.95, size=(B, 4)) * (net["xmax"][:4] - net["xmin"][:4])
    th[:, 4] = rng.uniform(9.0, 11.0, B)
    th[:, 5] = rng.uniform(0.5, 5.0, B)
    th[:, 7] = rng.uniform(25000.0, 30000.0, B)
    return th


def run_case(case, n_cu=None):
    """({result name: ndarray}, {batch label: (kernel launched, kernel expected)}) of one case of CASES on the library the package
    loads.  None if the case needs more tiles than compute units and the device has `n_cu` of them or more."""
    from thepayne_amd import nnio, synth
    from thepayne_amd.engine import PayneEngine
    kind, kw = case
    if n_cu is not None and kw.get("tiles", n_cu + 1) <= n_cu:
        return None
    rng = np.random.default_rng(_seed(case))
    raw = synth.make_yst_net(npix=kw["npix"], H=kw["H"], seed=kw["H"] + kw["npix"], line_depth=0.2)
    net = nnio.normalize_spec_net(raw)
    obs = None
    if kind != "pixels":
        w = synth.obs_grid(raw["wavelength"], kw["nobs"])
        obs = (w, 1.0 + rng.normal(0, 0.01, kw["nobs"]), np.full(kw["nobs"], 0.01))
    b_max = max(B for _, B, _ in kw["runs"])
    eng = PayneEngine(net, obs=obs, b_max=b_max, variant=kw["variant"])
    res, kernels = {}, {}
    try:
        th = _theta(rng, net, b_max, eng.ncols)
        for label, B, expect in kw["runs"]:
            t = th[:B].copy()
            if label == "one does not":
                t[3, 5] = 0.0
            if kind == "pixels":
                res["rows/" + label] = eng.predict_batch(t, stage=0).cpu().numpy()
            else:
                res["lnl/" + label] = eng.lnlike_batch(t).cpu().numpy()
            # rows in the frequency domain also where a candidate does not rotate: the switch to pixel rows is made on the device
            rows = "pixels" if kind == "pixels" else "frequency"
            kernels[label] = (eng.kernels_used()["out"] + ", rows: " + eng.kernels_used()["rows"], expect + ", rows: " + rows)
    finally:
        eng.close()
    return res, kernels


def digests():
    """(keys, sha256 hex digests, fp64 sums) over all of CASES, in order; the kernels that ran are checked on the way."""
    keys, sha, sums = [], [], []
    for case in CASES:
        res, kernels = run_case(case)
        for label, (got, want) in kernels.items():
            print("%-50s %-14s %s%s" % (case_id(case), label, got, "" if got == want else "   EXPECTED " + want), flush=True)
        for name, a in res.items():
            keys.append(case_id(case) + "::" + name)
            sha.append(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
            sums.append(float(np.nansum(a, dtype=np.float64)))
            assert np.isfinite(a).sum() >= 0.9 * a.size, (keys[-1], "mostly not finite")
            assert all(got == want for got, want in kernels.values()), (case_id(case), kernels)
    return keys, sha, sums


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch
    if len(sys.argv) < 2 or not os.environ.get("PAYNE_HIP_LIB"):
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    assert torch.cuda.get_device_properties(0).multi_processor_count < MANY_TILES, "freeze on a device with fewer compute units than 264"
    keys, sha, sums = digests()
    assert len(set(keys)) == len(keys) and all(np.isfinite(sums)), "duplicate keys or non-finite sums"
    np.savez_compressed(out, keys=np.array(keys), sha256=np.array(sha), sums=np.array(sums, dtype=np.float64),
                        parent_commit=np.array(sys.argv[1]), rocm_version=np.array(str(torch.version.hip)))
    print("%d digests of %d cases from %s (commit %s, ROCm %s) -> %s" % (len(keys), len(CASES), os.environ["PAYNE_HIP_LIB"], sys.argv[1],
                                                                          torch.version.hip, out))
