#!/usr/bin/env python
"""Freeze the bits of the fit kernels (payne_lmfit_update, payne_lmfit_update_poly, payne_contfit_batch) as
tests/golden/g24_fit_bits.npz: per case of the table below, the sha256 of every result's bytes and its fp64 sum (NaN counted as
zero; for a readable failure message), obtained through the public ABI only.

Run on the MI355X with PAYNE_HIP_LIB pointing at a library built from a known-good commit (the one named on the command line):

    PAYNE_HIP_LIB=/path/to/known-good/libpayne_hip.so python tools/freeze_fit_bits_golden.py <commit hash> [out.npz]

tests/test_fit_bits_gpu.py runs the same table (CASES, run_case) on the tree's library and demands equal digests.  The inputs come
from np.random.default_rng seeds alone.  The shapes are the smallest that reach every branch of the shared normal-equations tile
(csrc/normal_tile.hpp), of the scaled solve behind it and of the Chebyshev series (csrc/cheb_series.hpp):
    n = 1, 5, 37, 1000: less than a quarter group, a ragged group, three groups (one wave has none), many groups a wave
    layouts  "vec": every leading dimension a multiple of four and every pointer on a 16-byte boundary (16-byte loads);
             "elem": leading dimension n + 1 and every pointer one element behind a boundary (element by element)
    a tenth of the weights zero, NaN under them in star 1, 1e30 beyond n
    payne_lmfit_update       K = 1, 4, 15; B = 3; three updates on fresh rows; payne_lmfit_result's eight arrays after each
    payne_lmfit_update_poly  (Km, P) = (0, 1), (0, 4), (4, 4), (14, 1), (1, 14); the same
    payne_contfit_batch      P = 1, 4, 15; n = 5, 37, 1000; nclip 0, and 3 with rescale and drop_clipped both ways; N = 3: star 1's
                             model_index is out of range, star 2 has P - 1 counting pixels; with and without the output rows: coef,
                             chisq, npix, status, rounds and, where written, flux_out and w_out
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g24_fit_bits.npz")

B = 3                                                # stars of every call
UPDATES = 3
LM_N = (1, 5, 37, 1000)
CF_N = (5, 37, 1000)
LAYOUTS = ("vec", "elem")
CLIP = ((0, False, True), (3, False, False), (3, False, True), (3, True, False), (3, True, True))   # nclip, rescale, drop_clipped
LM_RESULTS = (("x_best", np.float64), ("chisq", np.float64), ("A", np.float64), ("g", np.float64), ("lambda", np.float64),
              ("status", np.int32), ("niter", np.int32), ("at_bound", np.int32))   # (at_bound: a bit mask, its bytes as int32)


def _cases():
    out = []
    for layout in LAYOUTS:
        for K in (1, 4, 15):
            out.append(("lmfit", dict(K=K, layout=layout)))
        for Km, P in ((0, 1), (0, 4), (4, 4), (14, 1), (1, 14)):
            out.append(("lmfit_poly", dict(Km=Km, P=P, layout=layout)))
        for P in (1, 4, 15):
            out.append(("contfit", dict(P=P, layout=layout)))
    return out


CASES = _cases()


def case_id(case):
    fam, kw = case
    return fam + "/" + ",".join("%s=%s" % (k, v) for k, v in sorted(kw.items()))


def _seed(case):
    return int.from_bytes(hashlib.sha256(case_id(case).encode()).digest()[:4], "little")


def _ld(n, layout, pad):
    """The leading dimension of a row of n values; pad: whole quads behind them in the vec layout."""
    return (n + 3) // 4 * 4 + 4 * pad if layout == "vec" else n + 1


def _dev(a, layout):
    """a on the device: on a 16-byte boundary (vec) or one element behind one (elem)."""
    import torch
    flat = np.ascontiguousarray(a).ravel()
    if layout == "vec":
        t = torch.as_tensor(flat).to("cuda:0")
        assert t.data_ptr() % 16 == 0
        return t
    t = torch.as_tensor(np.concatenate([np.zeros(1, dtype=flat.dtype), flat])).to("cuda:0")[1:]
    assert t.data_ptr() % 16 != 0
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _laid(a, ld, fill):
    """a [..., n] in rows of ld values, `fill` beyond n."""
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _weights(rng, n):
    """[B][n] positive weights, a tenth of them zero; star 1 has a zero weight wherever n allows one beside a counting pixel."""
    w = rng.uniform(50.0, 150.0, (B, n))
    w[rng.random((B, n)) < 0.1] = 0.0
    if n >= 5:
        w[1, n // 2] = 0.0
    return w


def _abscissa(rng, n):
    x = np.sort(rng.uniform(-1.0, 1.0, n))
    return x


def _lm_rows(rng, w, n_rows, n):
    """[B][n_rows][n] fp32: row 0 a model about 1, the others derivatives; star 1 holds NaN under its zero weights."""
    rows = rng.normal(0.0, 1.0, (B, n_rows, n)).astype(np.float32)
    rows[:, 0] = (1.0 + 0.1 * rng.normal(0.0, 1.0, (B, n))).astype(np.float32)
    rows[1][:, w[1] == 0.0] = np.nan
    return rows


def _run_lm(lib, rng, K, Km, P, layout):
    """Three updates on fresh rows for every n of LM_N; P == 0: payne_lmfit_update, otherwise payne_lmfit_update_poly."""
    import torch
    from thepayne_amd import _lib
    res = {}
    for n in LM_N:
        ld, ld_f = _ld(n, layout, 1), _ld(n, layout, 2)
        w = _weights(rng, n)
        flux = (1.0 + 0.1 * rng.normal(0.0, 1.0, (B, n))).astype(np.float32)
        flux[1, w[1] == 0.0] = np.nan
        x0 = rng.uniform(-0.5, 0.5, (B, K))
        if P:
            x0[:, Km] += 1.0                                         # the series' constant term
        lo, hi = np.full(K, -10.0), np.full(K, 10.0)
        flux_d, w_d = _dev(_laid(flux, ld_f, np.float32(1e30)), layout), _dev(_laid(w, ld_f, 1e30), layout)
        x_d = _dev(_abscissa(rng, n), layout) if P else None
        x0_d = torch.as_tensor(x0).to("cuda:0")
        o = _lib.LmfitOpts()
        h = C.c_void_p()
        assert lib.payne_lmfit_create(0, K, B, C.byref(o), C.byref(h)) == 0
        try:
            assert lib.payne_lmfit_begin(h, x0_d.data_ptr(), lo.ctypes.data, hi.ctypes.data, B, None) == 0
            for t in range(UPDATES):
                rows_d = _dev(_laid(_lm_rows(rng, w, 1 + Km, n), ld, np.float32(1e30)), layout)
                if P:
                    rc = lib.payne_lmfit_update_poly(h, P, rows_d.data_ptr(), ld, flux_d.data_ptr(), w_d.data_ptr(), ld_f, x_d.data_ptr(), n, None)
                else:
                    rc = lib.payne_lmfit_update(h, rows_d.data_ptr(), ld, flux_d.data_ptr(), w_d.data_ptr(), ld_f, n, None)
                assert rc == 0
                shapes = dict(x_best=(B, K), A=(B, K, K), g=(B, K))
                out = [torch.zeros(shapes.get(name, (B,)), dtype=getattr(torch, np.dtype(dt).name), device="cuda:0") for name, dt in LM_RESULTS]
                assert lib.payne_lmfit_result(h, *([a.data_ptr() for a in out] + [None])) == 0
                for (name, dt), a in zip(LM_RESULTS, out):
                    res["%s/n=%d,update=%d" % (name, n, t)] = _host(a)
        finally:
            lib.payne_lmfit_destroy(h)
    return res


def _run_lmfit(lib, rng, K, layout):
    return _run_lm(lib, rng, K, K, 0, layout)


def _run_lmfit_poly(lib, rng, Km, P, layout):
    return _run_lm(lib, rng, Km + P, Km, P, layout)


def _run_contfit(lib, rng, P, layout):
    import torch
    from thepayne_amd import _lib
    res = {}
    for n in CF_N:
        ld_f, ld_m, ld_o = _ld(n, layout, 1), _ld(n, layout, 2), _ld(n, layout, 0)
        x = _abscissa(rng, n)
        w = _weights(rng, n)
        w[2, rng.permutation(n)[P - 1:]] = 0.0                       # star 2: P - 1 counting pixels
        model = (1.0 + 0.2 * rng.normal(0.0, 1.0, (B, n))).astype(np.float32)
        index = np.array([1, B + 4, 0], dtype=np.int32)              # star 1: out of range
        cont = np.polynomial.chebyshev.chebval(x, np.r_[1.0, rng.uniform(-0.2, 0.2, P - 1)])
        flux = model[[1, 1, 0]] * cont * (1.0 + rng.normal(0.0, 1.0, (B, n)) / np.sqrt(np.where(w > 0.0, w, 1.0)))
        flux[:, ::7] *= 1.0 + rng.uniform(0.5, 1.0, flux[:, ::7].shape)   # outliers for the clipping rounds
        flux = flux.astype(np.float32)
        flux[1, w[1] == 0.0] = np.nan
        flux_d, w_d = _dev(_laid(flux, ld_f, np.float32(1e30)), layout), _dev(_laid(w, ld_f, 1e30), layout)
        model_d, x_d, index_d = _dev(_laid(model, ld_m, np.float32(1e30)), layout), _dev(x, layout), torch.as_tensor(index).to("cuda:0")
        for nclip, rescale, drop in CLIP:
            for rows in (True, False):
                coef = torch.zeros((B, P), dtype=torch.float64, device="cuda:0")
                chisq = torch.zeros(B, dtype=torch.float64, device="cuda:0")
                ints = torch.zeros((3, B), dtype=torch.int32, device="cuda:0")
                fo, wo = _dev(np.zeros((B, ld_o), dtype=np.float32), layout), _dev(np.zeros((B, ld_o)), layout)
                o = _lib.ContfitOpts(P=P, nclip=nclip, rescale=rescale, drop_clipped=drop, kappa_lo=3.0, kappa_hi=3.0)
                rc = lib.payne_contfit_batch(0, flux_d.data_ptr(), w_d.data_ptr(), ld_f, model_d.data_ptr(), ld_m, B, index_d.data_ptr(), x_d.data_ptr(), B, n,
                                             C.byref(o), coef.data_ptr(), chisq.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(),
                                             fo.data_ptr() if rows else None, wo.data_ptr() if rows else None, ld_o, None)
                assert rc == 0, lib.payne_last_error(None)
                tag = "n=%d,nclip=%d,rescale=%d,drop=%d,rows=%d" % (n, nclip, rescale, drop, rows)
                got = dict(coef=coef, chisq=chisq, npix=ints[0], status=ints[1], rounds=ints[2])
                if rows:
                    got.update(flux_out=fo, w_out=wo)
                for name, a in got.items():
                    res[name + "/" + tag] = _host(a)
    return res


_RUN = {"lmfit": _run_lmfit, "lmfit_poly": _run_lmfit_poly, "contfit": _run_contfit}


def run_case(lib, case):
    """{result name: ndarray} of one case of CASES on the loaded library."""
    fam, kw = case
    return _RUN[fam](lib, np.random.default_rng(_seed(case)), **kw)


def sha_of(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def sum_of(a):
    return float(np.nansum(a, dtype=np.float64))


def digests(lib):
    """(keys, sha256 digests as bytes, fp64 sums) over all of CASES, in order."""
    keys, sha, sums = [], [], []
    for case in CASES:
        for name, a in run_case(lib, case).items():
            keys.append(case_id(case) + "::" + name)
            sha.append(sha_of(a))
            sums.append(sum_of(a))
    return keys, sha, sums


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch
    from thepayne_amd import _lib
    if len(sys.argv) < 2 or not os.environ.get("PAYNE_HIP_LIB"):
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    keys, sha, sums = digests(_lib.load())
    assert len(set(keys)) == len(keys) and all(np.isfinite(sums)), "duplicate keys or non-finite sums"
    np.savez_compressed(out, keys=np.array(keys), sha256=np.frombuffer(b"".join(sha), dtype=np.uint8).reshape(len(sha), 32),
                        sums=np.array(sums, dtype=np.float64), parent_commit=np.array(sys.argv[1]), rocm_version=np.array(str(torch.version.hip)))
    print("%d digests of %d cases from %s (commit %s, ROCm %s) -> %s" % (len(keys), len(CASES), os.environ["PAYNE_HIP_LIB"], sys.argv[1],
                                                                          torch.version.hip, out))
