#!/usr/bin/env python
"""Freeze the bits of the photometric nets' kernels (sed_tile riding in the hidden-layer launch, payne_sed_kernel, payne_sedfit_jac,
payne_sedfit_run) as tests/golden/g25_phot_bits.npz: per case of the table below, the sha256 of every result's bytes and its fp64 sum
(NaN counted as zero; for a readable failure message), obtained through the public ABI only (PayneEngine.lnlike_batch, sed_batch,
bc_batch; SEDFit.grad and SEDFit.run).

Run on the MI355X with PAYNE_HIP_LIB pointing at a library built from a known-good commit (the one named on the command line):

    PAYNE_HIP_LIB=/path/to/known-good/libpayne_hip.so python tools/freeze_phot_bits_golden.py <commit hash> [out.npz]

tests/test_phot_bits_gpu.py runs the same table (CASES, run_case) on the tree's library and demands equal digests.  The inputs come
from seeds alone, through the generators the other photometric tests use (tests/test_phot_shapes.py, tests/test_sedfit.py).  The
shapes are the smallest that reach every branch of the tile the two families share (csrc/sed_tile.hpp):
    tile     sed_tile through lnlike_batch on the isolated spectrum of test_phot_shapes_gpu.py (yst_problem('small', H = 32), eflux =
             1e15: lnL is the photometric chi^2 alone), both photscale modes.  (F, H) of TILE_SHAPES with H = 16, 32, 48, 64; B of
             TILE_B such that on the MI355X's 256 compute units the tiles take 16, 32 and 48 candidates, each with a last tile whose
             live rows are no multiple of 16 (tile_plan: sed_tile_cands restated; the test asserts it on the device it runs on).
             The rows (theta_rows) hold Av >= 5 and a NaN label; the nets have a high-Av row for every filter, and (7, 48) runs
             again with one filter's row missing.
    wave     the same likelihood at (7, 20), where the tile does not apply: payne_sed_kernel's use of the row functions (mode 1)
    entry    payne_sed_batch / payne_bc_batch at (3, 17) and (7, 64) on sed_rows (modes 0 and 2)
    jac      payne_sedfit_jac at (1, 1), (3, 17), (5, 48), (7, 64); B = 1, 9, 26; both modes
    run      payne_sedfit_run at FIT_SHAPES with the free sets of test_sedfit_gpu.py's RUN_MODES (Kn = 0, 2, 5): the 24 stars of
             test_sedfit.fit_case, star 24 with every third filter at w = 0 and NaN magnitudes there, star 25 with too few filters;
             all seven outputs
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g25_phot_bits.npz")
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

EFLUX = 1e15
SPEC_H = 32
TILE = [((255, 16), (10, 40, 70, 130)), ((60, 32), (20, 130, 200)), ((7, 48), (1, 70)), ((7, 64), (10, 200))]
ENTRY_SHAPES = [(3, 17), (7, 64)]
JAC_SHAPES = [(1, 1), (3, 17), (5, 48), (7, 64)]
JAC_B = (1, 9, 26)
RUN_FREE = [("scaled", ("logA",)), ("dist", ("Teff", "logR", "Av")), ("scaled", ("Teff", "logA", "Av")),
            ("dist", ("Teff", "logg", "FeH", "aFe", "logR", "Dist", "Av")), ("scaled", ("Teff", "logg", "FeH", "aFe", "logA", "Av"))]
RUN_OUT = ("pars", "chisq", "fisher", "status", "niter", "at_bound", "nfilt")


def _cases():
    import test_phot_shapes as PS
    import test_sedfit as TS
    assert all(s in PS.TILE_SHAPES and set(bs) <= set(PS.TILE_B) for s, bs in TILE) and {h for (_, h), _ in TILE} == {16, 32, 48, 64}
    assert RUN_FREE == [(m, tuple(f)) for m, f in (("scaled", ("logA",)), ("dist", TS.FREE3[False]), ("scaled", TS.FREE3[True]),
                                                   ("dist", TS.FREE_ALL[False]), ("scaled", TS.FREE_ALL[True]))]
    out = []
    for (F, H), batches in TILE:
        for photscale in (1, 0):
            out.append(("tile", dict(F=F, H=H, photscale=photscale, nan_row=0, batches=batches)))
    out.append(("tile", dict(F=7, H=48, photscale=1, nan_row=1, batches=(70,))))
    out.append(("wave", dict(F=7, H=PS.FALLBACK_H[1], photscale=1, nan_row=0, batches=(40,))))
    for F, H in ENTRY_SHAPES:
        out.append(("entry", dict(F=F, H=H)))
    for F, H in JAC_SHAPES:
        for photscale in (0, 1):
            out.append(("jac", dict(F=F, H=H, photscale=photscale)))
    for F, H in TS.FIT_SHAPES:
        for mode, free in RUN_FREE:
            out.append(("run", dict(F=F, H=H, mode=mode, free="+".join(free))))
    return out


def case_id(case):
    fam, kw = case
    return fam + "/" + ",".join("%s=%s" % (k, "+".join(str(b) for b in v) if isinstance(v, tuple) else v) for k, v in sorted(kw.items()))


def tile_plan(n_cu):
    """[(F, H, B, cb)] of the tile cases on a device with n_cu compute units: the workgroup slots the hidden-layer launch leaves
    free (test_phot_shapes.free_slots) and sed_core.hpp's sed_tile_cands, restated."""
    from test_phot_shapes import free_slots
    out = []
    for (F, H), batches in TILE:
        for B in batches:
            slots = free_slots(n_cu, B, SPEC_H)
            nblk = slots // F if slots >= F else 1
            cb = ((B + nblk - 1) // nblk + 15) & ~15
            out.append((F, H, B, 16 if cb < 16 else min(cb, 48)))
    return out


_SMALL = {}


def _small():
    """The spectral side of the joint cases and the 200 rows every case takes its first B of (test_phot_shapes_gpu.py's `small`)."""
    if not _SMALL:
        from helpers import yst_problem
        from test_phot_shapes import theta_rows
        from thepayne_amd import nnio
        raw, obs, flux, _ = yst_problem("small", H=SPEC_H)
        thp, th7 = theta_rows(200)
        _SMALL.update(net=nnio.normalize_spec_net(raw), obs=(obs, flux, np.full(len(obs), EFLUX)), thp=thp, th7=th7)
    return _SMALL


def _joint_theta(th7, thp, photscale):
    from helpers import theta_full
    t = theta_full(th7)
    t[:, 0:4] = thp[:, 0:4]
    t[:, 8] = thp[:, 4]
    if not photscale:
        t[:, 9] = thp[:, 5]
    t[:, 10] = thp[:, 6]
    return t


def _run_joint(want_tile, F, H, photscale, nan_row, batches):
    from test_phot_shapes import make_nets, obs_phot
    from thepayne_amd.engine import PayneEngine
    s = _small()
    phot = make_nets(F, H, nan_row=bool(nan_row))
    eng = PayneEngine(s["net"], obs=s["obs"], phot=phot, obs_phot=obs_phot(phot), photscale=bool(photscale), b_max=256)
    th = _joint_theta(s["th7"], s["thp"], photscale)
    res = {}
    try:
        for B in batches:
            res["lnl/B=%d" % B] = eng.lnlike_batch(th[:B]).cpu().numpy()
            assert (eng.kernels_used()["sed"] != "payne_sed_kernel") == want_tile, eng.kernels_used()
    finally:
        eng.close()
    return res


def _run_tile(**kw):
    return _run_joint(True, **kw)


def _run_wave(**kw):
    return _run_joint(False, **kw)


def _run_entry(F, H):
    from test_phot_shapes import make_nets, sed_rows, bc_rows
    from thepayne_amd.engine import PayneEngine
    phot = make_nets(F, H)
    rows = sed_rows(phot)
    eng = PayneEngine(phot=phot, b_max=64)
    try:
        return dict(mags=eng.sed_batch(rows).cpu().numpy(), bc=eng.bc_batch(bc_rows(rows)).cpu().numpy())
    finally:
        eng.close()


def _run_jac(F, H, photscale):
    import test_sedfit as TS
    from thepayne_amd.fitting import SEDFit
    phot = TS.make_nets(F, H)
    th = TS.jac_rows(phot, photscale, n=max(JAC_B))
    fit = SEDFit(usebands=phot["filters"], nnpath=phot, photscale=bool(photscale))
    res = {}
    try:
        for B in JAC_B:
            res["mags/B=%d" % B], res["dmags/B=%d" % B] = fit.grad(th[:B])
    finally:
        fit.close()
    return res


def _run_run(F, H, mode, free):
    import torch
    import test_sedfit as TS
    from thepayne_amd.fitting import SEDFit
    photscale, free = mode == "scaled", tuple(free.split("+"))
    phot = TS.fit_nets(F, H)
    case = TS.fit_case(phot, photscale, free, seed=F + H)
    c = {k: (np.concatenate([v, v[:2]]) if isinstance(v, np.ndarray) and v.ndim == 2 and len(v) == TS.FIT_N else v) for k, v in case.items()}
    K = len(c["cols"])
    c["w"][24, 1::3] = 0.0                                           # star 24: filters that do not count, NaN under them
    c["w"][25, K - 1:] = 0.0                                         # star 25: too few
    if c["sigma"] is not None:
        c["sigma"][25] = np.inf
    c["obs"] = np.where(c["w"] != 0.0, c["obs"], np.nan)
    fit = SEDFit(usebands=phot["filters"], nnpath=phot, photscale=photscale)
    try:
        fit._setup()
        dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(fit.device)   # noqa: E731
        out = fit.run(dev(c["obs"]), dev(c["w"]), dev(c["start"]), c["cols"], c["lo"], c["hi"], dev(c["mu"]), dev(c["sigma"]), dict(TS.DEFAULTS))
        torch.cuda.synchronize()
        res = {k: out[k].cpu().numpy() for k in RUN_OUT}
    finally:
        fit.close()
    assert res["status"][25] == TS.TOO_FEW and res["nfilt"][24] == F - len(range(1, F, 3))
    return res


_RUN = {"tile": _run_tile, "wave": _run_wave, "entry": _run_entry, "jac": _run_jac, "run": _run_run}
CASES = _cases()


def run_case(case):
    """{result name: ndarray} of one case of CASES on the library thepayne_amd loads."""
    fam, kw = case
    return _RUN[fam](**kw)


def sha_of(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def sum_of(a):
    return float(np.nansum(a, dtype=np.float64))


def digests():
    """(keys, sha256 digests as bytes, fp64 sums) over all of CASES, in order."""
    keys, sha, sums = [], [], []
    for case in CASES:
        for name, a in run_case(case).items():
            keys.append(case_id(case) + "::" + name)
            sha.append(sha_of(a))
            sums.append(sum_of(a))
    return keys, sha, sums


if __name__ == "__main__":
    import torch
    if len(sys.argv) < 2 or not os.environ.get("PAYNE_HIP_LIB"):
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    keys, sha, sums = digests()
    assert len(set(keys)) == len(keys) and all(np.isfinite(sums)), "duplicate keys or non-finite sums"
    np.savez_compressed(out, keys=np.array(keys), sha256=np.frombuffer(b"".join(sha), dtype=np.uint8).reshape(len(sha), 32),
                        sums=np.array(sums, dtype=np.float64), parent_commit=np.array(sys.argv[1]), rocm_version=np.array(str(torch.version.hip)),
                        n_cu=np.array(torch.cuda.get_device_properties(0).multi_processor_count))
    print("%d digests of %d cases from %s (commit %s, ROCm %s) -> %s" % (len(keys), len(CASES), os.environ["PAYNE_HIP_LIB"], sys.argv[1],
                                                                          torch.version.hip, out))
