#!/usr/bin/env python
"""Freeze the reference's quick-look classes (Payne/fitting/fitutils.py: RVcalc, BROADcalc, PCcalc) on small synthetic
inputs as tests/golden/g17_quicklook.npz.

Run where the unmodified reference is present (it is imported through oracle.ref_shim, as oracle/gen_golden.py does):

    python tools/freeze_quicklook_golden.py

The file holds data only: the inputs, the reference's chi^2 on every grid value, its brute / minimize results and, for the
polynomial fit, the closed-form weighted least-squares minimiser of the same chi^2.  The script asserts the conditions the
tests rely on (tests/test_quicklook.py, tests/test_quicklook_gpu.py) and writes nothing when one fails.  The reference's
SEDopt reads HDF5 network files through h5py and gets no fixture.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim as rs  # noqa: E402

rs.install()
import scipy  # noqa: E402
from numpy.polynomial.chebyshev import chebvander  # noqa: E402
from Payne.fitting import fitutils as ref  # noqa: E402
from Payne.utils import smoothing as ref_smoothing  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g17_quicklook.npz")
C_KMS = 299792.458
NM, G = 1000, 67
NOBS = (1, 63, 257)


def lines(wave, centres, depths, sigmas):
    f = np.ones_like(wave)
    for c, d, s in zip(centres, depths, sigmas):
        f -= d * np.exp(-0.5 * ((wave - c) / s) ** 2)
    return f


def restated_chisq_rv(modwave, modflux, wave, flux, eflux, rv):
    """interp1d's own linear rule (searchsorted side left, clipped): what csrc/quicklook_core.hpp computes."""
    xs = modwave * (1.0 + (rv / C_KMS))
    hi = np.clip(np.searchsorted(xs, wave, side='left'), 1, len(xs) - 1)
    lo = hi - 1
    m = (modflux[hi] - modflux[lo]) / (xs[hi] - xs[lo]) * (wave - xs[lo]) + modflux[lo]
    m[(wave < xs[0]) | (wave > xs[-1])] = 1.0
    return np.sum((m - flux) ** 2 / eflux ** 2)


def rv_cases(out):
    rng = np.random.default_rng(1701)
    # a non-uniform, strictly increasing model grid of 1000 pixels
    modwave = 5150.0 + np.cumsum(rng.uniform(0.05, 0.25, NM))
    cen = rng.uniform(modwave[0] + 1, modwave[-1] - 1, 40)
    modflux = lines(modwave, cen, rng.uniform(0.1, 0.7, 40), rng.uniform(0.15, 0.4, 40))
    out["rv_modwave"], out["rv_modflux_clean"] = modwave, modflux.copy()
    modflux_nan = modflux.copy()
    modflux_nan[400] = np.nan                    # reached only by the velocities that bring an observed pixel next to it
    out["rv_modflux"] = modflux_nan
    rv = np.linspace(-1000.0, 1000.0, G)
    out["rv_grid"] = rv
    true_rv = 37.3
    for nobs in NOBS:
        if nobs == 1:
            wave = np.array([modwave[-1] * (1.0 + (rv[5] / C_KMS))])       # on the shifted model's last point for rv[5]
        else:
            wave = np.sort(rng.uniform(modwave[0] + 2.0, modwave[-1] - 2.0, nobs))
            wave[0] = modwave[0] * (1.0 + (rv[40] / C_KMS))                # on the shifted first point for rv[40]
            wave[-1] = modwave[-1] * (1.0 + (rv[20] / C_KMS))              # on the shifted last point for rv[20]
            wave[nobs // 2] = modwave[500] * (1.0 + (rv[33] / C_KMS))      # on an interior point for rv[33] (= 0 km/s)
            wave = np.sort(wave)
            assert np.all(np.diff(wave) > 0)
        eflux = 0.002 * 10.0 ** rng.uniform(0.0, 2.0, nobs)                # two decades of error bars
        xs = modwave * (1.0 + (true_rv / C_KMS))
        flux = np.interp(wave, xs, modflux, left=1.0, right=1.0) + eflux * rng.standard_normal(nobs)
        R = ref.RVcalc(inwave=wave, influx=flux, einflux=eflux, modflux=modflux_nan, modwave=modwave)
        chisq = np.array([R.chisq_rv(v) for v in rv])
        mine = np.array([restated_chisq_rv(modwave, modflux_nan, wave, flux, eflux, v) for v in rv])
        # the tests rely on: the searchsorted-left rule and the installed scipy (which may hand fp64 input to np.interp)
        # agree on these inputs -- no pixel sits on a knot next to the NaN
        assert np.array_equal(np.isnan(chisq), np.isnan(mine)), nobs
        fin = np.isfinite(chisq)
        assert np.all(np.abs(mine[fin] - chisq[fin]) <= 1e-12 * np.abs(chisq[fin])), nobs
        if nobs > 1:
            assert fin.any() and (~fin).any(), "the NaN must be reached by some velocities only"
            assert wave[0] < modwave[0] * (1 + rv[-1] / C_KMS) and wave[-1] > modwave[-1] * (1 + rv[0] / C_KMS)   # off both ends
        out["rv%d_wave" % nobs], out["rv%d_flux" % nobs], out["rv%d_eflux" % nobs] = wave, flux, eflux
        out["rv%d_chisq" % nobs] = chisq
    # brute on the clean model: the grid's argmin and scipy's polish
    nobs = 257
    wave, eflux = out["rv257_wave"], out["rv257_eflux"] * 0.2
    xs = modwave * (1.0 + (true_rv / C_KMS))
    flux = np.interp(wave, xs, modflux, left=1.0, right=1.0) + eflux * rng.standard_normal(nobs)
    R = ref.RVcalc(inwave=wave, influx=flux, einflux=eflux, modflux=modflux, modwave=modwave)
    ranges = ((-300.0, 300.0),)
    grid = np.linspace(ranges[0][0], ranges[0][1], G)
    chisq = np.array([R.chisq_rv(v) for v in grid])
    two = np.sort(chisq)[:2]
    assert (two[1] - two[0]) > 1e-6 * two[0], "the reference's two lowest grid values must differ by more than 1e-6 relative"
    out["rvb_flux"], out["rvb_eflux"], out["rvb_ranges"] = flux, eflux, np.array(ranges)
    out["rvb_grid_chisq"] = chisq
    out["rvb_brute"] = np.atleast_1d(R(ranges=ranges, Ns=G))
    out["rvb_true"] = np.array(true_rv)


def broad_case(out):
    rng = np.random.default_rng(1702)
    n, modres = 1024, 100000.0
    modwave = 5150.0 * np.exp(np.arange(n) / 3.0e5)                        # geometric grid
    px = modwave[1] - modwave[0]
    cen = modwave[0] + (modwave[-1] - modwave[0]) * (np.arange(8) + 0.5 + rng.uniform(-0.2, 0.2, 8)) / 8.0
    modflux = lines(modwave, cen, rng.uniform(0.35, 0.8, 8), rng.uniform(1.3, 1.8, 8) * px)
    eflux = 0.004 * 10.0 ** rng.uniform(0.0, 1.0, n)

    def smooth(b):
        return ref_smoothing.smoothspec(modwave, modflux, resolution=2.355 * b, outwave=modwave, smoothtype='R',
                                        fftsmooth=True, inres=2.355 * modres)
    flux = np.nan_to_num(smooth(0.7 * modres), nan=1.0) + eflux * rng.standard_normal(n)
    # 16 values in [0.5, 0.98] modres for which no broadened pixel lies within 1e-3 of the 0.95 threshold (an fp32 row then
    # cannot flip the mask): candidates on a fine grid, the first passing one of each sixteenth of the range
    cand = np.linspace(0.5, 0.98, 16 * 12 + 1)[:-1].reshape(16, 12) * modres
    values, rows = [], []
    for group in cand:
        for b in group:
            m = smooth(b)
            if not np.any(np.abs(m - 0.95) <= 1e-3):
                values.append(b)
                rows.append(m)
                break
        else:
            raise AssertionError("no value in this part of the range keeps every pixel 1e-3 away from 0.95")
    values, rows = np.array(values), np.array(rows)
    assert len(values) == 16 and not np.any(np.abs(rows - 0.95) <= 1e-3)
    B = ref.BROADcalc(inwave=modwave, influx=flux, einflux=eflux, modflux=modflux, modwave=modwave, modres=modres)
    grid = np.concatenate([[-1.0], values, [modres]])
    chisq = np.array([B.chisq_broad(b) for b in grid])
    assert np.isinf(chisq[0]) and np.isinf(chisq[-1]) and np.all(np.isfinite(chisq[1:-1]))
    with np.errstate(invalid="ignore"):
        kept = (rows < 0.95).sum(axis=1)
    assert np.all(kept > 0) and np.all(kept < n)
    out.update(br_modwave=modwave, br_modflux=modflux, br_flux=flux, br_eflux=eflux, br_modres=np.array(modres),
               br_grid=grid, br_chisq=chisq, br_rows=rows, br_kept=kept.astype(np.int32))
    ranges = ((0.5 * modres, 0.98 * modres),)
    out["br_ranges"] = np.array(ranges)
    out["br_brute"] = np.atleast_1d(B(ranges=ranges, Ns=16))


def pc_cases(out):
    rng = np.random.default_rng(1703)
    modwave, modflux = out["rv_modwave"], out["rv_modflux_clean"]
    for numpoly in (2, 4):
        nobs = 300
        wave = np.sort(rng.uniform(modwave[0] - 1.0, modwave[-1] + 1.0, nobs))   # non-uniform, a little beyond the model
        truth = np.array([1.1, 0.08, -0.05, 0.03])[:numpoly]
        eflux = 0.003 * 10.0 ** rng.uniform(0.0, 1.0, nobs)
        model = np.interp(wave, modwave, modflux, left=1.0, right=1.0)
        flux = model * ref.polycalc(truth, wave) + eflux * rng.standard_normal(nobs)
        P = ref.PCcalc(inwave=wave, influx=flux, einflux=eflux, modflux=modflux, modwave=modwave, numpoly=numpoly)
        got = np.asarray(P()[0])
        # closed form: chi^2 = |A pc - b|^2, A = chebvander(x) / e, b = (flux / model) / e
        span = wave - wave.min()
        x = 2.0 * (span / span.max()) - 1.0
        A = chebvander(x, numpoly - 1) / eflux[:, None]
        b = (flux / model) / eflux
        exact = np.linalg.lstsq(A, b, rcond=None)[0]
        assert P.chisq_pc(exact) <= P.chisq_pc(got) * (1 + 1e-12)
        k = "pc%d_" % numpoly
        out[k + "wave"], out[k + "flux"], out[k + "eflux"] = wave, flux, eflux
        out[k + "ref"], out[k + "exact"], out[k + "ref_chisq"] = got, exact, np.array(P.chisq_pc(got))


def main():
    out = {}
    rv_cases(out)
    broad_case(out)
    pc_cases(out)
    out["versions"] = np.array(json.dumps(dict(numpy=np.__version__, scipy=scipy.__version__)))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 700 * 1024, size
    print("wrote %s (%.1f KB)" % (OUT, size / 1e3))


if __name__ == "__main__":
    main()
