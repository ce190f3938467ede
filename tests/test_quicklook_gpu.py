"""The quick-look scans on the MI355X: payne_rv_scan and payne_chisq_below (csrc/k_quicklook.hip) and the classes built on
them (thepayne_amd/fitting/fitutils.py) against what the reference's classes gave on the same inputs (g17,
tools/freeze_quicklook_golden.py).  The arithmetic on the host: tests/test_quicklook.py."""
import numpy as np
import pytest

import oracle as O
from thepayne_amd import synth
from test_gpu_parity import FLUX_TOL
from test_quicklook import NOBS, below_cases, below_reference

pytestmark = pytest.mark.gpu


def _rvcalc(g, nobs, modflux="rv_modflux"):
    from thepayne_amd.fitting.fitutils import RVcalc
    return RVcalc(inwave=g["rv%d_wave" % nobs], influx=g["rv%d_flux" % nobs], einflux=g["rv%d_eflux" % nobs],
                  modflux=g[modflux], modwave=g["rv_modwave"])


@pytest.mark.parametrize("nobs", NOBS)
def test_rv_scan_matches_the_reference_on_the_whole_grid(golden, nobs):
    """1000 model pixels on a non-uniform grid, 67 velocities that push the observed pixels off either end of the model, pixels
    exactly on a shifted end point and on an interior point, one NaN model pixel that only some velocities reach, error bars
    over two decades: relative 1e-10 on every finite value (derivation: tests/test_quicklook.py), NaN where the reference is
    NaN, the same bits on a second call; then G = 1 through the scalar method."""
    g = golden("g17_quicklook")
    R = _rvcalc(g, nobs)
    rv, ref = g["rv_grid"], g["rv%d_chisq" % nobs]
    got = R.scan(rv)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    rel = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    print("nobs %d: max relative difference %.3g" % (nobs, rel.max()))
    assert np.all(rel <= 1e-10), rv[fin][rel > 1e-10]
    assert got.tobytes() == R.scan(rv).tobytes()
    for k in (0, 33, int(np.flatnonzero(~fin)[0]) if (~fin).any() else 66):           # G = 1: the same block, the same bits
        one = R.chisq_rv(np.array([rv[k]]))
        assert np.array([one]).tobytes() == got[k:k + 1].tobytes()


def test_rv_scan_refuses_malformed_calls(golden):
    from thepayne_amd import _lib
    lib = _lib.load()
    g = golden("g17_quicklook")
    mw, mf = g["rv_modwave"].copy(), g["rv_modflux_clean"].copy()
    w, f, e = (g["rv63_" + k].copy() for k in ("wave", "flux", "eflux"))
    rv, out = np.zeros(1), np.zeros(1)

    def call(mw_=mw, nm=len(mw), nobs=63, G=1, rv_=rv):
        return lib.payne_rv_scan(0, mw_.ctypes.data, mf.ctypes.data, nm, w.ctypes.data, f.ctypes.data, e.ctypes.data, nobs,
                                 None if rv_ is None else rv_.ctypes.data, G, out.ctypes.data)
    assert call() == 0
    flat = mw.copy()
    flat[7] = flat[6]
    for bad in (call(nm=1), call(nobs=0), call(G=0), call(rv_=None), call(mw_=flat)):
        assert bad == _lib.E_INVALID


def test_rvcalc_finds_the_reference_velocity(golden):
    """RVcalc()(ranges, Ns=67) against the reference's brute: the same grid argmin (the freeze script asserts that the
    reference's two lowest grid values differ by more than 1e-6 relative), and the polished velocity within 5e-4 km/s: fmin's
    default xtol is 1e-4, two runs each stop within xtol of the same local minimum, 5 xtol is the margin."""
    from thepayne_amd.fitting.fitutils import RVcalc
    g = golden("g17_quicklook")
    R = RVcalc(inwave=g["rv257_wave"], influx=g["rvb_flux"], einflux=g["rvb_eflux"], modflux=g["rv_modflux_clean"],
               modwave=g["rv_modwave"])
    lo, hi = g["rvb_ranges"][0]
    grid = np.linspace(lo, hi, 67)
    assert int(np.argmin(R.scan(grid))) == int(np.argmin(g["rvb_grid_chisq"]))
    out = R(ranges=((lo, hi),), Ns=67)
    print("velocity %.9g, reference %.9g" % (out[0], g["rvb_brute"][0]))
    assert out.shape == (1,) and abs(out[0] - g["rvb_brute"][0]) <= 5e-4


def test_chisq_below_matches_numpy_compaction():
    """payne_chisq_below on synthetic device rows: n in {1, 64, 1000} with ld > n, NaN runs at both ends, rows with nothing
    kept (chisq = 0, n_kept = 0) and everything kept; n_kept exact, chi^2 within relative 1e-12 (a sum of <= 1000 positive
    terms in another order: 1000 * 2^-53 ~ 1e-13), the same bits on a second call."""
    import torch
    from thepayne_amd import _lib
    lib = _lib.load()
    for rows, n, flux, eflux in below_cases():
        G, ld = rows.shape
        ref_chisq, ref_kept = below_reference(rows, n, flux, eflux, 0.95)
        assert ref_kept[1] == 0 and ref_chisq[1] == 0.0 and ref_kept[2] == n
        dev = torch.as_tensor(rows).to("cuda:0")
        res = []
        for _ in range(2):
            chisq, kept = np.full(G, -1.0), np.full(G, -1, dtype=np.int32)
            rc = lib.payne_chisq_below(0, dev.data_ptr(), ld, n, G, flux.ctypes.data, eflux.ctypes.data, 0.95, chisq.ctypes.data,
                                       kept.ctypes.data, None)
            assert rc == 0
            res.append((chisq, kept))
        assert np.array_equal(res[0][1], ref_kept), n
        assert np.all(np.abs(res[0][0] - ref_chisq) <= 1e-12 * np.abs(ref_chisq)), n
        assert res[0][0].tobytes() == res[1][0].tobytes()
    assert lib.payne_chisq_below(0, dev.data_ptr(), ld, ld + 1, G, flux.ctypes.data, eflux.ctypes.data, 0.95, chisq.ctypes.data,
                                 kept.ctypes.data, None) == _lib.E_INVALID


def test_broadcalc_scan_matches_the_reference_grid(golden):
    """BROADcalc.scan on the 1024-pixel geometric model: 16 values in [0.5, 0.98] modres plus one < 0 and one >= modres (inf).
    The freeze script asserts that no broadened reference pixel lies within 1e-3 of 0.95, so the fp32 rows cannot flip the
    mask: n_kept equals the reference's count.  chi^2: the rows are fp32-class, eps = FLUX_TOL per pixel (what
    tests/test_gpu_parity.py allows a model flux), so |chi^2 - ref| <= sum_i (2 |m_i - o_i| eps + eps^2) / s_i^2 over the
    reference's kept pixels with its pairing of the error bars."""
    from thepayne_amd.fitting.fitutils import BROADcalc
    g = golden("g17_quicklook")
    B = BROADcalc(inwave=g["br_modwave"], influx=g["br_flux"], einflux=g["br_eflux"], modflux=g["br_modflux"],
                  modwave=g["br_modwave"], modres=float(g["br_modres"]))
    grid, ref = g["br_grid"], g["br_chisq"]
    got = B.scan(grid)
    assert np.isinf(got[0]) and np.isinf(got[-1]) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.array_equal(B.n_kept[1:-1], g["br_kept"]) and B.n_kept[0] == -1 and B.n_kept[-1] == -1
    eps = FLUX_TOL
    for k, m in enumerate(g["br_rows"]):
        with np.errstate(invalid="ignore"):
            cond = m < 0.95
        mk, ok = m[cond], g["br_flux"][cond]
        sk = g["br_eflux"][:len(mk)]
        bound = np.sum((2.0 * np.abs(mk - ok) * eps + eps ** 2) / sk ** 2)
        print("broad %.1f: chi^2 %.6f, reference %.6f, difference %.3g, bound %.3g" % (grid[k + 1], got[k + 1], ref[k + 1], abs(got[k + 1] - ref[k + 1]), bound))
        assert abs(got[k + 1] - ref[k + 1]) <= bound, grid[k + 1]
    assert B.chisq_broad(np.array([grid[3]])) == got[3]


def _sed_problem():
    phot = synth.make_phot_nets()
    truth = {'FeH': -0.15, 'logA': 2.9, 'Av': 0.2}
    fixed = {'Teff': 5850.0, 'logg': 4.3, 'aFe': 0.1}
    return phot, truth, fixed


def test_sedopt_recovers_the_parameters_behind_synthetic_magnitudes():
    """Magnitudes generated from known parameters through payne_sed_batch; the free parameters (FeH, logA, Av) are recovered:
    chi^2 at the result <= 1e-12, and the result as close to the truth as scipy's Nelder-Mead stops on the oracle's restatement
    of the SED for the same inputs, times 4 (distance: Euclidean, logA in units of its starting value 3, FeH and Av -- started
    at 0 -- in dex / mag).  Teff is fixed here: a simplex around 6000 K cannot meet the reference's absolute 1e-14 on x (one
    ulp of 6000 is 9e-13) and runs to its 1e5 iterations, in the reference as here -- half a minute, too long for a test."""
    from scipy.optimize import minimize
    from thepayne_amd.fitting.fitutils import SEDopt
    from thepayne_amd.predict.predictsed import FastPayneSEDPredict
    phot, truth, fixed = _sed_problem()
    S = FastPayneSEDPredict(usebands=phot["filters"], nnpath=phot)
    pars = np.array([[np.log10(fixed['Teff']), fixed['logg'], truth['FeH'], fixed['aFe'], truth['Av'], 3.1, np.nan, np.nan, truth['logA']]])
    mags = S.sed_batch(pars).cpu().numpy()[0]
    inputphot = {f: (m, 0.05) for f, m in zip(phot["filters"], mags)}
    init = {'Teff': 6000.0, 'FeH': 0.0, 'logg': 4.44, 'aFe': 0.0, 'logA': 3.0, 'Av': 0.0}
    fit = SEDopt(inputphot=inputphot, photANNpath=phot, fixedpars=fixed, initpars=init, returnsed=True)
    assert fit.fitpars == ['FeH', 'logA', 'Av']
    output, sedmod = fit()
    x = output[0]
    chisq = fit.chisq_sed(x)
    oph = dict(phot)
    oph["hiav"] = np.array(S.HiAv.Avlist, dtype=float)

    def oracle_chisq(p):
        m = O.sed_mags(oph, np.log10(fixed['Teff']), fixed['logg'], p[0], fixed['aFe'], av=p[2], rv=3.1, logA=p[1])
        return np.sum((m - mags) ** 2 / 0.05 ** 2)
    xo = minimize(oracle_chisq, [0.0, 3.0, 0.0], method='Nelder-Mead', tol=1e-14, options={'maxiter': 1e5}).x
    t, scale = np.array([truth['FeH'], truth['logA'], truth['Av']]), np.array([1.0, 3.0, 1.0])
    d, d_oracle = np.linalg.norm((x - t) / scale), np.linalg.norm((xo - t) / scale)
    print("chi^2 %.3g; distance from the truth %.3g, oracle run %.3g; x = %s" % (chisq, d, d_oracle, x))
    assert list(sedmod.keys()) == list(phot["filters"])
    assert np.allclose([sedmod[f] for f in phot["filters"]], mags, atol=1e-9)
    assert chisq <= 1e-12
    assert d <= 4.0 * d_oracle


def test_sedopt_wants_every_parameter_fitted_or_fixed():
    """The fitted / fixed split of fitutils.py:308-320 around the reference's defaults: the fitted and the fixed parameters
    together must be exactly the model's.  A fixed logA while initpars names a luminosity (the model is then Teff, logg, FeH,
    aFe, logL, Dist, Av), or a fixed parameter the model does not take, leaves the count wrong: IOError."""
    from thepayne_amd.fitting.fitutils import SEDopt
    phot, _, _ = _sed_problem()
    inputphot = {f: (10.0, 0.05) for f in phot["filters"]}
    defaults = {'logg': 4.44, 'aFe': 0.0, 'Av': 0.0}
    with pytest.raises(IOError):
        SEDopt(inputphot=inputphot, photANNpath=phot, fixedpars=dict(defaults, logA=3.0),
               initpars={'Teff': 6000.0, 'FeH': 0.0, 'logL': 0.0, 'Dist': 100.0})
    with pytest.raises(IOError):
        SEDopt(inputphot=inputphot, photANNpath=phot, fixedpars=dict(defaults, Rv=3.1))
    assert SEDopt(inputphot=inputphot, photANNpath=phot).fitpars == ['Teff', 'FeH', 'logA']
