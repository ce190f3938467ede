"""Payne/fitting/fitutils.py: the small host-side helpers of the fit (numpy) and the four quick-look classes a user runs
before FitPayne to centre the Vrad, Inst_R, pc_* and Teff / logA priors.  The two grid scans (RVcalc, BROADcalc) evaluate
their whole grid on the GPU (csrc/k_quicklook.hip); the simplex polish and the two small fits (PCcalc, SEDopt) are scipy's,
on the host.  scipy is imported where it is used: the package imports without it."""
import numpy as np
from numpy.polynomial.chebyshev import chebval

__all__ = ["polycalc", "airtovacuum", "vacuumtoair", "RVcalc", "BROADcalc", "PCcalc", "SEDopt"]


def polycalc(coef, inwave):
    """Chebyshev blaze on the wavelength range rescaled to [-1, 1]
    (Payne/fitting/fitutils.py:11-20).  The batched likelihood evaluates the same
    series on the GPU (post_core.hpp, phase_obs); this host version backs the
    public helper."""
    inwave = np.asarray(inwave, dtype=np.float64)
    span = inwave - inwave.min()
    return chebval(2.0 * (span / span.max()) - 1.0, coef)


def airtovacuum(inwave):
    """Ciddor (1996) air -> vacuum (Payne/fitting/fitutils.py:22-37); applied once
    to the observed wavelengths when inputdict['spec']['convertair'] is set."""
    mu = np.asarray(inwave, dtype=np.float64) * 1e-4          # micron
    s2 = 1.0 / mu ** 2.0
    refr = 0.0 + (5.792105e-2 / (238.0185 - s2)) + (1.67917e-3 / (57.362 - s2))
    return (mu * (refr + 1)) * 1e4


def vacuumtoair(inwave):
    """Payne/fitting/fitutils.py:39-44."""
    inwave = np.asarray(inwave, dtype=np.float64)
    s2 = ((10 ** 4) / inwave) ** 2.0
    return inwave / (1.0 + 0.0000834254 + 0.02406147 / (130.0 - s2) + 0.00015998 / (38.9 - s2))


def _scipy_optimize():
    try:
        from scipy import optimize
    except ImportError as e:
        raise ImportError("the quick-look fits (RVcalc, BROADcalc, PCcalc, SEDopt) need scipy (scipy.optimize): %s" % (e,))
    return optimize


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _strictly_increasing(modwave):
    if modwave.ndim != 1 or len(modwave) < 2 or not np.all(np.diff(modwave) > 0.0):
        raise ValueError("modwave must be one-dimensional and strictly increasing (at least two pixels)")


def _interp_fill(modwave, modflux, wave):
    """interp1d(modwave, modflux, kind='linear', bounds_error=False, fill_value=1.0)(wave) by interp1d's own rule: bracket
    by searchsorted (side left) clipped to [1, nm - 1], both end points inside, 1.0 outside (quicklook_core.hpp, interp_fill)."""
    hi = np.clip(np.searchsorted(modwave, wave, side='left'), 1, len(modwave) - 1)
    lo = hi - 1
    slope = (modflux[hi] - modflux[lo]) / (modwave[hi] - modwave[lo])
    out = slope * (wave - modwave[lo]) + modflux[lo]
    out[(wave < modwave[0]) | (wave > modwave[-1])] = 1.0
    return out


def _brute_1d(scan, scalar, ranges, Ns):
    """scipy.optimize.brute(scalar, ranges, Ns) for one dimension with its default finish=fmin, the grid evaluated by one
    batched `scan`: Ns values from lo to hi, end points included (or lo, hi, step as brute takes them), the simplex started
    from the grid's argmin.  Returns a length-1 array, as brute does."""
    opt = _scipy_optimize()
    if len(ranges) != 1:
        raise ValueError("the quick-look scans are one-dimensional: ranges=((lo, hi),)")
    r = tuple(ranges[0].indices(2 ** 62)) if isinstance(ranges[0], slice) else tuple(ranges[0])
    grid = np.linspace(r[0], r[1], int(Ns)) if len(r) < 3 else np.arange(r[0], r[1], r[2], dtype=np.float64)
    chisq = scan(grid)
    x0 = grid[int(np.argmin(chisq))]
    return np.atleast_1d(opt.fmin(scalar, x0, full_output=1, disp=False)[0])


def _no_gpu():
    # (the error utils/smoothing.py raises without a GPU: the scans have no CPU path either)
    return RuntimeError("the quick-look scans need a ROCm GPU (there is no CPU fallback)")


class RVcalc(object):
    """Brute-force radial-velocity scan (Payne/fitting/fitutils.py:46-94): chi^2 of the observed spectrum against the model
    interpolated from its Doppler-shifted grid, on a grid of velocities, then scipy's fmin from the best grid value.
    New: ``scan(rvs)``, the whole grid in one payne_rv_scan call."""

    def __init__(self, **kwargs):
        self.wave = kwargs.get('inwave', [])
        self.flux = kwargs.get('influx', [])
        self.eflux = kwargs.get('einflux', [])
        self.modflux = kwargs.get('modflux', [])
        self.modwave = kwargs.get('modwave', [])
        self.device = kwargs.get('device', None)

    def __call__(self, **kwargs):
        return _brute_1d(self.scan, self.chisq_rv, kwargs.get('ranges', ((-1000, 1000),)), kwargs.get('Ns', 1000))

    def chisq_rv(self, rv):
        return float(self.scan(np.ravel(rv)[:1])[0])

    def scan(self, rvs):
        """chisq[len(rvs)] (fp64) for the velocities `rvs` (km/s)."""
        rvs = _f64(np.ravel(rvs))
        modwave, modflux = _f64(self.modwave), _f64(self.modflux)
        wave, flux, eflux = _f64(self.wave), _f64(self.flux), _f64(self.eflux)
        _strictly_increasing(modwave)
        if modflux.shape != modwave.shape:
            raise ValueError("modflux and modwave differ in shape")
        if wave.ndim != 1 or len(wave) < 1 or flux.shape != wave.shape or eflux.shape != wave.shape:
            raise ValueError("inwave, influx and einflux must be one-dimensional, of one length, and not empty")
        if len(rvs) == 0:
            return np.empty(0)
        import torch
        if not torch.cuda.is_available():
            raise _no_gpu()
        from .. import _lib
        lib = _lib.load()
        dev = torch.cuda.current_device() if self.device is None else int(self.device)
        out = np.empty(len(rvs))
        rc = lib.payne_rv_scan(dev, modwave.ctypes.data, modflux.ctypes.data, len(modwave), wave.ctypes.data, flux.ctypes.data,
                               eflux.ctypes.data, len(wave), rvs.ctypes.data, len(rvs), out.ctypes.data)
        if rc == _lib.E_INVALID:
            raise ValueError("payne_rv_scan: invalid arguments")
        if rc != 0:
            raise RuntimeError("payne_rv_scan failed (%d)" % rc)
        return out


class BROADcalc(object):
    """Brute-force instrumental-resolution scan (Payne/fitting/fitutils.py:96-155): the model broadened from ``modres`` to
    each grid value (smoothspec, smoothtype 'R', on its own grid), chi^2 over the pixels whose broadened flux is below 0.95.
    As in the reference the observed spectrum is on the model's grid.  New: ``scan(broads)``: the rows are broadened in
    batches through the likelihood's kernels and reduced by payne_chisq_below without leaving the device."""

    b_max = 256                      # rows per payne_smooth_batch call: the default grid of 1000 values takes four
    threshold = 0.95                 # fitutils.py:148

    def __init__(self, **kwargs):
        self.wave = kwargs.get('inwave', [])
        self.flux = kwargs.get('influx', [])
        self.eflux = kwargs.get('einflux', [])
        self.modflux = kwargs.get('modflux', [])
        self.modwave = kwargs.get('modwave', [])
        self.modres = kwargs.get('modres', 300000.0)
        self.device = kwargs.get('device', None)
        self.n_kept = None           # pixels below the threshold for each value of the last scan (-1 where chi^2 is inf)

    def __call__(self, **kwargs):
        return _brute_1d(self.scan, self.chisq_broad, kwargs.get('ranges', ((27000, 35000),)), kwargs.get('Ns', 1000))

    def chisq_broad(self, broad):
        return float(self.scan(np.ravel(broad)[:1])[0])

    def scan(self, broads):
        """chisq[len(broads)] (fp64); inf for values < 0 or >= modres (fitutils.py:138-141), without GPU work."""
        broads = _f64(np.ravel(broads))
        modwave, modflux = _f64(self.modwave), _f64(self.modflux)
        flux, eflux = _f64(self.flux), _f64(self.eflux)
        _strictly_increasing(modwave)
        if modflux.shape != modwave.shape:
            raise ValueError("modflux and modwave differ in shape")
        if flux.shape != modwave.shape or eflux.shape != modwave.shape:
            raise ValueError("influx and einflux must be on the model's grid (the reference masks them with the model's "
                             "pixels): %d and %d values for %d model pixels" % (flux.size, eflux.size, modwave.size))
        if np.size(self.wave) and not np.array_equal(_f64(self.wave), modwave):
            raise ValueError("inwave is not the model's grid: the observed spectrum must be on modwave")
        out = np.full(len(broads), np.inf)
        self.n_kept = np.full(len(broads), -1, dtype=np.int32)
        on = ~((broads < 0.0) | (broads >= self.modres))
        if on.any():
            out[on], self.n_kept[on] = self._scan_device(broads[on], modwave, modflux, flux, eflux)
        return out

    def _scan_device(self, broads, modwave, modflux, flux, eflux):
        import torch
        if not torch.cuda.is_available():
            raise _no_gpu()
        from .. import _lib
        from ..utils.smoothing import _Smoother
        sm = self.__dict__.setdefault('_smoother', _Smoother(device=self.device))
        dev = sm._device_index()
        # smoothspec(modwave, modflux, resolution=2.355 broad, outwave=modwave, smoothtype='R', inres=2.355 modres): the path
        # PayneSpecPredict.smoothspec takes (predict/_spec.py), stage 2 of a context whose model grid is modwave
        eng = sm._smooth_engine(modwave, 2.355 * float(self.modres), b_max=self.b_max)
        eng.set_obs(modwave)
        lib, n = eng.lib, len(modwave)
        spec = torch.as_tensor(np.nan_to_num(modflux, nan=1.0).astype(np.float32)).to(eng.device)     # smoothing.py:137-138
        spec = spec.expand(min(self.b_max, len(broads)), n).contiguous()
        # np.interp(outwave, exp(linspace(ln wmin, ln wmax, n2)), conv, left = right = NaN): an end pixel is NaN whenever
        # exp(log(w)) rounds to the inside of w (predict/_spec.py, native_grid_edges); NaN is below no threshold
        lo, hi = np.exp(np.log(modwave.min())), np.exp(np.log(modwave.max()))
        edge = np.flatnonzero((modwave < lo) | (modwave > hi))
        chisq, kept = np.empty(len(broads)), np.empty(len(broads), dtype=np.int32)
        for s in range(0, len(broads), self.b_max):
            m = min(self.b_max, len(broads) - s)
            th = np.full((m, eng.ncols), np.nan)
            th[:, :6] = [5000.0, 4.0, 0.0, 0.0, 0.0, 0.0]
            th[:, 7] = 2.355 * broads[s:s + m]
            rows = eng.smooth_batch(spec[:m], th, stage=2)
            if len(edge):
                rows[:, torch.as_tensor(edge, device=rows.device)] = float("nan")
            c, k = chisq[s:s + m], kept[s:s + m]
            rc = lib.payne_chisq_below(dev, rows.data_ptr(), rows.stride(0), n, m, flux.ctypes.data, eflux.ctypes.data,
                                       float(self.threshold), c.ctypes.data, k.ctypes.data, eng._stream())
            if rc != 0:
                raise RuntimeError("payne_chisq_below failed (%d)" % rc)
        return chisq, kept


class PCcalc(object):
    """Blaze-polynomial fit (Payne/fitting/fitutils.py:159-196): Nelder-Mead from [1, 0, ...] on chi^2 of the Chebyshev
    series ``polycalc(pc, inwave)`` against influx / model, the model interpolated onto inwave (fill value 1.0) once.
    Host only: the objective is a dot product."""

    def __init__(self, **kwargs):
        self.wave = kwargs.get('inwave', [])
        self.flux = kwargs.get('influx', [])
        self.eflux = kwargs.get('einflux', [])
        self.modflux = kwargs.get('modflux', [])
        self.modwave = kwargs.get('modwave', [])
        self.numpoly = kwargs.get('numpoly', 4)
        self._target = None

    def __call__(self):
        opt = _scipy_optimize()
        self._target = None
        start = np.zeros(int(self.numpoly))
        start[0] = 1.0
        return [opt.minimize(self.chisq_pc, start, method='Nelder-Mead', tol=1e-14, options={'maxiter': 1e4}).x]

    def _ratio(self):
        """(x in [-1, 1], influx / model, 1 / einflux): constant during the fit."""
        if self._target is None:
            wave, modwave = _f64(self.wave), _f64(self.modwave)
            _strictly_increasing(modwave)
            span = wave - wave.min()
            self._target = (2.0 * (span / span.max()) - 1.0,
                            _f64(self.flux) / _interp_fill(modwave, _f64(self.modflux), wave), 1.0 / _f64(self.eflux))
        return self._target

    def chisq_pc(self, pc):
        x, ratio, inv_e = self._ratio()
        r = (chebval(x, pc) - ratio) * inv_e
        return float(np.dot(r, r))


class SEDopt(object):
    """Photometric Nelder-Mead fit (Payne/fitting/fitutils.py:286-406): every parameter of the SED model is either fitted
    (started from ``initpars``) or fixed (``fixedpars``); the objective is chi^2 of FastPayneSEDPredict.sed -- on the GPU in
    this build -- against ``inputphot`` = {filter: (mag, err)}."""

    def __init__(self, **kwargs):
        self.inputphot = kwargs.get('inputphot', {})
        self.fixedpars = kwargs.get('fixedpars', {'logg': 4.44, 'aFe': 0.0, 'Av': 0.0})
        self.filterarray = [f for f in self.inputphot.keys() if f != 'photANNpath']
        photANNpath = self.inputphot['photANNpath'] if 'photANNpath' in self.inputphot else kwargs.get('photANNpath', None)
        self.returnsed = kwargs.get('returnsed', False)
        self.init_p0 = kwargs.get('initpars', {'Teff': 6000.0, 'FeH': 0.0, 'logg': 4.44, 'aFe': 0.0, 'logA': 3.0, 'Av': 0.0})
        self.tol = kwargs.get('tol', 1e-15)              # (kept, as in the reference, but the fit runs at 1e-14 / 1e5: :332-338)
        self.maxiter = kwargs.get('maxiter', 1e5)
        self.verbose = kwargs.get('verbose', False)
        # luminosity and distance, or the normalisation logA (:308-320)
        if 'logL' in self.fixedpars or 'logL' in self.init_p0:
            allpars = ['Teff', 'logg', 'FeH', 'aFe', 'logL', 'Dist', 'Av']
        else:
            allpars = ['Teff', 'logg', 'FeH', 'aFe', 'logA', 'Av']
        self.fitpars = [p for p in allpars if p not in self.fixedpars]
        if len(self.fitpars) + len(self.fixedpars) != len(allpars):
            raise IOError("every SED parameter must be either fitted or fixed: fitted %s, fixed %s, the model takes %s"
                          % (self.fitpars, list(self.fixedpars), allpars))
        from ..predict.predictsed import FastPayneSEDPredict
        self.fsed = FastPayneSEDPredict(usebands=self.filterarray, nnpath=photANNpath, **kwargs.get('sedkwargs', {}))

    def _sed(self, values):
        p = dict(zip(self.fitpars, values))
        p.update(self.fixedpars)
        kw = dict(logt=np.log10(p['Teff']), logg=p['logg'], feh=p['FeH'], afe=p['aFe'], av=p['Av'])
        if 'logL' in p:
            kw.update(logl=p['logL'], dist=p['Dist'])
        else:
            kw['logA'] = p['logA']
        return dict(zip(self.filterarray, self.fsed.sed(**kw)))

    def __call__(self):
        opt = _scipy_optimize()
        start = [self.init_p0[p] for p in self.fitpars]
        output = [opt.minimize(self.chisq_sed, start, method='Nelder-Mead', tol=1e-14,
                               options={'maxiter': 1e5, 'disp': self.verbose}).x]
        if self.returnsed:
            return output, self._sed(output[0])
        return output

    def chisq_sed(self, pars):
        sedmod = self._sed(pars)
        return float(np.sum([((sedmod[f] - self.inputphot[f][0]) ** 2.0) / (self.inputphot[f][1] ** 2.0) for f in self.filterarray]))
