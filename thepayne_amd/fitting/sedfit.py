"""SED fits for many stars at once on the GPU: the photometric magnitudes' derivatives and a Levenberg-Marquardt fit of them.

``SEDFit.grad`` returns the likelihood's magnitudes (``GenMod.genphot`` / ``genphot_scaled``) and their derivatives with respect to
every parameter of the row; ``SEDFit.fit`` fits the free parameters of every star to its observed magnitudes in ONE launch
(payne_sedfit_run; include/payne_hip.h states the rules): a point estimate, its Fisher matrix and Cramer-Rao errors, usable as
starting points and prior centres for ``FitPayne``'s photometric block.  A row is ``[Teff, logg, FeH, aFe, logR, Dist, Av]``, or
``[Teff, logg, FeH, aFe, logA, Av]`` with ``photscale``; Rv is 3.1, as in the likelihood.

This is not ``SEDopt``: that minimises chi^2 for one star by Nelder-Mead on the host and stays as it is.
"""
import ctypes as C

import numpy as np

from .. import _lib

__all__ = ["SEDFit", "PARS_DIST", "PARS_SCALED", "check_fit_args"]

PARS_DIST = ("Teff", "logg", "FeH", "aFe", "logR", "Dist", "Av")
PARS_SCALED = ("Teff", "logg", "FeH", "aFe", "logA", "Av")
AV_MAX = 5.0                                         # the reference's model jumps there (predictsed.py:86-90)
WIDE = {"logR": (-3.0, 3.5), "Dist": (1e-1, 1e6), "logA": (-20.0, 20.0)}
LM_DEFAULTS = dict(lambda0=1e-3, down=10.0, up=10.0, lambda_min=1e-12, lambda_max=1e8, xtol=1e-3, maxiter=50)


def par_names(photscale):
    return PARS_SCALED if photscale else PARS_DIST


def default_box(xmin, xmax, photscale):
    """(lo, hi) [P]: the nets' range for the labels and Av (below 5), wide ranges for logR / Dist / logA."""
    names = par_names(photscale)
    lo, hi = np.empty(len(names)), np.empty(len(names))
    for p, nm in enumerate(names):
        if p < 4:
            lo[p], hi[p] = xmin[p], xmax[p]
        elif nm == "Av":
            lo[p], hi[p] = xmin[4], min(xmax[4], np.nextafter(AV_MAX, 0.0))
        else:
            lo[p], hi[p] = WIDE[nm]
    return lo, hi


def check_fit_args(mags, emags, start, F, xmin, xmax, photscale=False, free=("Teff", "logR", "Av"), bounds=None, prior=None, N=None, **opts):
    """What ``SEDFit.fit`` checks of host arrays; no GPU.  Returns dict(obs, w [N, F]; start [N, P]; cols (the free parameters' columns,
    ascending: the order of every K-sized result); lo, hi [K]; mu, sigma [N, K] or None; opts).  mags None: the per-star arrays are
    on the device and N says how many stars; obs, w and start come back None."""
    names = par_names(photscale)
    P = len(names)
    if mags is not None:
        mags, emags = np.atleast_2d(np.asarray(mags, dtype=np.float64)), np.atleast_2d(np.asarray(emags, dtype=np.float64))
        start = np.atleast_2d(np.asarray(start, dtype=np.float64))
        if mags.ndim != 2 or mags.shape[1] != F or emags.shape != mags.shape:
            raise ValueError("mags and emags must be [N, %d], got %s and %s" % (F, mags.shape, emags.shape))
        N = mags.shape[0]
        if start.shape != (N, P):
            raise ValueError("start must be [%d, %d] (%s), got %s" % (N, P, ", ".join(names), start.shape))
    free = [free] if isinstance(free, str) else list(free)
    if not free or len(set(free)) != len(free) or any(f not in names for f in free):
        raise ValueError("free must name parameters among %s, each once; got %r" % (names, free))
    cols = sorted(names.index(f) for f in free)
    K = len(cols)
    lo_all, hi_all = default_box(np.asarray(xmin, dtype=np.float64), np.asarray(xmax, dtype=np.float64), photscale)
    if bounds is not None:
        if isinstance(bounds, dict):
            for nm, (a, b) in bounds.items():
                if nm not in names:
                    raise ValueError("bounds names %r, which is not among %s" % (nm, names))
                lo_all[names.index(nm)], hi_all[names.index(nm)] = float(a), float(b)
        else:
            bb = np.asarray(bounds, dtype=np.float64)
            if bb.shape != (P, 2):
                raise ValueError("bounds must be a dict or [%d, 2], got %s" % (P, bb.shape))
            lo_all, hi_all = bb[:, 0].copy(), bb[:, 1].copy()
    lo, hi = lo_all[cols], hi_all[cols]
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("bounds must be finite with lo < hi")
    if "Av" in free and not hi_all[P - 1] < AV_MAX:
        raise ValueError("the upper Av bound must be below %g: the model jumps there" % AV_MAX)
    mu = sigma = None
    if prior is not None:
        mu, sigma = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in prior)
        if mu.shape != (N, K) or sigma.shape != (N, K):
            raise ValueError("prior must be (mu [%d, %d], sigma [%d, %d]), columns in the row's order" % (N, K, N, K))
        if np.any(np.isnan(sigma)) or np.any(sigma <= 0.0) or np.any(np.isnan(mu) & np.isfinite(sigma)):
            raise ValueError("prior sigmas must be positive (inf: no prior) and their centres numbers")
        mu = np.where(np.isfinite(sigma), mu, 0.0)
    if "logR" in free and "Dist" in free:
        k1, k2 = cols.index(names.index("logR")), cols.index(names.index("Dist"))
        if sigma is None or not np.all(np.isfinite(sigma[:, k1]) | np.isfinite(sigma[:, k2])):
            raise ValueError("logR and Dist are exactly degenerate in the magnitudes: every star needs a finite prior sigma on one of them")
    unknown = set(opts) - set(LM_DEFAULTS)
    if unknown:
        raise TypeError("unknown options %s" % sorted(unknown))
    o = dict(LM_DEFAULTS, **opts)
    vals = [float(o[k]) for k in ("lambda0", "down", "up", "lambda_min", "lambda_max", "xtol")]
    if not (all(np.isfinite(vals)) and o["lambda_min"] >= 0 and o["lambda_max"] >= o["lambda_min"] and o["lambda_min"] <= o["lambda0"] <= o["lambda_max"]
            and o["down"] >= 1 and o["up"] >= 1 and o["xtol"] >= 0 and int(o["maxiter"]) == o["maxiter"] and o["maxiter"] >= 1):
        raise ValueError("an option is out of range: %r" % o)
    res = dict(obs=None, w=None, start=None, cols=cols, lo=lo, hi=hi, mu=mu, sigma=sigma, opts=o)
    if mags is not None:
        ok = np.isfinite(mags) & np.isfinite(emags) & (emags > 0.0)
        res.update(obs=np.where(ok, mags, 0.0), w=np.where(ok, 1.0 / np.where(ok, emags, 1.0) ** 2, 0.0), start=np.ascontiguousarray(start))
    return res


class SEDFit(object):
    """SEDFit(usebands=None, nnpath=None, photscale=False, device=None): the per-filter nets are loaded as ``FastPayneSEDPredict``
    loads them (``nnpath`` may be an already stacked dict, whose ``hiav`` [F, 5], if present, replaces the shipped high-Av table)."""

    def __init__(self, usebands=None, nnpath=None, photscale=False, device=None):
        from .. import nnio
        from ..engine import highav_coefficients
        if usebands is None:
            from ..predict.predictsed import _ALLFILTERS
            usebands = _ALLFILTERS
        self.filternames = list(usebands)
        self.photscale = bool(photscale)
        self.names = par_names(self.photscale)
        st = nnio.load_phot_nets(self.filternames, nnpath)
        F, H = st["w1"].shape[0], st["w1"].shape[1]
        if H > _lib.SEDFIT_MAX_H:
            raise NotImplementedError("nets of width %d: payne_sedfit handles up to %d" % (H, _lib.SEDFIT_MAX_H))
        self.F, self.H = F, H
        self.xmin, self.xmax = np.asarray(st["xmin"], dtype=np.float64).copy(), np.asarray(st["xmax"], dtype=np.float64).copy()
        hiav = st.get("hiav") if isinstance(st, dict) else None
        self._hiav = np.ascontiguousarray(highav_coefficients(self.filternames) if hiav is None else hiav, dtype=np.float64)
        self._nets = [np.ascontiguousarray(np.asarray(st[k], dtype=np.float32).reshape(s))
                      for k, s in (("w1", (F, H, 6)), ("b1", (F, H)), ("w2", (F, H, H)), ("b2", (F, H)), ("w3", (F, H)), ("b3", (F,)))]
        self._device, self._h, self.lib = device, None, None

    def _setup(self):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("SEDFit needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        if self._h is None:
            d = self._device
            self.device = d if isinstance(d, torch.device) else torch.device("cuda", torch.cuda.current_device() if d is None else int(d))
            self.lib = _lib.load()
            h = C.c_void_p()
            ptr = [a.ctypes.data_as(C.c_void_p) for a in self._nets + [self.xmin, self.xmax, self._hiav]]
            rc = self.lib.payne_sedfit_create(self.device.index, self.F, self.H, *ptr, C.byref(h))
            if rc != 0:
                raise RuntimeError("payne_sedfit_create failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))
            self._h = h
        return torch

    def close(self):
        if self._h is not None:
            self.lib.payne_sedfit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, torch):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def grad_device(self, pars):
        """pars: contiguous fp64 device tensor [N, P] -> (mags [N, F], dmags [N, F, P]), device tensors."""
        torch = self._setup()
        P = len(self.names)
        if pars.dtype != torch.float64 or pars.dim() != 2 or pars.shape[1] != P or not pars.is_contiguous():
            raise ValueError("pars must be contiguous fp64 [N, %d]" % P)
        N = pars.shape[0]
        mags = torch.empty((N, self.F), dtype=torch.float64, device=self.device)
        dmags = torch.empty((N, self.F, P), dtype=torch.float64, device=self.device)
        rc = self.lib.payne_sedfit_jac(self._h, pars.data_ptr(), N, int(self.photscale), mags.data_ptr(), dmags.data_ptr(), self._stream(torch))
        if rc != 0:
            raise RuntimeError("payne_sedfit_jac failed (%d)" % rc)
        return mags, dmags

    def grad(self, pars):
        """pars [N, 7 | 6] -> (mags [N, F], dmags [N, F, 7 | 6]): the magnitudes and d mag / d parameter.  A device tensor in gives
        device tensors out, anything else numpy arrays."""
        torch = self._setup()
        on_device = isinstance(pars, torch.Tensor)
        p = torch.as_tensor(np.asarray(pars, dtype=np.float64) if not on_device else pars).to(device=self.device, dtype=torch.float64)
        p = p.reshape(-1, len(self.names)).contiguous()
        m, dm = self.grad_device(p)
        return (m, dm) if on_device else (m.cpu().numpy(), dm.cpu().numpy())

    def run(self, obs, w, start, cols, lo, hi, mu=None, sigma=None, opts=None):
        """The launch on contiguous fp64 device tensors: obs, w [N, F], start [N, P], mu, sigma [N, K] or None; cols the free columns
        (ascending), lo, hi host [K] -> dict of device tensors (``fit``'s without ``err``)."""
        torch = self._setup()
        N, K, P, dev = obs.shape[0], len(cols), len(self.names), self.device
        mask = sum(1 << c for c in cols)
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        out = dict(pars=torch.empty((N, P), dtype=torch.float64, device=dev), chisq=torch.empty(N, dtype=torch.float64, device=dev),
                   fisher=torch.empty((N, K, K), dtype=torch.float64, device=dev), status=torch.empty(N, dtype=torch.int32, device=dev),
                   niter=torch.empty(N, dtype=torch.int32, device=dev), at_bound=torch.empty(N, dtype=torch.int32, device=dev),
                   nfilt=torch.empty(N, dtype=torch.int32, device=dev))
        o = _lib.LmfitOpts(**(opts or LM_DEFAULTS))
        rc = self.lib.payne_sedfit_run(self._h, int(self.photscale), mask, start.data_ptr(), obs.data_ptr(), w.data_ptr(), N,
                                       lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                                       None if mu is None else mu.data_ptr(), None if sigma is None else sigma.data_ptr(), C.byref(o),
                                       out["pars"].data_ptr(), out["chisq"].data_ptr(), out["fisher"].data_ptr(), out["status"].data_ptr(),
                                       out["niter"].data_ptr(), out["at_bound"].data_ptr(), out["nfilt"].data_ptr(), self._stream(torch))
        if rc != 0:
            raise RuntimeError("payne_sedfit_run failed (%d)" % rc)
        return out

    def fit(self, mags, emags, start, free=("Teff", "logR", "Av"), bounds=None, prior=None, **opts):
        """mags, emags [N, F] (a NaN magnitude, or an error that is NaN, inf or <= 0: the filter does not count), start [N, 7 | 6].
        ``free``: the fitted parameters; the others stay at ``start``.  ``bounds``: {name: (lo, hi)} or [P, 2] over the defaults (the
        nets' range for the labels and Av, which must stay below 5; wide ranges for logR / Dist / logA).  ``prior`` = (mu, sigma)
        [N, K], Gaussian, columns in the row's order of the free parameters, an infinite sigma meaning none; ``free`` with both logR
        and Dist needs a finite one on either for every star.  ``opts``: payne_lmfit_opts' fields.  Returns a dict: ``pars`` [N, P],
        ``err`` [N, K] (sqrt diag of the inverse Fisher matrix: marginalised; NaN where it has none), ``fisher`` [N, K, K], ``chisq``,
        ``nfilt``, ``status`` (``_lib.LMFIT_*`` and ``_lib.SEDFIT_TOO_FEW``), ``niter``, ``at_bound`` (bit k: free parameter k) and
        ``free`` (the names in the order of every K-sized axis).  Device tensors in give device tensors out."""
        torch = self._setup()
        on_device = any(isinstance(a, torch.Tensor) for a in (mags, emags, start))

        def host(a):
            return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        if on_device:
            # the per-star arrays stay on the device; the checks run on shapes and on the few host-side values
            m = torch.as_tensor(mags).to(device=self.device, dtype=torch.float64).reshape(-1, self.F)
            e = torch.as_tensor(emags).to(device=self.device, dtype=torch.float64).reshape(-1, self.F)
            s = torch.as_tensor(start).to(device=self.device, dtype=torch.float64).reshape(-1, len(self.names)).contiguous()
            N = m.shape[0]
            pr = None if prior is None else tuple(host(a) for a in prior)
            c = check_fit_args(None, None, None, self.F, self.xmin, self.xmax, self.photscale, free, bounds, pr, N=N, **opts)
            if tuple(e.shape) != tuple(m.shape) or s.shape[0] != N:
                raise ValueError("mags, emags [N, F] and start [N, P] disagree")
            ok = torch.isfinite(m) & torch.isfinite(e) & (e > 0.0)
            w = torch.where(ok, 1.0 / torch.where(ok, e, torch.ones_like(e)) ** 2, torch.zeros_like(e)).contiguous()
            obs = torch.where(ok, m, torch.zeros_like(m)).contiguous()
        else:
            c = check_fit_args(mags, emags, start, self.F, self.xmin, self.xmax, self.photscale, free, bounds, prior, **opts)
            obs, w, s = (torch.as_tensor(c[k]).to(self.device) for k in ("obs", "w", "start"))
        mu = sigma = None
        if c["mu"] is not None:
            mu, sigma = torch.as_tensor(c["mu"]).to(self.device).contiguous(), torch.as_tensor(c["sigma"]).to(self.device).contiguous()
        out = self.run(obs, w, s, c["cols"], c["lo"], c["hi"], mu, sigma, c["opts"])
        out["err"] = marginal_errors(torch, out["fisher"], out["status"])
        res = out if on_device else {k: v.cpu().numpy() for k, v in out.items()}
        res["free"] = tuple(self.names[k] for k in c["cols"])
        return res


def marginal_errors(torch, fisher, status):
    """sqrt diag(A^-1) [N, K] through the unit-diagonal scaling S A S; NaN where the star has no solution or A no inverse."""
    d = torch.diagonal(fisher, dim1=1, dim2=2)
    good = (d > 0.0).all(dim=1) & torch.isfinite(fisher).all(dim=2).all(dim=1)
    good &= (status == _lib.LMFIT_CONVERGED) | (status == _lib.LMFIT_STALLED) | (status == _lib.LMFIT_MAXITER)
    s = torch.rsqrt(torch.where(good[:, None], d, torch.ones_like(d)))
    M = torch.where(good[:, None, None], fisher * s[:, :, None] * s[:, None, :], torch.eye(fisher.shape[1], dtype=fisher.dtype, device=fisher.device))
    L, info = torch.linalg.cholesky_ex(M)
    good &= info == 0
    inv = torch.cholesky_inverse(torch.where(good[:, None, None], L, torch.eye(fisher.shape[1], dtype=fisher.dtype, device=fisher.device).expand_as(L)))
    err = torch.sqrt(torch.diagonal(inv, dim1=1, dim2=2)) * s
    return torch.where(good[:, None], err, torch.full_like(err, float("nan")))
