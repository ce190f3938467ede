"""Continuum (blaze) polynomials for many spectra on one wavelength grid, against a given model spectrum each, on the GPU.

``ContinuumFit.fit`` finds, per star, the Chebyshev coefficients c that minimise chi^2 = sum_p w_p (flux_p - model_p p(x_p))^2,
p = sum_j c_j T_j: the likelihood's own objective in its ``pc_*`` parameters (``modpoly``: model x ``polycalc``) for a fixed model,
which is a linear least-squares problem.  One launch solves it for every star (payne_contfit_batch; include/payne_hip.h states the
rules), optionally with kappa-sigma clipping of cosmic rays and of lines the model lacks, and returns the spectra divided by their
polynomial with the weights carried along: sum w (f - m p)^2 = sum (w p^2) (f / p - m)^2, so a fit of the normalised flux with the
scaled errors (``OptFit.fit``, ``TemplateBank.match``) minimises the same chi^2.  The coefficients are in ``polycalc``'s basis and
abscissa and can centre ``priordict['blaze_coeff']``.

This is not ``PCcalc``: that fits a polynomial to flux / model with weights 1 / eflux^2 (the model is 1.0 outside its range), one
star at a time by Nelder-Mead on the host.  Here the residual is flux - model x polynomial with the flux's own errors, as in the
likelihood, solved in closed form.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .forecast import weights_from_errors

__all__ = ["ContinuumFit", "check_setup", "check_contfit_args", "abscissa"]


def abscissa(obs_wave):
    """``polycalc``'s x in [-1, 1] (fitutils.polycalc: the same expression, so the same bits)."""
    wave = np.asarray(obs_wave, dtype=np.float64)
    span = wave - wave.min()
    return 2.0 * (span / span.max()) - 1.0


def check_setup(obs_wave, npoly=4, nclip=0, kappa=(3.0, 3.0), rescale=False, drop_clipped=True):
    """What ``ContinuumFit`` checks of its own arguments; no GPU.  Returns (obs_wave fp64 [nobs], x fp64 [nobs], opts dict for
    ``_lib.ContfitOpts``)."""
    wave = np.ascontiguousarray(obs_wave, dtype=np.float64)
    if wave.ndim != 1 or len(wave) < 2:
        raise ValueError("obs_wave must be a vector of at least 2 points")
    if not np.all(np.isfinite(wave)) or not np.all(np.diff(wave) > 0.0):
        raise ValueError("obs_wave must be finite and increasing")
    if len(wave) > _lib.CONTFIT_MAX_N:
        raise ValueError("obs_wave holds %d points; at most %d" % (len(wave), _lib.CONTFIT_MAX_N))
    if int(npoly) != npoly or not (1 <= int(npoly) <= _lib.CONTFIT_MAX_P):
        raise ValueError("npoly must be 1 .. %d, got %r" % (_lib.CONTFIT_MAX_P, npoly))
    if int(nclip) != nclip or not (0 <= int(nclip) <= _lib.CONTFIT_MAX_NCLIP):
        raise ValueError("nclip must be 0 .. %d, got %r" % (_lib.CONTFIT_MAX_NCLIP, nclip))
    k = np.atleast_1d(np.asarray(kappa, dtype=np.float64))
    if k.shape == (1,):
        k = np.repeat(k, 2)
    if k.shape != (2,) or not np.all(k > 0.0):
        raise ValueError("kappa must be a positive number or (kappa_lo, kappa_hi), both positive")
    return wave, abscissa(wave), dict(P=int(npoly), nclip=int(nclip), rescale=bool(rescale), drop_clipped=bool(drop_clipped),
                                      kappa_lo=float(k[0]), kappa_hi=float(k[1]))


def check_contfit_args(flux, eflux, model, index, nobs):
    """What ``ContinuumFit.fit`` checks of host arrays before anything reaches the device: (flux fp32 [N, nobs], w fp64 [N, nobs],
    model fp32 [M, nobs], index int32 [N] or None).  w = 1 / eflux^2, 0 where eflux is zero or not finite (``weights_from_errors``).
    An index outside [0, M) is not an error: that star gets the status BAD_MODEL."""
    flux = np.atleast_2d(np.asarray(flux, dtype=np.float32))
    eflux = np.atleast_2d(np.asarray(eflux, dtype=np.float64))
    model = np.atleast_2d(np.asarray(model, dtype=np.float32))
    if flux.ndim != 2 or flux.shape[1] != nobs:
        raise ValueError("flux must be [N, %d], got %s" % (nobs, flux.shape))
    if eflux.shape != flux.shape:
        raise ValueError("eflux %s and flux %s differ in shape" % (eflux.shape, flux.shape))
    if model.ndim != 2 or model.shape[1] != nobs or model.shape[0] < 1:
        raise ValueError("model must be [M, %d], got %s" % (nobs, model.shape))
    index = check_index(index, flux.shape[0], model.shape[0])
    return np.ascontiguousarray(flux), weights_from_errors(eflux), np.ascontiguousarray(model), index


def check_index(index, N, M):
    """index [N] as int32, or None where the model has a row per star."""
    if index is None:
        if M != N:
            raise ValueError("model has %d rows for %d stars: pass index [N]" % (M, N))
        return None
    idx = np.asarray(index)
    if idx.shape != (N,) or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("index must be %d integers, got %s %s" % (N, idx.dtype, idx.shape))
    return np.ascontiguousarray(np.clip(idx, -1, M), dtype=np.int32)


class ContinuumFit(object):
    """ContinuumFit(obs_wave, npoly=4): polynomials of ``npoly`` Chebyshev coefficients on the observed grid ``obs_wave``.
    ``nclip``: at most that many re-fits after clipping pixels whose residual in sigma lies outside [-kappa_lo, kappa_hi] (times the
    reduced chi's root with ``rescale``); ``drop_clipped``: the returned errors are 0 (the pixel does not count) for clipped pixels."""

    def __init__(self, obs_wave, npoly=4, nclip=0, kappa=(3.0, 3.0), rescale=False, drop_clipped=True, device=None):
        self.obs_wave, self.x, self.opts = check_setup(obs_wave, npoly=npoly, nclip=nclip, kappa=kappa, rescale=rescale, drop_clipped=drop_clipped)
        self.npoly = self.opts["P"]
        self._device, self._x_dev = device, None

    def _setup(self):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("ContinuumFit needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        if self._x_dev is None:
            d = self._device
            self.device = d if isinstance(d, torch.device) else torch.device("cuda", torch.cuda.current_device() if d is None else int(d))
            self.lib = _lib.load()
            self._x_dev = torch.as_tensor(self.x).to(self.device)
        return torch

    def run(self, flux, w, model, index=None, normalise=True):
        """The launch on device tensors: flux fp32 [N, nobs], w fp64 [N, nobs], model fp32 [M, nobs], all contiguous; index int32 [N]
        or None -> dict of device tensors (``fit``'s, with ``weights`` but without ``eflux``)."""
        torch = self._setup()
        N, n, P = flux.shape[0], len(self.obs_wave), self.npoly
        if flux.dtype != torch.float32 or model.dtype != torch.float32 or w.dtype != torch.float64 or not (flux.is_contiguous() and w.is_contiguous() and model.is_contiguous()):
            raise ValueError("flux and model contiguous fp32, w contiguous fp64")
        if tuple(flux.shape) != (N, n) or tuple(w.shape) != (N, n) or model.dim() != 2 or model.shape[1] != n:
            raise ValueError("flux and w [N, %d], model [M, %d]; got %s, %s, %s" % (n, n, tuple(flux.shape), tuple(w.shape), tuple(model.shape)))
        if index is not None and (index.dtype != torch.int32 or tuple(index.shape) != (N,) or not index.is_contiguous()):
            raise ValueError("index must be contiguous int32 [N]")
        if index is None and model.shape[0] < N:
            raise ValueError("model has %d rows for %d stars: pass index [N]" % (model.shape[0], N))
        dev = self.device
        out = dict(coef=torch.empty((N, P), dtype=torch.float64, device=dev), chisq=torch.empty(N, dtype=torch.float64, device=dev),
                   npix=torch.empty(N, dtype=torch.int32, device=dev), status=torch.empty(N, dtype=torch.int32, device=dev),
                   rounds=torch.empty(N, dtype=torch.int32, device=dev))
        if normalise:
            out["flux"] = torch.empty((N, n), dtype=torch.float32, device=dev)
            out["weights"] = torch.empty((N, n), dtype=torch.float64, device=dev)
        opts = _lib.ContfitOpts(**self.opts)
        rc = self.lib.payne_contfit_batch(dev.index, flux.data_ptr(), w.data_ptr(), n, model.data_ptr(), n, model.shape[0],
                                          index.data_ptr() if index is not None else None, self._x_dev.data_ptr(), N, n, C.byref(opts),
                                          out["coef"].data_ptr(), out["chisq"].data_ptr(), out["npix"].data_ptr(), out["status"].data_ptr(),
                                          out["rounds"].data_ptr(), out["flux"].data_ptr() if normalise else None,
                                          out["weights"].data_ptr() if normalise else None, n,
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError("payne_contfit_batch failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))
        return out

    def fit(self, flux, eflux, model, index=None, normalise=True):
        """flux, eflux [N, nobs] on ``obs_wave`` (eflux zero or not finite: the pixel does not count); model [N, nobs], or [M, nobs]
        with index [N] (star s is fitted against row index[s]; outside [0, M): status BAD_MODEL).  Host arrays or device tensors: a
        device tensor among flux, eflux and model gives device tensors out, anything else numpy arrays.  Returns a dict: ``coef``
        [N, npoly] (``polycalc``'s), ``chisq`` (over the kept pixels), ``npix`` (kept pixels), ``status`` (``_lib.CONTFIT_*``),
        ``rounds`` (solves) and, with ``normalise``, ``flux`` = flux / polynomial (fp32), ``weights`` = w x polynomial^2 and
        ``eflux`` = 1 / sqrt(weights), 0 where the weight is 0 (the pixel does not count: it did not before, it was clipped, or the
        polynomial is not positive there).  A status other than OK / NONPOSITIVE: NaN coefficients, the flux unchanged, eflux 0."""
        torch = self._setup()
        nobs, dev = len(self.obs_wave), self.device
        on_device = any(isinstance(a, torch.Tensor) for a in (flux, eflux, model))
        if on_device:
            f = torch.as_tensor(flux).to(device=dev, dtype=torch.float32).reshape(-1, nobs).contiguous()
            e = torch.as_tensor(eflux).to(device=dev, dtype=torch.float64).reshape(-1, nobs)
            m = torch.as_tensor(model).to(device=dev, dtype=torch.float32).reshape(-1, nobs).contiguous()
            if tuple(e.shape) != tuple(f.shape):
                raise ValueError("eflux %s and flux %s differ in shape" % (tuple(e.shape), tuple(f.shape)))
            ok = torch.isfinite(e) & (e != 0.0)
            w = torch.where(ok, 1.0 / (e * e), torch.zeros_like(e)).contiguous()
            idx = index.cpu().numpy() if isinstance(index, torch.Tensor) else index
            idx = check_index(idx, f.shape[0], m.shape[0])
        else:
            fh, wh, mh, idx = check_contfit_args(flux, eflux, model, index, nobs)
            f, w, m = torch.as_tensor(fh).to(dev), torch.as_tensor(wh).to(dev), torch.as_tensor(mh).to(dev)
        idx_d = None if idx is None else torch.as_tensor(idx).to(dev)
        out = self.run(f, w, m, idx_d, normalise=normalise)
        if normalise:
            wo = out["weights"]
            out["eflux"] = torch.where(wo > 0.0, torch.rsqrt(torch.where(wo > 0.0, wo, torch.ones_like(wo))), torch.zeros_like(wo))
        return out if on_device else {k: v.cpu().numpy() for k, v in out.items()}

    def fit_to_bank(self, flux, eflux, bank, match=None, rank=0):
        """``fit`` against the template of rank ``rank`` that ``bank`` (a ``tmatch.TemplateBank`` on this ``obs_wave``) matched to each
        star: the bank's templates are read in place through the index, nothing is gathered.  ``match``: ``bank.match``'s dict (run
        here with topk = rank + 1 when None).  A star without such a template (index -1) gets the status BAD_MODEL.  For spectra
        that are not on the model's continuum hand in ``bank.match(flux, eflux, npoly=P)``'s dict: its ranking has the polynomial
        minimised out, and only its ``index`` is read here."""
        if not hasattr(bank, "match") or not hasattr(bank, "obs_wave"):
            raise TypeError("bank must be a TemplateBank")
        if np.shape(bank.obs_wave) != self.obs_wave.shape or not np.array_equal(np.asarray(bank.obs_wave), self.obs_wave):
            raise ValueError("the bank's obs_wave differs from the fitter's")
        if bank.templates is None:
            raise RuntimeError("the bank is empty: call build(theta) or lattice(steps, ...) first")
        if match is None:
            match = bank.match(flux, eflux, topk=int(rank) + 1)
        index = np.asarray(match["index"])
        if index.ndim != 2 or not (0 <= int(rank) < index.shape[1]):
            raise ValueError("match['index'] must be [N, topk] with topk > rank")
        torch = self._setup()
        out = self.fit(flux, eflux, bank.templates, index=np.ascontiguousarray(index[:, int(rank)], dtype=np.int32))
        on_device = isinstance(flux, torch.Tensor) or isinstance(eflux, torch.Tensor)
        return out if on_device else {k: v.cpu().numpy() for k, v in out.items()}
