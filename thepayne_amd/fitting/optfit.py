"""Least-squares point estimates of the stellar labels for many spectra on one wavelength grid: batched Levenberg-Marquardt on
the GPU.

``OptFit.fit`` minimises, per star, chi^2 = sum_p w_p (flux_p - model_p(x))^2 over the labels of the spectral network (and, with
``fit_vrad``, the radial velocity) inside a box, at the star's own fixed Vrot, Inst_R (and Vrad).  One iteration is three enqueued
steps and nothing in between: the network and its Jacobian at every star's trial point (payne_specjac_eval), the engine's
broadening and resampling applied to those rows (payne_smooth_batch), and one launch that forms every star's normal equations on
the fp64 matrix instruction and takes its damped step (payne_lmfit_update: include/payne_hip.h states the rules).  The host looks
at the stars' status only every ``check_every`` iterations.

The model whose chi^2 is minimised is payne_specjac_eval's y pushed through payne_smooth_batch, so that the model and its
Jacobian come from the same arithmetic.  This is NOT the likelihood's forward pass (whose dense layers split their operands in
fp16 parts): the two agree within the bound tests/test_specjac_gpu.py holds them to, and a fit's chi^2 is not lnlike's to the bit.

What is fitted: Teff, log(g), [Fe/H], [alpha/Fe] and, for a five-label network, Vmic; Vrad with ``fit_vrad`` (its derivative is a
central difference of the broadened model at Vrad +- ``vrad_step``).  Vrot and Inst_R are fixed at the values ``start`` gives, and
Vmic too for a four-label network.  ``fisher`` is the normal matrix J^T W J at the solution and ``err`` its Cramer-Rao bounds
(``forecast.crlb_from_fisher``): conditional on the fixed parameters, as ``Forecast``'s are.  A continuum network and an LSF vector
are not supported (``PayneSpecPredict.getgrad`` explains why).

``OptFit.fit_joint`` fits a continuum polynomial (``polycalc``'s Chebyshev coefficients) along with these parameters, in the same
loop: its update, payne_lmfit_update_poly, forms the rows of model x polynomial in registers.

``OptFit.fit_specphot`` fits spectrum and photometry together: one chi^2 over the labels both share, Vmic / Vrad / the polynomial,
which only the spectrum sees, and log R, distance, Av (or log A, Av), which only the magnitudes see, Gaussian priors on any of them
included.  An iteration has a fourth enqueued step, ``SEDFit.grad_device`` at the trial point, and its update,
payne_lmfit_update_phot, adds the magnitudes' normal equations and the priors to the spectral tile before the step is taken.  The
errors that come back are marginal over all fitted parameters.  The spectral model is fp32: where the magnitudes pull the shared labels
off the spectrum's own minimum, its rounding reaches chi^2 at a few 1e-6, which is more than a step of xtol = 1e-3 sigma gains, and a
star may end ``STALLED`` (or ``CONVERGED`` after a dozen rejected trials) AT the solution; ``fit_specphot``'s docstring says what to
make of that.

``OptFit.fit_binary`` fits a double-lined binary: two components, each with its own labels and Vrad (some labels tied), a light ratio
q and the polynomial in one fit of chi^2 = sum w (flux - p [(1 - q) m_A + q m_B])^2.  Its update, payne_lmfit_update_pair, reads both
components' rows and mixes them in registers (csrc/lmfit_pair_core.hpp).
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..engine import THETA_SPEC_COLS
from ..predict._spec import PayneSpecPredict, smooth_rows
from .forecast import crlb_from_fisher, weights_from_errors

__all__ = ["OptFit", "check_fit_args", "check_joint_args", "check_specphot_args", "check_binary_args", "LM_DEFAULTS", "VRAD_BOUND", "COEF_BOUND"]

LM_DEFAULTS = dict(lambda0=1e-3, down=10.0, up=10.0, lambda_min=1e-12, lambda_max=1e8, xtol=1e-3, maxiter=50)
VRAD_BOUND = 500.0                                   # km/s: the default box of a fitted Vrad


def fitted_columns(n_labels, fit_vrad):
    """The columns of getspec's eight that are fitted: the network's labels, then Vrad."""
    return [0, 1, 2, 3] + ([6] if n_labels == 5 else []) + ([4] if fit_vrad else [])


def _npoly_int(npoly, least):
    """``npoly`` as an int: an integer (no bool) of at least ``least``."""
    if isinstance(npoly, bool) or int(npoly) != npoly or int(npoly) < least:
        raise ValueError("npoly must be an integer >= %d, got %r" % (least, npoly))
    return int(npoly)


def _coef_array(coef, N, P):
    """Starting coefficients as fp64 [N, P], finite."""
    coef = np.atleast_2d(np.asarray(coef.cpu() if hasattr(coef, "cpu") else coef, dtype=np.float64))     # (ContinuumFit's may be a device tensor)
    if coef.shape != (N, P):
        raise ValueError("coef must be [%d, %d], got %s" % (N, P, coef.shape))
    if not np.all(np.isfinite(coef)):
        raise ValueError("coef is not finite")
    return coef


def _named_bounds(bounds, names, lo, hi, what, elsewhere=None):
    """``bounds`` = {name: (lo, hi)} written into the box lo, hi [K] of the parameters ``names``.  ``elsewhere``: (a name whose box is
    not set here, where it is set)."""
    if not isinstance(bounds, dict):
        raise ValueError("bounds must be a dict {name: (lo, hi)} over %s" % (names,))
    for name, (a, b) in bounds.items():
        if name not in names or (elsewhere is not None and name == elsewhere[0]):
            have = ", ".join(n for n in names if elsewhere is None or n != elsewhere[0])
            raise ValueError("bounds: %r is not a fitted %s (%s)%s" % (name, what, have, "" if elsewhere is None else " (%s's box is %s)" % elsewhere))
        lo[names.index(name)], hi[names.index(name)] = float(a), float(b)


def _check_box(lo, hi, what, each):
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
        raise ValueError("%s: lo < hi, both finite, for every %s" % (what, each))


def check_fit_args(flux, eflux, start, nobs, n_labels, xmin, xmax, fit_vrad=False, bounds=None, vrad_step=0.25, check_every=4, **opts):
    """What ``OptFit.fit`` checks before anything reaches the device.  Returns (flux [N, nobs] fp32, eflux [N, nobs] fp64, start
    [N, 8] fp64, lo [K], hi [K], opts dict).  ``bounds``: {column name of THETA_SPEC_COLS: (lo, hi)} for some of the fitted columns,
    or an array [K, 2] for all of them."""
    flux = np.atleast_2d(np.asarray(flux, dtype=np.float32))
    eflux = np.atleast_2d(np.asarray(eflux, dtype=np.float64))
    start = np.atleast_2d(np.asarray(start, dtype=np.float64))
    if flux.ndim != 2 or flux.shape[1] != nobs:
        raise ValueError("flux must be [N, %d], got %s" % (nobs, flux.shape))
    if eflux.shape != flux.shape:
        raise ValueError("eflux %s and flux %s differ in shape" % (eflux.shape, flux.shape))
    if start.ndim != 2 or start.shape != (flux.shape[0], 8):
        raise ValueError("start must be [%d, 8] (getspec's columns), got %s" % (flux.shape[0], start.shape))
    cols = fitted_columns(n_labels, fit_vrad)
    K = len(cols)
    if not np.all(np.isfinite(start[:, cols])):
        raise ValueError("start is not finite in a fitted column")
    if not np.all(np.isfinite(start[:, 5])):
        raise ValueError("start's Vrot is not finite")
    if not fit_vrad and not np.all(np.isfinite(start[:, 4])):
        raise ValueError("start's Vrad is not finite")
    lo = np.concatenate([np.asarray(xmin, dtype=np.float64)[:n_labels], [-VRAD_BOUND] if fit_vrad else []])
    hi = np.concatenate([np.asarray(xmax, dtype=np.float64)[:n_labels], [VRAD_BOUND] if fit_vrad else []])
    if bounds is not None:
        if isinstance(bounds, dict):
            _named_bounds(bounds, [THETA_SPEC_COLS[c] for c in cols], lo, hi, "column")
        else:
            bd = np.asarray(bounds, dtype=np.float64)
            if bd.shape != (K, 2):
                raise ValueError("bounds must be [%d, 2] or a dict, got %s" % (K, bd.shape))
            lo, hi = bd[:, 0].copy(), bd[:, 1].copy()
    _check_box(lo, hi, "bounds", "fitted column")
    if not (np.isfinite(vrad_step) and vrad_step > 0.0):
        raise ValueError("vrad_step must be positive")
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    unknown = sorted(set(opts) - set(LM_DEFAULTS))
    if unknown:
        raise TypeError("unknown options %s (have %s)" % (unknown, sorted(LM_DEFAULTS)))
    o = dict(LM_DEFAULTS, **opts)
    fin = all(np.isfinite(float(o[k])) for k in LM_DEFAULTS)
    if not fin or o["lambda_min"] < 0 or o["lambda_max"] < o["lambda_min"] or not (o["lambda_min"] <= o["lambda0"] <= o["lambda_max"]) \
            or o["down"] < 1 or o["up"] < 1 or o["xtol"] < 0 or int(o["maxiter"]) < 1:
        raise ValueError("options out of range: %s" % (o,))
    return flux, eflux, start, lo, hi, o


COEF_BOUND = 1e30                                    # the default box of a fitted Chebyshev coefficient: finite, as payne_lmfit_begin requires


def check_joint_args(flux, eflux, start, nobs, n_labels, xmin, xmax, npoly=4, coef=None, clip=None, coef_bounds=None, **fit_args):
    """What ``OptFit.fit_joint`` checks before anything reaches the device: ``check_fit_args`` on ``fit``'s arguments, then the
    polynomial's.  Returns (flux, eflux, start, lo [K], hi [K], opts dict, coef fp64 [N, npoly] or None, clip dict) with
    K = K_m + npoly, the coefficients' box behind the fitted columns'."""
    flux, eflux, start, lo, hi, o = check_fit_args(flux, eflux, start, nobs, n_labels, xmin, xmax, **fit_args)
    P, Km = _npoly_int(npoly, 1), len(lo)
    if Km + P > _lib.LMFIT_MAX_K:
        raise ValueError("%d fitted columns and npoly = %d are %d parameters; at most %d (one 16 x 16 tile holds a star's normal equations)"
                         % (Km, P, Km + P, _lib.LMFIT_MAX_K))
    if coef is not None:
        coef = _coef_array(coef, flux.shape[0], P)
    clip = dict(clip or {})
    unknown = sorted(set(clip) - {"nclip", "kappa", "rescale"})
    if unknown:
        raise ValueError("clip: unknown keys %s (have nclip, kappa, rescale)" % unknown)
    if coef is not None and clip:
        raise ValueError("clip belongs to the starting continuum fit, which coef replaces")
    if coef_bounds is None:
        cb = np.tile([-COEF_BOUND, COEF_BOUND], (P, 1))
    else:
        cb = np.asarray(coef_bounds, dtype=np.float64)
        if cb.shape != (P, 2):
            raise ValueError("coef_bounds must be [%d, 2], got %s" % (P, cb.shape))
        _check_box(cb[:, 0], cb[:, 1], "coef_bounds", "coefficient")
    return flux, eflux, start, np.concatenate([lo, cb[:, 0]]), np.concatenate([hi, cb[:, 1]]), o, coef, clip


def check_specphot_args(flux, eflux, mags, emags, start, phot_start, nobs, n_labels, xmin, xmax, F, sed_xmin, sed_xmax, photscale=False,
                        free_phot=("logR", "Av"), npoly=0, coef=None, clip=None, fit_vrad=False, bounds=None, coef_bounds=None, prior=None,
                        vrad_step=0.25, check_every=4, **opts):
    """What ``OptFit.fit_specphot`` checks before anything reaches the device; no GPU.  ``F``, ``sed_xmin``, ``sed_xmax``,
    ``photscale``: the ``SEDFit``'s.  The K = K_m + K_p + npoly parameters are the fitted columns of ``start`` (the labels, Vrad), the
    free photometric-only parameters in the row's order, the coefficients.  Returns a dict: flux, eflux, start, coef, clip, opts as
    ``check_joint_args`` returns them; obs, pw [N, F]; phot_start [N, ncol - 4]; names [K]; lo, hi [K]; Km, Kp, P; phot_cols (the K_p
    columns of the photometric row); sed_col [K] (the column of the row that parameter k is, -1: none); mu, sigma [N, K] or None."""
    from . import sedfit
    pnames = sedfit.par_names(photscale)
    ncol = len(pnames)
    free = [free_phot] if isinstance(free_phot, str) else list(free_phot)
    if len(set(free)) != len(free) or any(f not in pnames[4:] for f in free):
        raise ValueError("free_phot must name parameters among %s, each once; got %r" % (pnames[4:], free))
    P = _npoly_int(npoly, 0)
    cols = fitted_columns(n_labels, fit_vrad)
    Km, Kp = len(cols), len(free)
    K = Km + Kp + P
    if K > _lib.LMFIT_MAX_K:
        raise ValueError("%d fitted columns of the spectrum, %d photometric parameters and npoly = %d are %d parameters; at most %d (one 16 x 16 "
                         "tile holds a star's normal equations)" % (Km, Kp, P, K, _lib.LMFIT_MAX_K))
    if int(F) > _lib.LMFIT_PHOT_MAX_F:
        raise ValueError("%d filters; payne_lmfit_update_phot takes at most %d" % (F, _lib.LMFIT_PHOT_MAX_F))
    fit_args = dict(fit_vrad=fit_vrad, vrad_step=vrad_step, check_every=check_every, **opts)
    if P:
        flux, eflux, start, lo_s, hi_s, o, coef, clip = check_joint_args(flux, eflux, start, nobs, n_labels, xmin, xmax, npoly=P, coef=coef, clip=clip,
                                                                         coef_bounds=coef_bounds, **fit_args)
    else:
        if coef is not None or clip or coef_bounds is not None:
            raise ValueError("coef, clip and coef_bounds belong to the polynomial; npoly is 0")
        flux, eflux, start, lo_s, hi_s, o = check_fit_args(flux, eflux, start, nobs, n_labels, xmin, xmax, **fit_args)
        coef, clip = None, {}
    N = flux.shape[0]
    mags, emags = np.atleast_2d(np.asarray(mags, dtype=np.float64)), np.atleast_2d(np.asarray(emags, dtype=np.float64))
    if mags.shape != (N, int(F)) or emags.shape != mags.shape:
        raise ValueError("mags and emags must be [%d, %d], got %s and %s" % (N, F, mags.shape, emags.shape))
    phot_start = np.atleast_2d(np.asarray(phot_start, dtype=np.float64))
    if phot_start.shape != (N, ncol - 4) or not np.all(np.isfinite(phot_start)):
        raise ValueError("phot_start must be [%d, %d] (%s) and finite, got %s" % (N, ncol - 4, ", ".join(pnames[4:]), phot_start.shape))
    ok = np.isfinite(mags) & np.isfinite(emags) & (emags > 0.0)
    obs, pw = np.where(ok, mags, 0.0), np.where(ok, 1.0 / np.where(ok, emags, 1.0) ** 2, 0.0)
    # the box: a shared label's is the intersection of the two networks', a photometric parameter's is SEDFit's
    plo, phi = sedfit.default_box(np.asarray(sed_xmin, dtype=np.float64), np.asarray(sed_xmax, dtype=np.float64), photscale)
    phot_cols = sorted(pnames.index(f) for f in free)
    names = [THETA_SPEC_COLS[c] for c in cols] + [pnames[c] for c in phot_cols] + ["pc_%d" % j for j in range(P)]
    lo, hi = np.concatenate([lo_s[:Km], plo[phot_cols], lo_s[Km:]]), np.concatenate([hi_s[:Km], phi[phot_cols], hi_s[Km:]])
    lo[:4], hi[:4] = np.maximum(lo[:4], plo[:4]), np.minimum(hi[:4], phi[:4])
    if not np.all(lo[:4] < hi[:4]):
        raise ValueError("the spectral and the photometric networks' ranges of %s do not overlap" % names[int(np.flatnonzero(~(lo[:4] < hi[:4]))[0])])
    if bounds is not None:
        _named_bounds(bounds, names, lo, hi, "parameter")
    _check_box(lo, hi, "bounds", "fitted parameter")
    if "Av" in free and not hi[names.index("Av")] < sedfit.AV_MAX:
        raise ValueError("the upper Av bound must be below %g: the model jumps there" % sedfit.AV_MAX)
    sed_col = np.full(K, -1, dtype=np.int32)
    sed_col[:4] = np.arange(4)
    sed_col[Km:Km + Kp] = phot_cols
    mu = sigma = None
    if prior:
        mu, sigma = np.zeros((N, K)), np.full((N, K), np.inf)
        for name, ms in prior.items():
            if name not in names:
                raise ValueError("prior: %r is not a fitted parameter (%s)" % (name, ", ".join(names)))
            m, s = (np.broadcast_to(np.asarray(a, dtype=np.float64), (N,)) for a in ms)
            if np.any(np.isnan(s)) or np.any(s <= 0.0) or np.any(~np.isfinite(m) & np.isfinite(s)):
                raise ValueError("prior on %s: sigmas must be positive (inf: no prior) and their centres finite" % name)
            mu[:, names.index(name)], sigma[:, names.index(name)] = np.where(np.isfinite(s), m, 0.0), s
    if "logR" in free and "Dist" in free:
        if sigma is None or not np.all(np.isfinite(sigma[:, names.index("logR")]) | np.isfinite(sigma[:, names.index("Dist")])):
            raise ValueError("logR and Dist are exactly degenerate in the magnitudes and the spectrum sees neither: every star needs a finite prior "
                             "sigma on one of them")
    return dict(flux=flux, eflux=eflux, start=start, coef=coef, clip=clip, opts=o, obs=obs, pw=pw, phot_start=np.ascontiguousarray(phot_start), names=names,
                lo=lo, hi=hi, Km=Km, Kp=Kp, P=P, cols=cols, phot_cols=phot_cols, sed_col=sed_col, mu=mu, sigma=sigma)


TIE_ALIASES = {"teff": "Teff", "logg": "log(g)", "feh": "[Fe/H]", "afe": "[a/Fe]", "vmic": "Vmic"}


def check_binary_args(flux, eflux, start_a, start_b, nobs, n_labels, xmin, xmax, ratio=0.3, tie=(), fit_vrad=True, npoly=0, coef=None, bounds=None,
                      ratio_bounds=(0.01, 0.99), vrad_step=0.25, check_every=4, **opts):
    """What ``OptFit.fit_binary`` checks before anything reaches the device; no GPU.  The K = K_l + 1 + npoly parameters are A's fitted
    columns (the labels, then Vrad), B's that are not tied, the ratio, the coefficients.  ``tie``: names of network labels
    (``THETA_SPEC_COLS``'s, or teff / logg / feh / afe / vmic) that both components share.  ``bounds``: {name of ``labels``: (lo, hi)}.
    Returns a dict: flux, eflux, start_a, start_b, ratio [N], coef (or None), opts; cols (a component's fitted columns of getspec's
    eight); Ka; Kl; P; ia, ib int32 [Kl]; b_pos [Ka] (where B's fitted column k sits among the parameters); names, lo, hi [K]."""
    flux, eflux, start_a, lo_c, hi_c, o = check_fit_args(flux, eflux, start_a, nobs, n_labels, xmin, xmax, fit_vrad=fit_vrad, vrad_step=vrad_step,
                                                         check_every=check_every, **opts)
    start_b = check_fit_args(flux, eflux, start_b, nobs, n_labels, xmin, xmax, fit_vrad=fit_vrad)[2]
    N = flux.shape[0]
    cols = fitted_columns(n_labels, fit_vrad)
    cnames = [THETA_SPEC_COLS[c] for c in cols]
    Ka, D = len(cols), n_labels
    tie = [tie] if isinstance(tie, str) else list(tie)
    tied = []
    for t in tie:
        name = TIE_ALIASES.get(t, t)
        if name not in cnames[:D]:
            raise ValueError("tie: %r is not a label of the network (%s)" % (t, ", ".join(cnames[:D])))
        tied.append(cnames.index(name))
    if len(set(tied)) != len(tied):
        raise ValueError("tie names a label twice: %r" % (tie,))
    P = _npoly_int(npoly, 0)
    free_b = [k for k in range(Ka) if k not in tied]
    Kl = Ka + len(free_b)
    K = Kl + 1 + P
    if K > _lib.LMFIT_MAX_K:
        raise ValueError("%d parameters of the two components, the ratio and npoly = %d are %d parameters; at most %d (one 16 x 16 tile holds a "
                         "star's normal equations): tie labels or lower npoly" % (Kl, P, K, _lib.LMFIT_MAX_K))
    rb = np.asarray(ratio_bounds, dtype=np.float64)
    if rb.shape != (2,) or not (0.0 < rb[0] < rb[1] < 1.0):
        raise ValueError("ratio_bounds must be (lo, hi) with 0 < lo < hi < 1 (at q = 0 or 1 one component's rows vanish), got %r" % (ratio_bounds,))
    ratio = np.array(np.broadcast_to(np.asarray(ratio, dtype=np.float64), (N,)))   # (a copy: broadcast_to's view is read-only)
    if not np.all((ratio >= rb[0]) & (ratio <= rb[1])):
        raise ValueError("ratio must lie inside ratio_bounds = (%g, %g)" % (rb[0], rb[1]))
    if coef is not None:
        if P == 0:
            raise ValueError("coef belongs to the polynomial; npoly is 0")
        coef = _coef_array(coef, N, P)
    ia = np.array(list(range(Ka)) + [-1] * len(free_b), dtype=np.int32)
    ib = np.array([k if k in tied else -1 for k in range(Ka)] + free_b, dtype=np.int32)
    b_pos = np.array([k if k in tied else Ka + free_b.index(k) for k in range(Ka)], dtype=np.int64)
    names = [c + "_a" for c in cnames] + [cnames[k] + "_b" for k in free_b] + ["ratio"] + ["pc_%d" % j for j in range(P)]
    lo = np.concatenate([lo_c, lo_c[free_b], [rb[0]], np.full(P, -COEF_BOUND)])
    hi = np.concatenate([hi_c, hi_c[free_b], [rb[1]], np.full(P, COEF_BOUND)])
    if bounds is not None:
        _named_bounds(bounds, names, lo, hi, "parameter", elsewhere=("ratio", "ratio_bounds"))
    _check_box(lo, hi, "bounds", "fitted parameter")
    return dict(flux=flux, eflux=eflux, start_a=start_a, start_b=start_b, ratio=ratio, coef=coef, opts=o, cols=cols, Ka=Ka, Kl=Kl, P=P, ia=ia, ib=ib,
                b_pos=b_pos, names=names, lo=lo, hi=hi)


def empty_results(N, K):
    """The result arrays every fit has, for N stars that no fit has reached yet: chisq and fisher NaN, status NAN, niter and at_bound 0."""
    return dict(chisq=np.full(N, np.nan), fisher=np.full((N, K, K), np.nan), status=np.full(N, _lib.LMFIT_NAN, dtype=np.int32),
                niter=np.zeros(N, dtype=np.int32), at_bound=np.zeros(N, dtype=np.uint32))


def keep_best_rank(index, out, per_star, fit_rank, record):
    """One result per star over the ranks of a bank search.  ``index`` [N, k]: < 0 where a star has no template of that rank.
    ``fit_rank(sel, r)``: the result dict of the fit of stars ``sel`` started from rank r, called once per rank that any star has.  A
    star takes the result of lowest chi^2 among those whose status is not NAN / SINGULAR, the lower rank on a tie, and rank 0's (its
    first) if none qualifies: the keys ``per_star`` of ``out`` and ``start_rank`` are written, and ``record(dst, r)`` records the starts
    of the stars ``dst`` that took rank r.  Returns ``out``."""
    def valid(status):
        return (status != _lib.LMFIT_NAN) & (status != _lib.LMFIT_SINGULAR)
    for r in range(index.shape[1]):
        sel = np.flatnonzero(index[:, r] >= 0)
        if len(sel) == 0:
            continue
        res = fit_rank(sel, r)
        held = out["start_rank"][sel] >= 0
        held_valid = held & valid(out["status"][sel])
        take = ~held | (valid(res["status"]) & (~held_valid | (res["chisq"] < out["chisq"][sel])))
        dst = sel[take]
        for name in per_star:
            out[name][dst] = res[name][take]
        out["start_rank"][dst] = r
        record(dst, r)
    return out


class _DeviceArray(object):
    """A device pointer the library owns, as torch reads it (``torch.as_tensor``)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


class LMHandle(object):
    """Owner of one ``payne_lmfit`` handle: K parameters, room for ``max_stars`` stars."""

    def __init__(self, K, max_stars, device, **opts):
        import torch
        self.torch, self.lib = torch, _lib.load()
        self.device, self.K, self.max_stars = device, int(K), int(max_stars)
        self.opts = _lib.LmfitOpts(**opts)
        self._h = C.c_void_p()
        rc = self.lib.payne_lmfit_create(self.device.index, self.K, self.max_stars, C.byref(self.opts), C.byref(self._h))
        if rc != 0:
            raise RuntimeError("payne_lmfit_create failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))
        self.B = 0
        with torch.cuda.device(self.device):
            self._trial = torch.as_tensor(_DeviceArray(self.lib.payne_lmfit_trial(self._h), (self.max_stars, self.K), "<f8"), device=self.device)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self, x0, lo, hi):
        """x0 [B, K] (a host array or a device tensor), the box lo, hi [K]."""
        torch = self.torch
        x = x0 if isinstance(x0, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x0, dtype=np.float64))
        x = x.to(device=self.device, dtype=torch.float64).contiguous()
        if x.dim() != 2 or x.shape[1] != self.K:
            raise ValueError("x0 must be [B, %d], got %s" % (self.K, tuple(x.shape)))
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        if lo.shape != (self.K,) or hi.shape != (self.K,):
            raise ValueError("lo and hi must be [%d]" % self.K)
        rc = self.lib.payne_lmfit_begin(self._h, x.data_ptr(), lo.ctypes.data, hi.ctypes.data, x.shape[0], self._stream())
        if rc != 0:
            raise RuntimeError("payne_lmfit_begin failed (%d)" % rc)
        self.B = x.shape[0]

    def trial(self):
        """x_trial [B, K]: a view of the handle's own memory, valid in stream order."""
        return self._trial[:self.B]

    def _check_blocks(self, blocks, flux, w, x=None, P=0):
        """What the four updates ask of the tensors they share: every (rows, r) of ``blocks`` contiguous fp32 [B, r, n] (r None: any
        number of rows), flux contiguous fp32 [B, n], w contiguous fp64 [B, n] and, with P > 0, x contiguous fp64 [n].  Returns n."""
        torch, B, n = self.torch, self.B, blocks[0][0].shape[-1]
        need_x = P > 0
        if any(t.dim() != 3 or t.shape[0] != B or t.shape[2] != n or (r is not None and t.shape[1] != r) for t, r in blocks) \
                or tuple(flux.shape) != (B, n) or tuple(w.shape) != (B, n) or (need_x and (x is None or tuple(x.shape) != (n,))):
            raise ValueError("rows %s, flux and w [%d, n]%s; got %s, %s, %s, %s"
                             % (" and ".join("[%d, %s, n]" % (B, "any" if r is None else r) for _, r in blocks), B, ", x [n]" if need_x else "",
                                [tuple(t.shape) for t, _ in blocks], tuple(flux.shape), tuple(w.shape), None if x is None else tuple(x.shape)))
        f32, f64 = [t for t, _ in blocks] + [flux], [w] + ([x] if need_x else [])
        if any(a.dtype != torch.float32 or not a.is_contiguous() for a in f32) or any(a.dtype != torch.float64 or not a.is_contiguous() for a in f64):
            raise ValueError("rows and flux contiguous fp32, w and x contiguous fp64")
        return n

    def update(self, rows, flux, w):
        """rows fp32 [B, 1 + K, n] (the model, then its derivatives), flux fp32 [B, n], w fp64 [B, n]: device tensors."""
        n = self._check_blocks([(rows, 1 + self.K)], flux, w)
        rc = self.lib.payne_lmfit_update(self._h, rows.data_ptr(), n, flux.data_ptr(), w.data_ptr(), n, n, self._stream())
        if rc != 0:
            raise RuntimeError("payne_lmfit_update failed (%d)" % rc)

    def update_poly(self, rows, flux, w, x, P):
        """The update for model x polynomial, the handle's last P parameters the Chebyshev coefficients (payne_lmfit_update_poly):
        rows fp32 [B, 1 + K - P, n] (the un-normalised model, then its derivatives), flux fp32 [B, n], w fp64 [B, n], x fp64 [n]
        (``contfit.abscissa``): device tensors."""
        P = int(P)
        if not 1 <= P <= self.K:
            raise ValueError("P must be 1 .. %d, got %d" % (self.K, P))
        n = self._check_blocks([(rows, 1 + self.K - P)], flux, w, x, P)
        rc = self.lib.payne_lmfit_update_poly(self._h, P, rows.data_ptr(), n, flux.data_ptr(), w.data_ptr(), n, x.data_ptr(), n, self._stream())
        if rc != 0:
            raise RuntimeError("payne_lmfit_update_poly failed (%d)" % rc)

    def update_phot(self, rows, flux, w, x, P, Kp, sed_col, mags, dmags, obs, pw, mu=None, sigma=None):
        """The update for spectrum and magnitudes together (payne_lmfit_update_phot): the handle's parameters are K - Kp - P of the
        spectral model, Kp that only the photometry sees and P >= 0 Chebyshev coefficients.  rows fp32 [B, 1 + K - Kp - P, n], flux,
        w, x as ``update_poly`` takes them (x None for P = 0); sed_col [K] host ints; mags, obs, pw fp64 [B, F], dmags fp64
        [B, F, ncol] (``SEDFit.grad_device``'s at the trial point); mu, sigma fp64 [B, K] or neither: device tensors."""
        torch = self.torch
        B, P, Kp, K = self.B, int(P), int(Kp), self.K
        Km = K - Kp - P
        sed_col = np.ascontiguousarray(sed_col, dtype=np.int32)
        if P < 0 or Kp < 0 or Km < 0 or sed_col.shape != (K,):
            raise ValueError("P >= 0, Kp >= 0, P + Kp <= %d and sed_col [%d]; got P = %d, Kp = %d, sed_col %s" % (K, K, P, Kp, sed_col.shape))
        n = self._check_blocks([(rows, 1 + Km)], flux, w, x, P)
        F = mags.shape[-1]
        if dmags.dim() != 3 or tuple(dmags.shape[:2]) != (B, F) or any(tuple(a.shape) != (B, F) for a in (mags, obs, pw)):
            raise ValueError("mags, obs, pw [%d, F] and dmags [%d, F, ncol]; got %s, %s, %s, %s" % (B, B, tuple(mags.shape), tuple(obs.shape), tuple(pw.shape), tuple(dmags.shape)))
        if (mu is None) != (sigma is None) or (mu is not None and (tuple(mu.shape) != (B, K) or tuple(sigma.shape) != (B, K))):
            raise ValueError("mu and sigma [%d, %d], both or neither" % (B, K))
        if any(a.dtype != torch.float64 or not a.is_contiguous() for a in [mags, dmags, obs, pw] + ([mu, sigma] if mu is not None else [])):
            raise ValueError("mags, dmags, obs, pw, mu and sigma contiguous fp64")
        rc = self.lib.payne_lmfit_update_phot(self._h, Km, Kp, P, rows.data_ptr(), n, flux.data_ptr(), w.data_ptr(), n, x.data_ptr() if P > 0 else None, n,
                                              F, dmags.shape[2], sed_col.ctypes.data, mags.data_ptr(), dmags.data_ptr(), obs.data_ptr(), pw.data_ptr(),
                                              None if mu is None else mu.data_ptr(), None if sigma is None else sigma.data_ptr(), self._stream())
        if rc != 0:
            raise RuntimeError("payne_lmfit_update_phot failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))

    def update_pair(self, rows_a, rows_b, flux, w, ia, ib, P=0, x=None):
        """The update for two components with a light ratio times a polynomial (payne_lmfit_update_pair): the handle's parameters are
        Kl = K - 1 - P that the components see, the ratio q and P >= 0 Chebyshev coefficients.  rows_a fp32 [B, 1 + Ka, n] and rows_b
        fp32 [B, 1 + Kb, n] (a component's model, then its derivatives), flux fp32 [B, n], w fp64 [B, n], x fp64 [n] (None for
        P = 0): device tensors; ia, ib [Kl] host ints: parameter k is derivative ia[k] of A and ib[k] of B, -1 for none."""
        P, K = int(P), self.K
        Kl = K - 1 - P
        ia, ib = np.ascontiguousarray(ia, dtype=np.int32), np.ascontiguousarray(ib, dtype=np.int32)
        if P < 0 or Kl < 0 or ia.shape != (Kl,) or ib.shape != (Kl,):
            raise ValueError("P >= 0, 1 + P <= %d and ia, ib [%d]; got P = %d, ia %s, ib %s" % (K, max(Kl, 0), P, ia.shape, ib.shape))
        n = self._check_blocks([(rows_a, None), (rows_b, None)], flux, w, x, P)
        Ka, Kb = rows_a.shape[1] - 1, rows_b.shape[1] - 1
        if Ka < 0 or Kb < 0 or np.any(ia < -1) or np.any(ia >= Ka) or np.any(ib < -1) or np.any(ib >= Kb) or np.any((ia < 0) & (ib < 0)):
            raise ValueError("ia in [-1, %d), ib in [-1, %d), not both -1; got %s, %s" % (Ka, Kb, ia.tolist(), ib.tolist()))
        rc = self.lib.payne_lmfit_update_pair(self._h, Kl, P, ia.ctypes.data if Kl else None, ib.ctypes.data if Kl else None, rows_a.data_ptr(), Ka,
                                              rows_b.data_ptr(), Kb, n, flux.data_ptr(), w.data_ptr(), n, x.data_ptr() if P > 0 else None, n, self._stream())
        if rc != 0:
            raise RuntimeError("payne_lmfit_update_pair failed (%d)" % rc)

    def status(self):
        torch = self.torch
        s = torch.empty(self.B, dtype=torch.int32, device=self.device)
        rc = self.lib.payne_lmfit_result(self._h, None, None, None, None, None, s.data_ptr(), None, None, self._stream())
        if rc != 0:
            raise RuntimeError("payne_lmfit_result failed (%d)" % rc)
        return s

    def result(self):
        """dict of device tensors: x_best, chisq, A, g, lambda, status, niter, at_bound."""
        torch, B, K = self.torch, self.B, self.K
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        out = dict(x_best=torch.empty((B, K), **f64), chisq=torch.empty(B, **f64), A=torch.empty((B, K, K), **f64), g=torch.empty((B, K), **f64),
                   **{"lambda": torch.empty(B, **f64)}, status=torch.empty(B, **i32), niter=torch.empty(B, **i32), at_bound=torch.empty(B, **i32))
        order = ("x_best", "chisq", "A", "g", "lambda", "status", "niter", "at_bound")
        rc = self.lib.payne_lmfit_result(self._h, *([out[k].data_ptr() if B else None for k in order] + [self._stream()]))
        if rc != 0:
            raise RuntimeError("payne_lmfit_result failed (%d)" % rc)
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._trial = None
            self.lib.payne_lmfit_destroy(self._h)                   # (waits for the device)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OptFit(object):
    """OptFit(specANNpath, NNtype, obs_wave): least-squares fits of the labels on the observed grid ``obs_wave``."""

    def __init__(self, specANNpath, NNtype, obs_wave, device=None, b_max=256, Cnnpath=None):
        if Cnnpath is not None:
            raise NotImplementedError("OptFit with a continuum network (Cnnpath): the model is a product of two networks")
        self.obs_wave = np.ascontiguousarray(obs_wave, dtype=np.float64)
        if self.obs_wave.ndim != 1 or len(self.obs_wave) < 1:
            raise ValueError("obs_wave must be a vector")
        self.predictor = PayneSpecPredict(specANNpath, NNtype=NNtype, device=device, b_max=b_max)
        self.n_labels = self.predictor.anns.n_labels
        self.timing = None

    def labels(self, fit_vrad=False):
        return [THETA_SPEC_COLS[c] for c in fitted_columns(self.n_labels, fit_vrad)]

    def fit(self, flux, eflux, start, fit_vrad=False, bounds=None, vrad_step=0.25, check_every=4, lsf=None, timing=False, **opts):
        """flux, eflux [N, nobs] on ``obs_wave`` (eflux zero or not finite: the pixel does not count), start [N, 8] = Teff, logg,
        feh, afe, vrad, vrot, vmic, inst_R (getspec's columns, as ``Forecast.jacobian`` takes them) -> dict: ``pars`` [N, 8],
        ``chisq``, ``npix`` (pixels with w != 0), ``fisher`` [N, K, K], ``err`` [N, K], ``status`` (``_lib.LMFIT_*``), ``niter``
        (evaluations of the model), ``at_bound`` (bit k: fitted column k sits on its bound), ``labels`` (the K fitted columns).
        ``opts``: lambda0, down, up, lambda_min, lambda_max, xtol, maxiter (payne_lmfit_opts).  ``timing``: event pairs around the
        three steps of every iteration, summed into ``self.timing`` (ms; for tools/optfit_bench.py)."""
        if lsf is not None:
            raise NotImplementedError("OptFit with an LSF vector: the rows are not pushed through it (PayneSpecPredict.getgrad)")
        anns, D = self.predictor.anns, self.n_labels
        flux, eflux, start, lo, hi, o = check_fit_args(flux, eflux, start, len(self.obs_wave), D, anns.xmin, anns.xmax, fit_vrad=fit_vrad,
                                                       bounds=bounds, vrad_step=vrad_step, check_every=check_every, **opts)
        N = flux.shape[0]
        cols = fitted_columns(D, fit_vrad)
        w = weights_from_errors(eflux)
        out = dict(pars=start.copy(), npix=(w != 0.0).sum(axis=1), labels=self.labels(fit_vrad), **empty_results(N, len(cols)))

        def block(handle, idx):
            return start[idx][:, cols], start[idx], lambda rows, flux_d, w_d, mark: handle.update(rows, flux_d, w_d)

        def place(idx, xb):
            out["pars"][idx][:, cols] = xb                           # (idx is a slice here, so this writes through a view)
        return self._fit_blocks(out, None, flux, w, lo, hi, o, block, place, cols=cols, fit_vrad=fit_vrad, vrad_step=vrad_step, check_every=check_every,
                                timing=timing)

    def _fit_blocks(self, out, sel, flux, w, lo, hi, opts, block, place, *, cols, fit_vrad, vrad_step, check_every, timing, nc=1, labels_of=None,
                    vrad_of=None, steps=("network", "broadening", "update"), nan_results=False):
        """The driver of every fit: the stars ``sel`` (indices; None: every star, and a block's ``idx`` is then a slice, so that
        ``flux[idx]`` copies nothing) walk in blocks through one handle of K = len(lo) parameters, and what the handle
        gives for a block goes into ``out`` -- chisq, fisher, status, niter and at_bound here, x_best [nb, K] through the fit's own
        ``place(idx, x_best)``; ``err`` is added and ``out`` returned.  A block holds as many stars as ``b_max`` rows allow: a star
        needs, for each of its ``nc`` components, the model's row, one per fitted column ``cols`` and two for a fitted Vrad.
        ``block(handle, idx)`` gives the stars ``idx`` their ``_run_block`` arguments (x0, theta, update); ``labels_of``, ``vrad_of``,
        ``steps`` are ``_run_block``'s, one component's by default.  ``nan_results``: x_best, fisher and chisq of a star whose status
        is NAN are NaN (``fit_binary``).  ``timing``: the ``steps`` are timed and summed into ``self.timing``."""
        eng, D = self.predictor.anns.engine, self.n_labels
        fit_vrad = bool(fit_vrad)
        if labels_of is None:
            def labels_of(xt):
                return xt[:, :D] if xt.shape[1] > D else xt

            def vrad_of(xt):
                return xt[:, D]
        self.predictor._bind(self.obs_wave)
        step = max(1, eng.b_max // (nc * (1 + len(cols) + 2 * int(fit_vrad))))
        self.timing = dict([(name, 0.0) for name in steps], iterations=0) if timing else None
        n = len(flux) if sel is None else len(sel)
        if n:
            handle = LMHandle(len(lo), min(step, n), eng.device, **opts)
            try:
                for s in range(0, n, step):
                    idx = slice(s, min(n, s + step)) if sel is None else sel[s:s + step]
                    x0, theta, update = block(handle, idx)
                    res = self._run_block(handle, flux[idx], w[idx], x0, lo, hi, theta, labels_of, vrad_of if fit_vrad else None, update, len(cols),
                                          float(vrad_step), int(check_every), int(opts["maxiter"]), steps)
                    xb, st, fisher, chisq = (res[k].cpu().numpy() for k in ("x_best", "status", "A", "chisq"))
                    if nan_results:
                        nan = st == _lib.LMFIT_NAN
                        xb[nan], fisher[nan], chisq[nan] = np.nan, np.nan, np.nan
                    out["chisq"][idx] = chisq
                    out["fisher"][idx] = fisher
                    out["status"][idx] = st
                    out["niter"][idx] = res["niter"].cpu().numpy()
                    out["at_bound"][idx] = res["at_bound"].cpu().numpy().astype(np.uint32)
                    place(idx, xb)
            finally:
                handle.close()
        out["err"] = crlb_from_fisher(out["fisher"])
        return out

    def _run_block(self, handle, flux, w, x0, lo, hi, theta, labels_of, vrad_of, update, Kc, vrad_step, check_every, maxiter, steps):
        """One block of nb stars through the handle, from ``begin(x0, lo, hi)`` to ``result()``.  ``theta`` [nc * nb, 8]: getspec's
        columns of every component at the start, the nc components stacked along the batch axis, as the rows are: rows [nc * nb, 1 + Kc,
        nobs] holds a component's model, the derivatives by its labels and, with a fitted Vrad, by Vrad (a central difference of the
        broadened model at Vrad +- ``vrad_step``).  ``labels_of(x_trial)``: the labels [nc * nb, D] the network is evaluated at;
        ``vrad_of(x_trial)``: the fitted Vrad [nc * nb], None where Vrad is fixed.  They are two functions because a gather they
        enqueue belongs to the step that uses it.  ``update(rows, flux_d, w_d, mark)`` issues the handle's update from the filled
        rows, and calls ``mark()`` behind each further step it enqueues before that; ``steps`` names the timed steps in order."""
        Pr = self.predictor
        eng, D, jac_net = Pr.anns.engine, self.n_labels, Pr._jacobian()
        torch, dev = eng.torch, eng.device
        nobs, nr = flux.shape[1], theta.shape[0]
        flux_d = torch.as_tensor(np.ascontiguousarray(flux)).to(dev)
        w_d = torch.as_tensor(np.ascontiguousarray(w)).to(dev)
        handle.begin(x0, lo, hi)
        xt = handle.trial()
        # the theta blocks, uploaded once: the model's [nr], the derivative rows' [nr * D], and Vrad +- step's [2 nr]
        th = np.full((nr, eng.ncols), np.nan)
        th[:, :8] = theta
        th_y = torch.as_tensor(th).to(dev)
        th_j = th_y.repeat_interleave(D, dim=0)
        th_pm = th_y.repeat(2, 1) if vrad_of is not None else None
        rows = torch.empty((nr, 1 + Kc, nobs), dtype=torch.float32, device=dev)
        tm = self.timing
        marks = []

        def mark():
            if tm is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(torch.cuda.current_stream(dev))
                marks.append(ev)
        it = 0
        while it < maxiter:
            it += 1
            mark()
            y, jac = jac_net.eval(labels_of(xt))
            mark()
            if vrad_of is not None:
                v = vrad_of(xt)
                th_y[:, 4] = v
                th_j[:, 4] = v.repeat_interleave(D)
                th_pm[:nr, 4] = v + vrad_step
                th_pm[nr:, 4] = v - vrad_step
                pm = eng.smooth_batch(y.repeat(2, 1), th_pm, stage=2)
                rows[:, Kc] = (pm[:nr] - pm[nr:]) / (2.0 * vrad_step)
            rows[:, 0] = eng.smooth_batch(y, th_y, stage=2)
            rows[:, 1:1 + D] = smooth_rows(eng, jac.reshape(nr * D, -1), th_j, 2).reshape(nr, D, nobs)
            mark()
            update(rows, flux_d, w_d, mark)
            mark()
            if it % check_every == 0 and not bool((handle.status() == _lib.LMFIT_RUNNING).any().item()):
                break
        res = handle.result()
        if tm is not None:
            torch.cuda.synchronize(dev)
            for i in range(0, len(marks), len(steps) + 1):                                         # a mark before each step and one behind the last
                for j, name in enumerate(steps):
                    tm[name] += marks[i + j].elapsed_time(marks[i + j + 1])
            tm["iterations"] += it
        return res

    def model_spectra(self, pars):
        """The model ``fit`` minimises at pars [N, 8] (getspec's columns): payne_specjac_eval's y through payne_smooth_batch, fp32
        [N, nobs] on the device."""
        P = self.predictor
        eng = P.anns.engine
        pars = np.atleast_2d(np.asarray(pars, dtype=np.float64))
        P._bind(self.obs_wave)
        out = eng.torch.empty((len(pars), len(self.obs_wave)), dtype=eng.torch.float32, device=eng.device)
        cols = fitted_columns(self.n_labels, False)
        for s in range(0, len(pars), eng.b_max):
            blk = pars[s:s + eng.b_max]
            y, _ = P._jacobian().eval(blk[:, cols])
            th = np.full((len(blk), eng.ncols), np.nan)
            th[:, :8] = blk
            out[s:s + eng.b_max] = eng.smooth_batch(y, th, stage=2)
        return out

    def fit_with_continuum(self, flux, eflux, start, npoly=4, rounds=3, clip=None, **fit_kwargs):
        """Labels and a continuum polynomial of ``npoly`` Chebyshev coefficients per star, by block-coordinate descent on
        chi^2 = sum w (flux - model(x) p)^2.  Each of ``rounds`` rounds fits the polynomial against the model at the current
        parameters (``contfit.ContinuumFit.fit`` on ``model_spectra``: the linear block, solved exactly) and then runs ``fit`` on the
        normalised flux and errors, started from the round before: sum w (f - m p)^2 = sum (w p^2) (f / p - m)^2, so both blocks
        descend the same chi^2.  ``clip``: dict(nclip, kappa, rescale, drop_clipped) for the polynomial's kappa-sigma clipping.
        Returns ``fit``'s dict of the last round plus ``coef`` [N, npoly] (``polycalc``'s), ``cont_status`` (``_lib.CONTFIT_*``) and
        ``chisq_rounds`` [N, rounds] (the label fit's chi^2 of every round).  A star whose continuum status is not OK / NONPOSITIVE
        in some round keeps its last valid result from there on, and that status in ``cont_status``; one that never had a valid
        continuum has status NAN and NaN ``pars`` in the fitted columns.  ``fit_kwargs`` go to ``fit``.

        The alternation converges linearly and slowly (NOTES.md: about 40 rounds to come within 0.01 sigma of its fixed point);
        ``fit_joint`` minimises the same chi^2 over labels and coefficients in one Levenberg-Marquardt fit and is the method to
        prefer for up to 15 parameters."""
        from .contfit import ContinuumFit
        if int(rounds) < 1:
            raise ValueError("rounds must be at least 1")
        flux, eflux, start = check_fit_args(flux, eflux, start, len(self.obs_wave), self.n_labels, self.predictor.anns.xmin, self.predictor.anns.xmax,
                                            **{k: v for k, v in fit_kwargs.items() if k not in ("lsf", "timing")})[:3]
        fit_vrad = bool(fit_kwargs.get("fit_vrad", False))
        cols = fitted_columns(self.n_labels, fit_vrad)
        N, K = flux.shape[0], len(cols)
        cont = ContinuumFit(self.obs_wave, npoly=npoly, device=self.predictor.anns.engine.device, **(clip or {}))
        pars = start.copy()
        out = dict(pars=start.copy(), npix=np.zeros(N, dtype=np.int64), labels=self.labels(fit_vrad), err=np.full((N, K), np.nan),
                   coef=np.full((N, int(npoly)), np.nan), cont_status=np.full(N, _lib.CONTFIT_OK, dtype=np.int32),
                   chisq_rounds=np.full((N, int(rounds)), np.nan), **empty_results(N, K))
        out["pars"][:, cols] = np.nan
        alive = np.ones(N, dtype=bool)
        for r in range(int(rounds)):
            sel = np.flatnonzero(alive)
            if len(sel) == 0:
                break
            c = cont.fit(flux[sel], eflux[sel], self.model_spectra(pars[sel]))
            c = {k: v.cpu().numpy() for k, v in c.items()}
            good = (c["status"] == _lib.CONTFIT_OK) | (c["status"] == _lib.CONTFIT_NONPOSITIVE)
            out["cont_status"][sel] = c["status"]
            alive[sel[~good]] = False
            if not good.any():
                continue
            dst = sel[good]
            res = self.fit(c["flux"][good], c["eflux"][good], pars[dst], **fit_kwargs)
            for name in ("pars", "chisq", "npix", "fisher", "status", "niter", "at_bound", "err"):
                out[name][dst] = res[name]
            out["coef"][dst] = c["coef"][good]
            out["chisq_rounds"][dst, r] = res["chisq"]
            ok = (res["status"] != _lib.LMFIT_NAN) & (res["status"] != _lib.LMFIT_SINGULAR)
            pars[dst[ok]] = res["pars"][ok]
        return out

    def fit_joint(self, flux, eflux, start, npoly=4, coef=None, clip=None, fit_vrad=False, bounds=None, coef_bounds=None, vrad_step=0.25,
                  check_every=4, lsf=None, timing=False, **opts):
        """Labels (Vrad with ``fit_vrad``) and a continuum polynomial of ``npoly`` Chebyshev coefficients per star in ONE
        Levenberg-Marquardt fit of chi^2 = sum w (flux - model(x) p)^2 over all K = K_m + npoly <= 15 parameters: what
        ``fit_with_continuum`` approaches by alternation, at the cost of one ``fit``.  An iteration is ``fit``'s three enqueued
        steps with the update replaced by payne_lmfit_update_poly, which forms the rows p dm/dtheta, m T_j and flux - m p in
        registers; nothing is normalised and no row is stored.

        ``coef`` [N, npoly]: the starting coefficients (``polycalc``'s); by default one ``ContinuumFit.fit`` against
        ``model_spectra(start)``, with ``clip`` (dict(nclip, kappa, rescale)) its kappa-sigma clipping, and the pixels its last solve
        dropped do not count in the joint fit.  A star whose continuum status is not OK / NONPOSITIVE gets status NAN and NaN
        results.  ``coef_bounds`` [npoly, 2]: the coefficients' box, finite; +-1e30 by default.  The other arguments are ``fit``'s.

        Returns ``fit``'s dict with ``labels`` (the fitted columns, then pc_0 ..), ``fisher`` [N, K, K], ``err`` [N, K] and
        ``at_bound`` over all K parameters -- ``err`` is sqrt(diag(inv(fisher))), so the labels' entries are marginalised over the
        polynomial -- plus ``coef`` [N, npoly] and ``cont_status`` (``_lib.CONTFIT_*``; OK where ``coef`` was given)."""
        if lsf is not None:
            raise NotImplementedError("OptFit with an LSF vector: the rows are not pushed through it (PayneSpecPredict.getgrad)")
        Pr = self.predictor
        anns, eng, D = Pr.anns, Pr.anns.engine, self.n_labels
        flux, eflux, start, lo, hi, o, coef, clip = check_joint_args(flux, eflux, start, len(self.obs_wave), D, anns.xmin, anns.xmax, npoly=npoly, coef=coef,
                                                                     clip=clip, fit_vrad=fit_vrad, bounds=bounds, coef_bounds=coef_bounds,
                                                                     vrad_step=vrad_step, check_every=check_every, **opts)
        from .contfit import abscissa
        N = flux.shape[0]
        cols = fitted_columns(D, fit_vrad)
        Km, P = len(cols), int(npoly)
        w = weights_from_errors(eflux)
        cont_status = np.full(N, _lib.CONTFIT_OK, dtype=np.int32)
        if coef is None:
            coef, cont_status, w = self._start_continuum(flux, eflux, self.model_spectra(start), P, clip, w)
        out = dict(pars=start.copy(), npix=(w != 0.0).sum(axis=1), labels=self.labels(fit_vrad) + ["pc_%d" % j for j in range(P)],
                   coef=np.full((N, P), np.nan), cont_status=cont_status, **empty_results(N, Km + P))
        out["pars"][:, cols] = np.nan
        x_d = eng.torch.as_tensor(abscissa(self.obs_wave)).to(eng.device)

        def block(handle, idx):
            x0 = np.concatenate([start[idx][:, cols], np.ascontiguousarray(coef[idx], dtype=np.float64)], axis=1)
            return x0, start[idx], lambda rows, flux_d, w_d, mark: handle.update_poly(rows, flux_d, w_d, x_d, P)

        def place(idx, xb):
            out["pars"][idx[:, None], np.asarray(cols)[None, :]] = xb[:, :Km]
            out["coef"][idx] = xb[:, Km:]
        return self._fit_blocks(out, self._with_continuum(cont_status), flux, w, lo, hi, o, block, place, cols=cols, fit_vrad=fit_vrad, vrad_step=vrad_step,
                                check_every=check_every, timing=timing)

    @staticmethod
    def _with_continuum(cont_status):
        """The stars a starting continuum fit left fit to go on with: status OK or NONPOSITIVE."""
        return np.flatnonzero((cont_status == _lib.CONTFIT_OK) | (cont_status == _lib.CONTFIT_NONPOSITIVE))

    def _start_continuum(self, flux, eflux, model, P, clip, w):
        """The starting coefficients where the caller gave none: one ``ContinuumFit.fit`` of P coefficients against ``model`` (fp32
        [N, nobs] on the device).  ``clip``: ``fit_joint``'s dict (empty: no clipping) -- the pixels the last solve dropped get weight 0
        in ``w`` -- or None: ``ContinuumFit``'s own defaults and ``w`` as it is (``fit_binary``).  Returns (coef [N, P], cont_status
        int32 [N], w)."""
        from .contfit import ContinuumFit, abscissa
        cont = ContinuumFit(self.obs_wave, npoly=P, device=self.predictor.anns.engine.device, **({} if clip is None else dict(drop_clipped=True, **clip)))
        c = cont.fit(flux, eflux, model, normalise=bool(clip))
        coef = c["coef"].cpu().numpy()                                # (a device model gives device tensors)
        if clip:                                                      # a counting pixel whose weight came back 0 under a positive polynomial was clipped
            positive = np.polynomial.chebyshev.chebval(abscissa(self.obs_wave), np.nan_to_num(coef).T) > 0.0
            w = np.where((c["weights"].cpu().numpy() == 0.0) & positive, 0.0, w)
        return coef, c["status"].cpu().numpy().astype(np.int32), w

    def fit_specphot(self, flux, eflux, mags, emags, start, phot_start, sed, free_phot=("logR", "Av"), npoly=0, coef=None, clip=None, fit_vrad=False,
                     bounds=None, coef_bounds=None, prior=None, vrad_step=0.25, check_every=4, timing=False, **opts):
        """Spectrum and photometry in ONE Levenberg-Marquardt fit: chi^2 = sum_p w_p (flux_p - model_p p(x_p))^2 + sum_f (mag_f -
        model_f)^2 / emag_f^2 + Gaussian priors, over K = K_m + K_p + npoly <= 15 parameters.  Teff, log(g), [Fe/H], [a/Fe] are shared
        by both; Vmic (five-label network) and Vrad (``fit_vrad``) are the spectrum's; ``free_phot`` names the photometric-only
        parameters that are fitted (among logR, Dist, Av, or logA, Av with ``sed.photscale``).  ``sed``: a ``SEDFit`` on the same
        device, whose filters and ``photscale`` define the magnitudes; ``mags``, ``emags`` [N, F] follow ``SEDFit.fit``'s rule for a
        filter that does not count; ``phot_start`` [N, ncol - 4] holds the photometric-only columns in ``sedfit.par_names(photscale)[4:]``
        order, those not in ``free_phot`` stay fixed there.  ``flux``, ``eflux``, ``start``, ``npoly``, ``coef``, ``clip``,
        ``coef_bounds`` are ``fit_joint``'s; ``npoly=0``: no polynomial.

        The default box of a shared label is the intersection of the spectral network's and ``sed``'s; ``bounds`` = {name: (lo, hi)}
        over all fitted parameters (``labels`` of the result).  ``prior`` = {name: (mu [N], sigma [N])}, Gaussian, on any fitted
        parameter, an infinite sigma meaning none.  logR and Dist are exactly degenerate in the magnitudes and the spectrum sees
        neither: ``free_phot`` with both needs a finite prior on one of them for every star (a parallax, say).

        One iteration is four enqueued steps and no host look: payne_specjac_eval, the broadening of the 1 + K_m rows,
        ``sed.grad_device`` on the photometric rows gathered from x_trial on the device, and payne_lmfit_update_phot, which adds the
        photometric block and the priors to the spectral normal equations before the step is taken.

        Returns ``fit_joint``'s dict over all K parameters (``fisher`` [N, K, K] with the priors, ``err`` = sqrt(diag(inv(fisher))): the
        labels' errors are marginalised over logR / Dist / Av and the polynomial; ``chisq`` with the magnitudes' and the priors'
        terms) plus ``phot_pars`` [N, ncol] (the photometric row at the solution), ``nfilt`` (filters that count) and ``mags_model``
        [N, F] there (one more ``sed.grad`` a block of stars after the loop, with its copy to the host).  ``timing``: as ``fit``'s,
        with ``sed`` the third step.

        Status on real data.  The spectral model and its rows are fp32, so chi^2 at a trial point carries a rounding term of about
        2 w sqrt(n) |r| 6e-8 (r the spectral residual at the solution) that changes from trial to trial: 2e-6 .. 5e-6 measured with 37
        pixels at S/N 100 once magnitudes that scatter by their 0.02 mag errors pull the labels off the spectrum's own minimum.  The
        step that decides convergence, xtol = 1e-3 sigma, gains 1e-6.  update_star accepts a trial on chi^2 <= the best so far, so a
        best point that rounded low is followed by rejections until lambda is large enough for the model not to change (``CONVERGED``
        after ten or twenty evaluations) or reaches lambda_max (``STALLED``).  Both end within 1e-2 sigma of the fp64 solution
        (tests/test_lmfit_phot_gpu.py) and both carry a valid ``fisher`` and ``err``: treat ``STALLED`` as converged here, or pass a
        larger ``xtol``.  ``fit`` and ``fit_joint`` meet the same floor on spectra whose residuals are not small."""
        from . import sedfit
        if not isinstance(sed, sedfit.SEDFit):
            raise TypeError("sed must be a SEDFit")
        Pr = self.predictor
        anns, eng, D = Pr.anns, Pr.anns.engine, self.n_labels
        c = check_specphot_args(flux, eflux, mags, emags, start, phot_start, len(self.obs_wave), D, anns.xmin, anns.xmax, sed.F, sed.xmin, sed.xmax,
                                photscale=sed.photscale, free_phot=free_phot, npoly=npoly, coef=coef, clip=clip, fit_vrad=fit_vrad, bounds=bounds,
                                coef_bounds=coef_bounds, prior=prior, vrad_step=vrad_step, check_every=check_every, **opts)
        from .contfit import abscissa
        torch = sed._setup()
        dev = eng.device
        if sed.device != dev:
            raise ValueError("sed is on %s, the spectral network on %s" % (sed.device, dev))
        flux, eflux, start, coef, clip, o = c["flux"], c["eflux"], c["start"], c["coef"], c["clip"], c["opts"]
        cols, Km, Kp, P, lo, hi, phot_cols = c["cols"], c["Km"], c["Kp"], c["P"], c["lo"], c["hi"], c["phot_cols"]
        N = flux.shape[0]
        w = weights_from_errors(eflux)
        cont_status = np.full(N, _lib.CONTFIT_OK, dtype=np.int32)
        if P and coef is None:
            coef, cont_status, w = self._start_continuum(flux, eflux, self.model_spectra(start), P, clip, w)
        phot_pars = np.concatenate([start[:, :4], c["phot_start"]], axis=1)
        out = dict(pars=start.copy(), npix=(w != 0.0).sum(axis=1), labels=list(c["names"]), coef=np.full((N, P), np.nan), cont_status=cont_status,
                   phot_pars=phot_pars.copy(), nfilt=(c["pw"] != 0.0).sum(axis=1), mags_model=np.full((N, sed.F), np.nan),
                   **empty_results(N, Km + Kp + P))
        out["pars"][:, cols] = np.nan
        out["phot_pars"][:, :4] = np.nan
        out["phot_pars"][:, phot_cols] = np.nan
        x_d = torch.as_tensor(abscissa(self.obs_wave)).to(dev) if P else None
        idx_d = torch.as_tensor(np.asarray(phot_cols, dtype=np.int64)).to(dev)

        def block(handle, idx):
            # on the device: the photometric rows (their fitted columns are overwritten from x_trial every iteration), the magnitudes
            # and 1 / sigma^2, the priors
            pars_d, obs_d, pw_d, mu_d, sigma_d = (None if a is None else torch.as_tensor(np.ascontiguousarray(a[idx], dtype=np.float64)).to(dev)
                                                  for a in (phot_pars, c["obs"], c["pw"], c["mu"], c["sigma"]))
            x0 = np.concatenate([start[idx][:, cols], phot_pars[idx][:, phot_cols]] + ([np.ascontiguousarray(coef[idx], dtype=np.float64)] if P else []), axis=1)

            def update(rows, flux_d, w_d, mark):
                xt = handle.trial()
                pars_d[:, :4] = xt[:, :4]
                if Kp:
                    pars_d.index_copy_(1, idx_d, xt[:, Km:Km + Kp])
                mags, dmags = sed.grad_device(pars_d)
                mark()
                handle.update_phot(rows, flux_d, w_d, x_d, P, Kp, c["sed_col"], mags, dmags, obs_d, pw_d, mu_d, sigma_d)
            return x0, start[idx], update

        def place(idx, xb):
            out["pars"][idx[:, None], np.asarray(cols)[None, :]] = xb[:, :Km]
            out["phot_pars"][idx, :4] = xb[:, :4]
            if Kp:
                out["phot_pars"][idx[:, None], np.asarray(phot_cols)[None, :]] = xb[:, Km:Km + Kp]
            out["coef"][idx] = xb[:, Km + Kp:]
            out["mags_model"][idx] = sed.grad(out["phot_pars"][idx])[0]
        return self._fit_blocks(out, self._with_continuum(cont_status), flux, w, lo, hi, o, block, place, cols=cols, fit_vrad=fit_vrad, vrad_step=vrad_step,
                                check_every=check_every, timing=timing, steps=("network", "broadening", "sed", "update"))

    def fit_from_bank(self, flux, eflux, bank, topk=1, **fit_kwargs):
        """``fit`` started from the ``topk`` templates of ``bank`` (a ``tmatch.TemplateBank`` on this fitter's ``obs_wave``) that
        match each star best: the template's labels, Vrot, Inst_R and Vrad are the start (``fit_vrad`` then refines Vrad).  One
        ``fit`` call per rank over the stars that have a template of that rank; per star the result of lowest chi^2 among those
        whose status is not NAN / SINGULAR is kept, the lower rank on a tie (rank 0's if none qualifies).  Returns ``fit``'s dict
        plus ``start_index`` (the template), ``start_chisq`` (its chi^2 in the search) and ``start_rank``.  A star that no template
        matches (every chi^2 NaN) keeps status NAN, NaN ``pars`` and ``start_index`` -1.  ``fit_kwargs`` go to ``fit``."""
        flux, eflux = self._bank_inputs(flux, eflux, bank, "match", fit_kwargs, ("start",), "fit_from_bank takes its starts from the bank")
        m = bank.match(flux, eflux, topk=topk)
        N = m["index"].shape[0]
        labels = self.labels(bool(fit_kwargs.get("fit_vrad", False)))
        out = dict(pars=np.full((N, 8), np.nan), npix=m["npix"], labels=labels, start_index=np.full(N, -1, dtype=np.int32), **self._bank_results(N, len(labels)))

        def record(dst, r):
            out["start_index"][dst], out["start_chisq"][dst] = m["index"][dst, r], m["chisq"][dst, r]
        return keep_best_rank(m["index"], out, ("pars", "chisq", "fisher", "status", "niter", "at_bound", "err"),
                              lambda sel, r: self.fit(flux[sel], eflux[sel], m["pars"][sel, r], **fit_kwargs), record)

    def _bank_inputs(self, flux, eflux, bank, search, kwargs, taken, message):
        """What the ``*_from_bank`` fits check first: ``bank`` has the method ``search`` and this fitter's grid, and ``kwargs`` names
        none of ``taken``, the arguments the bank supplies (``message`` says so).  Returns flux fp32 [N, nobs] and eflux fp64."""
        if not hasattr(bank, search) or not hasattr(bank, "obs_wave"):
            raise TypeError("bank must be a TemplateBank")
        if np.shape(bank.obs_wave) != self.obs_wave.shape or not np.array_equal(np.asarray(bank.obs_wave), self.obs_wave):
            raise ValueError("the bank's obs_wave differs from the fitter's")
        if any(name in kwargs for name in taken):
            raise TypeError(message)
        return np.atleast_2d(np.asarray(flux, dtype=np.float32)), np.atleast_2d(np.asarray(eflux, dtype=np.float64))

    @staticmethod
    def _bank_results(N, K):
        """``empty_results`` plus what a fit from a bank adds to them: ``err``, ``start_chisq`` and ``start_rank`` (-1: no rank yet)."""
        return dict(empty_results(N, K), err=np.full((N, K), np.nan), start_chisq=np.full(N, np.inf), start_rank=np.full(N, -1, dtype=np.int32))

    def fit_binary(self, flux, eflux, start_a, start_b, ratio=0.3, tie=(), fit_vrad=True, npoly=0, coef=None, bounds=None, ratio_bounds=(0.01, 0.99),
                   vrad_step=0.25, check_every=4, timing=False, **opts):
        """A double-lined binary: two emulated spectra fitted to one observation in ONE Levenberg-Marquardt fit of
        chi^2 = sum w (flux - p(x) [(1 - q) m_A + q m_B])^2.  m_A and m_B are ``fit``'s model, each at its own labels, Vrad, Vrot and
        Inst_R (``start_a``, ``start_b`` [N, 8], getspec's columns; Vrot and Inst_R stay fixed there); q is the light ratio, started at
        ``ratio`` (a number or [N]) inside ``ratio_bounds``; p is ``fit_joint``'s Chebyshev series of ``npoly`` coefficients (0: p = 1),
        started from ``coef`` [N, npoly] or from one ``ContinuumFit.fit`` against the mixed model at the start.  ``tie``: labels the two
        components share (``('feh', 'afe')``: a binary has one composition) -- one parameter that both see.  The parameters, in this
        order: A's labels and Vrad, B's that are not tied, q, the coefficients; K <= 15.  ``bounds``: {name of ``labels``: (lo, hi)}.

        An iteration is four enqueued steps and no host look: payne_specjac_eval at both components' trial labels (a tied label is
        gathered from A's on the device), the broadening of both row sets (Vrad rows by central difference, as ``fit``'s), and
        payne_lmfit_update_pair, which mixes the two components' rows in registers.

        Returns a dict: ``pars_a``, ``pars_b`` [N, 8], ``ratio`` [N], ``coef`` [N, npoly], ``chisq``, ``npix``, ``fisher`` [N, K, K],
        ``err`` [N, K] = sqrt(diag(inv(fisher))) -- every error is marginalised over the other component, q and the polynomial --
        ``status``, ``niter``, ``at_bound`` and ``labels`` (Teff_a .. Vrad_a, Teff_b .., ratio, pc_0 ..; a tied label once, under its A
        name).  A star whose first chi^2 is not finite, or whose starting continuum fit fails, has status NAN and NaN results.

        What to keep in mind.  Swapping A and B with q -> 1 - q is the same model: which component comes out as A is decided by the
        start.  A ratio that is constant in wavelength is an approximation for a narrow range.  The evidence for a binary is ``chisq``
        against ``fit_joint``'s (or ``fit``'s) on the same pixels, not anything this fit reports by itself.  The starting points are the
        caller's (``fit_binary_from_bank`` takes them from a bank's pair search); two components started at the same labels and Vrad
        have identical rows, which ends ``SINGULAR``."""
        Pr = self.predictor
        anns, eng, D = Pr.anns, Pr.anns.engine, self.n_labels
        a = check_binary_args(flux, eflux, start_a, start_b, len(self.obs_wave), D, anns.xmin, anns.xmax, ratio=ratio, tie=tie, fit_vrad=fit_vrad, npoly=npoly,
                              coef=coef, bounds=bounds, ratio_bounds=ratio_bounds, vrad_step=vrad_step, check_every=check_every, **opts)
        from .contfit import abscissa
        torch, dev = eng.torch, eng.device
        flux, eflux, start_a, start_b, q0, coef, o = a["flux"], a["eflux"], a["start_a"], a["start_b"], a["ratio"], a["coef"], a["opts"]
        cols, Ka, Kl, P, b_pos = a["cols"], a["Ka"], a["Kl"], a["P"], a["b_pos"]
        N = flux.shape[0]
        start_b = start_b.copy()
        tied = [k for k in range(Ka) if b_pos[k] < Ka]
        free_b = [k for k in range(Ka) if b_pos[k] >= Ka]
        start_b[:, [cols[k] for k in tied]] = start_a[:, [cols[k] for k in tied]]
        w = weights_from_errors(eflux)
        cont_status = np.full(N, _lib.CONTFIT_OK, dtype=np.int32)
        if P and coef is None:
            q_d = torch.as_tensor(q0).to(dev)[:, None]
            mixed = ((1.0 - q_d) * self.model_spectra(start_a) + q_d * self.model_spectra(start_b)).to(torch.float32).contiguous()
            coef, cont_status, w = self._start_continuum(flux, eflux, mixed, P, None, w)
        out = dict(pars_a=start_a.copy(), pars_b=start_b.copy(), ratio=np.full(N, np.nan), coef=np.full((N, P), np.nan), npix=(w != 0.0).sum(axis=1),
                   labels=list(a["names"]), **empty_results(N, Kl + 1 + P))
        out["pars_a"][:, cols] = np.nan
        out["pars_b"][:, cols] = np.nan
        x_d = torch.as_tensor(abscissa(self.obs_wave)).to(dev) if P else None
        b_lab = torch.as_tensor(b_pos[:D]).to(dev)                    # where B's labels sit in x_trial: a tied one is A's

        def block(handle, idx):
            nb = len(idx)
            x0 = np.concatenate([start_a[idx][:, cols], start_b[idx][:, [cols[k] for k in free_b]], q0[idx, None]]
                                + ([np.ascontiguousarray(coef[idx], dtype=np.float64)] if P else []), axis=1)

            def update(rows, flux_d, w_d, mark):
                handle.update_pair(rows[:nb], rows[nb:], flux_d, w_d, a["ia"], a["ib"], P, x_d)
            return x0, np.concatenate([start_a[idx], start_b[idx]]), update

        def place(idx, xb):
            out["pars_a"][idx[:, None], np.asarray(cols)[None, :]] = xb[:, :Ka]
            out["pars_b"][idx[:, None], np.asarray(cols)[None, :]] = xb[:, b_pos]
            out["ratio"][idx] = xb[:, Kl]
            out["coef"][idx] = xb[:, Kl + 1:]

        def labels_of(xt):
            return torch.cat([xt[:, :D], xt.index_select(1, b_lab)], dim=0)

        def vrad_of(xt):
            return torch.cat([xt[:, D], xt[:, int(b_pos[D])]])
        # the theta blocks and the rows hold A's stars, then B's; a block's size counts both components
        return self._fit_blocks(out, self._with_continuum(cont_status), flux, w, a["lo"], a["hi"], o, block, place, cols=cols, fit_vrad=fit_vrad,
                                vrad_step=vrad_step, check_every=check_every, timing=timing, nc=2, labels_of=labels_of, vrad_of=vrad_of, nan_results=True)

    def fit_binary_from_bank(self, flux, eflux, bank, topk=1, primaries=4, **fit_binary_kwargs):
        """``fit_binary`` started from the ``topk`` pairs of templates of ``bank`` that fit each star best with both amplitudes free
        (``bank.match_pairs(topk=topk, primaries=primaries)``): per rank the pair's theta rows are ``start_a`` and ``start_b`` (A the
        brighter), its light ratio, clipped into ``ratio_bounds``, is ``ratio``, and with ``npoly`` >= 1 the starting ``coef`` is
        (the pair's scale, 0, ...).  ``fit_from_bank``'s logic otherwise: one ``fit_binary`` call per rank over the stars that have
        a pair of that rank; per star the result of lowest chi^2 among those whose status is not NAN / SINGULAR is kept, the lower
        rank on a tie (rank 0's if none qualifies).  Returns ``fit_binary``'s dict plus ``start_index_a``, ``start_index_b`` (the
        templates), ``start_chisq`` (the pair's chi^2 in the search), ``start_rank`` and ``single_chisq`` (the best
        one-template-and-scale chi^2 of the same pixels: what ``chisq`` has to beat for the star to count as a binary).  A star
        without a pair keeps status NAN, NaN parameters and ``start_index_a`` -1.  ``fit_binary_kwargs`` go to ``fit_binary``; with
        ``npoly`` = 0 the model has no scale, so the spectra must be normalised."""
        flux, eflux = self._bank_inputs(flux, eflux, bank, "match_pairs", fit_binary_kwargs, ("start_a", "start_b", "ratio", "coef"),
                                        "fit_binary_from_bank takes its starts, ratio and coefficients from the bank")
        N = flux.shape[0]
        kw = dict(fit_binary_kwargs)
        rb = kw.get("ratio_bounds", (0.01, 0.99))
        P = int(kw.get("npoly", 0))
        probe = np.zeros((N, 8))                                     # (what does not depend on the starts is checked before the search)
        a = check_binary_args(flux, eflux, probe, probe, len(self.obs_wave), self.n_labels, self.predictor.anns.xmin, self.predictor.anns.xmax,
                              ratio=0.5 * (rb[0] + rb[1]), **kw)
        K = a["Kl"] + 1 + P
        m = bank.match_pairs(flux, eflux, topk=topk, primaries=primaries)
        out = dict(pars_a=np.full((N, 8), np.nan), pars_b=np.full((N, 8), np.nan), ratio=np.full(N, np.nan), coef=np.full((N, P), np.nan), npix=m["npix"],
                   labels=list(a["names"]), start_index_a=np.full(N, -1, dtype=np.int32), start_index_b=np.full(N, -1, dtype=np.int32),
                   single_chisq=m["single_chisq"], **self._bank_results(N, K))

        def fit_rank(sel, r):
            if P:
                kw["coef"] = np.concatenate([m["scale"][sel, r][:, None], np.zeros((len(sel), P - 1))], axis=1)
            return self.fit_binary(flux[sel], eflux[sel], m["pars_a"][sel, r], m["pars_b"][sel, r], ratio=np.clip(m["ratio"][sel, r], rb[0], rb[1]), **kw)

        def record(dst, r):
            out["start_index_a"][dst], out["start_index_b"][dst], out["start_chisq"][dst] = m["index_a"][dst, r], m["index_b"][dst, r], m["chisq"][dst, r]
        return keep_best_rank(m["index_a"], out, ("pars_a", "pars_b", "ratio", "coef", "chisq", "fisher", "status", "niter", "at_bound", "err"), fit_rank, record)

    def fit_joint_from_bank(self, flux, eflux, bank, npoly=4, topk=1, **fit_joint_kwargs):
        """``fit_joint`` started from the ``topk`` templates of ``bank`` that match each star best under a free continuum
        polynomial (``bank.match(npoly=npoly)``): per rank the template's parameters are the start and the match's coefficients
        the starting ``coef``.  ``fit_from_bank``'s logic otherwise: one ``fit_joint`` call per rank over the stars that have a
        template of that rank; per star the result of lowest chi^2 among those whose status is not NAN / SINGULAR is kept, the lower
        rank on a tie (rank 0's if none qualifies).  Returns ``fit_joint``'s dict plus ``start_index``, ``start_chisq`` and
        ``start_rank``; a star that no template matches keeps status NAN, NaN ``pars`` and ``start_index`` -1.
        ``fit_joint_kwargs`` go to ``fit_joint``."""
        flux, eflux = self._bank_inputs(flux, eflux, bank, "match", fit_joint_kwargs, ("start", "coef"),
                                        "fit_joint_from_bank takes its starts and coefficients from the bank")
        if isinstance(npoly, bool) or int(npoly) != npoly or not (1 <= int(npoly) <= _lib.TMATCH_MAX_POLY):
            raise ValueError("npoly must be 1 .. %d, got %r" % (_lib.TMATCH_MAX_POLY, npoly))
        P = int(npoly)
        m = bank.match(flux, eflux, topk=topk, npoly=P)
        N = m["index"].shape[0]
        labels = self.labels(bool(fit_joint_kwargs.get("fit_vrad", False))) + ["pc_%d" % j for j in range(P)]
        out = dict(pars=np.full((N, 8), np.nan), npix=m["npix"], labels=labels, coef=np.full((N, P), np.nan), cont_status=np.full(N, _lib.CONTFIT_OK, dtype=np.int32),
                   start_index=np.full(N, -1, dtype=np.int32), **self._bank_results(N, len(labels)))

        def record(dst, r):
            out["start_index"][dst], out["start_chisq"][dst] = m["index"][dst, r], m["chisq"][dst, r]
        return keep_best_rank(m["index"], out, ("pars", "chisq", "npix", "fisher", "status", "niter", "at_bound", "err", "coef", "cont_status"),
                              lambda sel, r: self.fit_joint(flux[sel], eflux[sel], m["pars"][sel, r], npoly=P, coef=m["coef"][sel, r], **fit_joint_kwargs), record)
