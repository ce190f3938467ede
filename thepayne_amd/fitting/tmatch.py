"""Brute-force chi^2 of many spectra against a bank of templates on the GPU: starting points for ``OptFit``.

``TemplateBank`` holds M model spectra on one observed grid (a lattice of labels times a grid of velocities, or any theta the caller
lists), made by the engine's own forward pass.  ``match`` gives, per star, the ``topk`` templates of lowest
chi^2 = sum_p w_p (flux_p - template_p)^2 with their chi^2 and parameters.  The N x M chi^2 are one matrix product over 2 n terms on
the fp64 matrix instruction (payne_tmatch_match; include/payne_hip.h states the rules): the three terms of the expanded square are
~1e4 times their sum at S/N 100, so the sums are fp64 throughout and the result is within (2 n + 4) 2^-53 of the terms' magnitudes.

``match(npoly=P)`` minimises a continuum polynomial of P <= 8 Chebyshev coefficients (``polycalc``'s basis and abscissa) out of
every (star, template) pair, chi^2 = min_c sum_p w_p (flux_p - template_p sum_j c_j T_j(x_p))^2: the chi^2 of ``ContinuumFit`` and
``OptFit.fit_joint``, so flux-calibrated or blaze-shaped spectra enter the pipeline here (payne_tmatch_match_poly: 3 P - 1 matrix
products, a scaled Cholesky solve per pair).  Its dict goes to ``ContinuumFit.fit_to_bank(match=)`` as it is, and
``OptFit.fit_joint_from_bank`` starts the joint fit from the best few with their coefficients.

``match_pairs`` searches PAIRS of templates with both amplitudes free, chi^2 = min sum_p w_p (flux_p - alpha m_a - beta m_b)^2: the
starting points of ``OptFit.fit_binary`` (payne_tmatch_match_pairs: the moments and a cross term per (star, primary) as matrix
products, a 2 x 2 solve per pair); ``OptFit.fit_binary_from_bank`` starts the two-component fit from the best few.

No interpolation between the lattice's nodes: the best template is a start for a fit, not a measurement.
``OptFit.fit_from_bank`` runs the fit from the best few.
"""
import ctypes as C
import itertools

import numpy as np

from .. import _lib
from ..engine import THETA_SPEC_COLS
from ..predict._spec import PayneSpecPredict
from .forecast import weights_from_errors

__all__ = ["TemplateBank", "TMatchHandle", "lattice_theta", "check_match_args", "check_npoly", "check_pair_args", "PAIR_WORKSPACE_BYTES"]

PAIR_WORKSPACE_BYTES = 256 * 1024 * 1024             # ``match_pairs`` walks the stars in blocks whose moments stay below this


def lattice_theta(xmin, xmax, steps, vrad=(0.0,), vrot=(5.0,), inst_R=(np.nan,), inner=(0.0, 1.0)):
    """theta [M, 8] (getspec's columns): the cell centres of a lattice of ``steps`` cells per label (an int, or one per label) over
    the part ``inner`` = (a, b) of the box [xmin, xmax] (fractions of its width), times the listed Vrad, Vrot and Inst_R.  The first
    label varies slowest, Inst_R fastest.  A fifth label is Vmic (column 6); a four-label network's Vmic is NaN (absent), as is an
    Inst_R of NaN (no instrumental broadening)."""
    xmin, xmax = np.asarray(xmin, dtype=np.float64), np.asarray(xmax, dtype=np.float64)
    D = len(xmin)
    if D not in (4, 5) or xmax.shape != xmin.shape:
        raise ValueError("xmin and xmax must hold 4 or 5 labels")
    st = np.full(D, steps, dtype=np.int64) if np.ndim(steps) == 0 else np.asarray(steps, dtype=np.int64)
    if st.shape != (D,) or np.any(st < 1):
        raise ValueError("steps must be a positive int or one per label (%d)" % D)
    a, b = float(inner[0]), float(inner[1])
    if not (0.0 <= a < b <= 1.0):
        raise ValueError("inner = (a, b) with 0 <= a < b <= 1")
    vrad, vrot, inst_R = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (vrad, vrot, inst_R))
    if min(len(vrad), len(vrot), len(inst_R)) < 1 or not (np.all(np.isfinite(vrad)) and np.all(np.isfinite(vrot))):
        raise ValueError("vrad, vrot and inst_R must each list at least one value; Vrad and Vrot finite")
    lo, span = xmin + a * (xmax - xmin), (b - a) * (xmax - xmin)
    axes = [lo[d] + (np.arange(st[d]) + 0.5) / st[d] * span[d] for d in range(D)] + [vrad, vrot, inst_R]
    grid = np.array(list(itertools.product(*axes)), dtype=np.float64)
    theta = np.full((len(grid), 8), np.nan)
    theta[:, 0:4] = grid[:, 0:4]
    if D == 5:
        theta[:, 6] = grid[:, 4]
    theta[:, 4], theta[:, 5], theta[:, 7] = grid[:, D], grid[:, D + 1], grid[:, D + 2]
    return theta


def check_match_args(flux, eflux, nobs, topk):
    """What ``TemplateBank.match`` checks of host arrays before anything reaches the device: (flux [N, nobs] fp32, w [N, nobs] fp64).
    w = 1 / eflux^2 (``weights_from_errors``), and 0 where the flux is not finite."""
    if not (1 <= int(topk) <= _lib.TMATCH_MAX_TOPK):
        raise ValueError("topk must be 1 .. %d, got %r" % (_lib.TMATCH_MAX_TOPK, topk))
    flux = np.atleast_2d(np.asarray(flux, dtype=np.float32))
    eflux = np.atleast_2d(np.asarray(eflux, dtype=np.float64))
    if flux.ndim != 2 or flux.shape[1] != nobs:
        raise ValueError("flux must be [N, %d], got %s" % (nobs, flux.shape))
    if eflux.shape != flux.shape:
        raise ValueError("eflux %s and flux %s differ in shape" % (eflux.shape, flux.shape))
    w = weights_from_errors(eflux)
    w[~np.isfinite(flux)] = 0.0
    return flux, w


def check_npoly(npoly):
    """``match``'s npoly: 0 (the template as it is) or the 1 .. 8 Chebyshev coefficients minimised out of every pair."""
    if isinstance(npoly, bool) or int(npoly) != npoly or not (0 <= int(npoly) <= _lib.TMATCH_MAX_POLY):
        raise ValueError("npoly must be 0 .. %d, got %r" % (_lib.TMATCH_MAX_POLY, npoly))
    return int(npoly)


def check_pair_args(topk, primaries, M, shortlist=None, N=None):
    """What ``TemplateBank.match_pairs`` checks of its own arguments: (topk, primaries, shortlist int32 [N, primaries] or None).  In a
    shortlist an index outside 0 .. M - 1 becomes -1 (an unused slot), and so does a template that an earlier slot of the same star
    names already: the device is never handed a primary twice."""
    if isinstance(topk, bool) or int(topk) != topk or not (1 <= int(topk) <= _lib.TMATCH_MAX_TOPK):
        raise ValueError("topk must be 1 .. %d, got %r" % (_lib.TMATCH_MAX_TOPK, topk))
    if isinstance(primaries, bool) or int(primaries) != primaries or not (1 <= int(primaries) <= _lib.TMATCH_MAX_PRIMARIES):
        raise ValueError("primaries must be 1 .. %d, got %r" % (_lib.TMATCH_MAX_PRIMARIES, primaries))
    k, kA = int(topk), int(primaries)
    if shortlist is None:
        if kA > _lib.TMATCH_MAX_TOPK:
            raise ValueError("primaries above %d need a shortlist: the single-template search lists at most %d" % (_lib.TMATCH_MAX_TOPK, _lib.TMATCH_MAX_TOPK))
        return k, kA, None
    raw = np.asarray(shortlist.cpu() if hasattr(shortlist, "cpu") else shortlist)
    if raw.dtype.kind not in "iu":
        raise ValueError("shortlist must hold integers (template indices, -1: an unused slot)")
    if raw.ndim == 1 and N in (None, 1):
        raw = raw[None, :]
    if raw.ndim != 2 or raw.shape[1] != kA or (N is not None and raw.shape[0] != N):
        raise ValueError("shortlist must be [%s, %d], got %s" % ("N" if N is None else N, kA, raw.shape))
    raw = raw.astype(np.int64)
    sl = np.where((raw >= 0) & (raw < M), raw, -1).astype(np.int32)
    for j in range(1, kA):
        sl[(sl[:, j:j + 1] == sl[:, :j]).any(axis=1), j] = -1
    return k, kA, sl


class TMatchHandle(object):
    """Owner of one ``payne_tmatch`` handle (its workspace of partial lists): at most ``max_stars`` x ``max_templates`` a call.
    ``max_poly`` > 0: the handle also holds ``match_poly``'s workspace for up to that many coefficients.  ``max_primaries`` > 0 (with
    ``max_poly`` = 0): it holds ``match_pairs``' workspace, the moments and the lists of ``max_stars * max_primaries`` rows."""

    def __init__(self, max_stars, max_templates, device, max_poly=0, max_primaries=0):
        import torch
        self.torch, self.lib = torch, _lib.load()
        self.device, self.max_stars, self.max_templates, self.max_poly = device, int(max_stars), int(max_templates), check_npoly(max_poly)
        if isinstance(max_primaries, bool) or int(max_primaries) != max_primaries or not (0 <= int(max_primaries) <= _lib.TMATCH_MAX_PRIMARIES):
            raise ValueError("max_primaries must be 0 .. %d, got %r" % (_lib.TMATCH_MAX_PRIMARIES, max_primaries))
        self.max_primaries = int(max_primaries)
        if self.max_poly and self.max_primaries:
            raise ValueError("a handle holds the polynomial's workspace or the pairs', not both")
        self._h = C.c_void_p()
        if self.max_primaries:
            rc = self.lib.payne_tmatch_create_pairs(self.device.index, self.max_stars, self.max_templates, self.max_primaries, C.byref(self._h))
        elif self.max_poly:
            rc = self.lib.payne_tmatch_create_poly(self.device.index, self.max_stars, self.max_templates, self.max_poly, C.byref(self._h))
        else:
            rc = self.lib.payne_tmatch_create(self.device.index, self.max_stars, self.max_templates, C.byref(self._h))
        if rc != 0:
            raise RuntimeError("payne_tmatch_create failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))

    def match(self, templates, flux, w, topk, n=None, return_all=False):
        """templates fp32 [M, ld_t], flux fp32 [N, ld_f], w fp64 [N, ld_f]: device tensors whose rows are contiguous; n pixels (the
        smaller of the two row lengths by default) -> (idx int32 [N, topk], chisq fp64 [N, topk], all fp64 [N, M] or None)."""
        torch = self.torch
        if templates.dtype != torch.float32 or flux.dtype != torch.float32 or w.dtype != torch.float64:
            raise ValueError("templates and flux fp32, w fp64")
        if templates.dim() != 2 or flux.dim() != 2 or tuple(w.shape) != tuple(flux.shape):
            raise ValueError("templates [M, ld_t], flux and w [N, ld_f]; got %s, %s, %s" % (tuple(templates.shape), tuple(flux.shape), tuple(w.shape)))
        if not (templates.is_contiguous() and flux.is_contiguous() and w.is_contiguous()):
            raise ValueError("templates, flux and w must be contiguous")
        M, N = templates.shape[0], flux.shape[0]
        n = min(templates.shape[1], flux.shape[1]) if n is None else int(n)
        idx = torch.empty((N, topk), dtype=torch.int32, device=self.device)
        chisq = torch.empty((N, topk), dtype=torch.float64, device=self.device)
        every = torch.empty((N, M), dtype=torch.float64, device=self.device) if return_all else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self.lib.payne_tmatch_match(self._h, templates.data_ptr(), templates.shape[1], M, flux.data_ptr(), w.data_ptr(), flux.shape[1], N, n,
                                         int(topk), idx.data_ptr(), chisq.data_ptr(), every.data_ptr() if return_all else None, M, stream)
        if rc != 0:
            raise RuntimeError("payne_tmatch_match failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))
        return idx, chisq, every

    def match_poly(self, templates, flux, w, x, npoly, topk, n=None, return_all=False):
        """``match`` with ``npoly`` coefficients minimised out of every pair; x fp64 [n] on the device (``contfit.abscissa``) ->
        (idx, chisq, coef fp64 [N, topk, npoly], flags int32 [N, topk], all or None)."""
        torch = self.torch
        if templates.dtype != torch.float32 or flux.dtype != torch.float32 or w.dtype != torch.float64 or x.dtype != torch.float64:
            raise ValueError("templates and flux fp32, w and x fp64")
        if templates.dim() != 2 or flux.dim() != 2 or tuple(w.shape) != tuple(flux.shape) or x.dim() != 1:
            raise ValueError("templates [M, ld_t], flux and w [N, ld_f], x [n]; got %s, %s, %s, %s"
                             % (tuple(templates.shape), tuple(flux.shape), tuple(w.shape), tuple(x.shape)))
        if not (templates.is_contiguous() and flux.is_contiguous() and w.is_contiguous() and x.is_contiguous()):
            raise ValueError("templates, flux, w and x must be contiguous")
        M, N, P = templates.shape[0], flux.shape[0], int(npoly)
        n = min(templates.shape[1], flux.shape[1]) if n is None else int(n)
        if x.shape[0] < n:
            raise ValueError("x holds %d abscissae for %d pixels" % (x.shape[0], n))
        idx = torch.empty((N, topk), dtype=torch.int32, device=self.device)
        chisq = torch.empty((N, topk), dtype=torch.float64, device=self.device)
        coef = torch.empty((N, topk, max(P, 1)), dtype=torch.float64, device=self.device)
        flags = torch.empty((N, topk), dtype=torch.int32, device=self.device)
        every = torch.empty((N, M), dtype=torch.float64, device=self.device) if return_all else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self.lib.payne_tmatch_match_poly(self._h, templates.data_ptr(), templates.shape[1], M, flux.data_ptr(), w.data_ptr(), flux.shape[1], N, n,
                                              x.data_ptr(), P, int(topk), idx.data_ptr(), chisq.data_ptr(), coef.data_ptr(), flags.data_ptr(),
                                              every.data_ptr() if return_all else None, M, stream)
        if rc != 0:
            raise RuntimeError("payne_tmatch_match_poly failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))
        return idx, chisq, coef, flags, every

    def match_pairs(self, templates, flux, w, cand, topk, n=None, return_all=False):
        """``match`` against pairs of templates: cand int32 [N, kA] on the device names each star's primaries (-1: an unused slot) ->
        (idx_a, idx_b int32 [N, topk] template indices, chisq fp64 [N, topk], amp fp64 [N, topk, 2] = (alpha, beta), all fp64
        [N, kA, M] or None)."""
        torch = self.torch
        if templates.dtype != torch.float32 or flux.dtype != torch.float32 or w.dtype != torch.float64 or cand.dtype != torch.int32:
            raise ValueError("templates and flux fp32, w fp64, cand int32")
        if templates.dim() != 2 or flux.dim() != 2 or tuple(w.shape) != tuple(flux.shape) or cand.dim() != 2 or cand.shape[0] != flux.shape[0]:
            raise ValueError("templates [M, ld_t], flux and w [N, ld_f], cand [N, kA]; got %s, %s, %s, %s"
                             % (tuple(templates.shape), tuple(flux.shape), tuple(w.shape), tuple(cand.shape)))
        if not (templates.is_contiguous() and flux.is_contiguous() and w.is_contiguous() and cand.is_contiguous()):
            raise ValueError("templates, flux, w and cand must be contiguous")
        M, N, kA = templates.shape[0], flux.shape[0], cand.shape[1]
        n = min(templates.shape[1], flux.shape[1]) if n is None else int(n)
        idx_a = torch.empty((N, topk), dtype=torch.int32, device=self.device)
        idx_b = torch.empty((N, topk), dtype=torch.int32, device=self.device)
        chisq = torch.empty((N, topk), dtype=torch.float64, device=self.device)
        amp = torch.empty((N, topk, 2), dtype=torch.float64, device=self.device)
        every = torch.empty((N, kA, M), dtype=torch.float64, device=self.device) if return_all else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self.lib.payne_tmatch_match_pairs(self._h, templates.data_ptr(), templates.shape[1], M, flux.data_ptr(), w.data_ptr(), flux.shape[1], N, n,
                                               cand.data_ptr(), kA, int(topk), idx_a.data_ptr(), idx_b.data_ptr(), chisq.data_ptr(), amp.data_ptr(),
                                               every.data_ptr() if return_all else None, M, stream)
        if rc != 0:
            raise RuntimeError("payne_tmatch_match_pairs failed (%d): %s" % (rc, self.lib.payne_last_error(None).decode()))
        return idx_a, idx_b, chisq, amp, every

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.payne_tmatch_destroy(self._h)                  # (waits for the device)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TemplateBank(object):
    """TemplateBank(specANNpath, NNtype, obs_wave): templates on the observed grid ``obs_wave`` and the chi^2 search against them.
    ``max_stars``: stars per call of the device search (``match`` walks more in blocks)."""

    def __init__(self, specANNpath, NNtype, obs_wave, device=None, b_max=256, max_stars=4096):
        self.obs_wave = np.ascontiguousarray(obs_wave, dtype=np.float64)
        if self.obs_wave.ndim != 1 or len(self.obs_wave) < 1:
            raise ValueError("obs_wave must be a vector")
        if int(max_stars) < 1:
            raise ValueError("max_stars must be at least 1")
        self.predictor = PayneSpecPredict(specANNpath, NNtype=NNtype, device=device, b_max=b_max)
        self.n_labels = self.predictor.anns.n_labels
        self.max_stars = int(max_stars)
        self.theta, self.templates, self._handle, self._pair_handle = None, None, None, None

    def lattice(self, steps, vrad=(0.0,), vrot=(5.0,), inst_R=(np.nan,), inner=(0.0, 1.0)):
        """``build`` on ``lattice_theta`` of the network's box; returns self."""
        anns = self.predictor.anns
        return self.build(lattice_theta(anns.xmin[:self.n_labels], anns.xmax[:self.n_labels], steps, vrad=vrad, vrot=vrot, inst_R=inst_R, inner=inner))

    def build(self, theta):
        """theta [M, 8] (getspec's columns, any Vrad / Vrot / Inst_R per template) -> the templates, ``predict_batch(theta, stage=2)``
        in the engine's blocks, as one fp32 device tensor [M, nobs]; returns self."""
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        if theta.ndim != 2 or theta.shape[1] != 8 or theta.shape[0] < 1:
            raise ValueError("theta must be [M, 8] (%s), got %s" % (", ".join(THETA_SPEC_COLS), theta.shape))
        P = self.predictor
        eng = P.anns.engine
        P._bind(self.obs_wave)
        M, step = theta.shape[0], eng.b_max
        out = eng.torch.empty((M, len(self.obs_wave)), dtype=eng.torch.float32, device=eng.device)
        for s in range(0, M, step):
            th = np.full((min(step, M - s), eng.ncols), np.nan)
            th[:, :8] = theta[s:s + step]
            out[s:s + step] = eng.predict_batch(th, stage=2)
        self.close()
        self.theta, self.templates = theta.copy(), out
        return self

    def __len__(self):
        return 0 if self.theta is None else len(self.theta)

    def _device_inputs(self, flux, eflux, topk):
        """(flux fp32 [N, nobs], w fp64 [N, nobs]) on the device from host arrays or device tensors, as ``match`` states."""
        eng = self.predictor.anns.engine
        torch, dev, nobs = eng.torch, eng.device, len(self.obs_wave)
        if isinstance(flux, torch.Tensor) or isinstance(eflux, torch.Tensor):
            if not (1 <= int(topk) <= _lib.TMATCH_MAX_TOPK):
                raise ValueError("topk must be 1 .. %d, got %r" % (_lib.TMATCH_MAX_TOPK, topk))
            f = torch.as_tensor(flux).to(device=dev, dtype=torch.float32).reshape(-1, nobs).contiguous()
            e = torch.as_tensor(eflux).to(device=dev, dtype=torch.float64)
            if tuple(e.shape) != tuple(f.shape):
                raise ValueError("eflux %s and flux %s differ in shape" % (tuple(e.shape), tuple(f.shape)))
            ok = torch.isfinite(e) & (e != 0.0) & torch.isfinite(f)
            w = torch.where(ok, 1.0 / (e * e), torch.zeros_like(e)).contiguous()
        else:
            fh, wh = check_match_args(flux, eflux, nobs, topk)
            f, w = torch.as_tensor(fh).to(dev), torch.as_tensor(wh).to(dev)
        return f, w

    def match(self, flux, eflux, topk=1, return_all=False, npoly=0):
        """flux, eflux [N, nobs] on ``obs_wave`` (host arrays or device tensors; eflux zero or not finite, or a flux that is not
        finite: the pixel does not count) -> dict: ``index`` int32 [N, topk] (-1: no such template), ``chisq`` [N, topk] ascending
        (+inf there), ``pars`` [N, topk, 8] the bank's theta rows (NaN there), ``npix`` (pixels with w != 0) and, with
        ``return_all``, ``all`` [N, M].  Equal chi^2 are listed in ascending template index; a NaN chi^2 is never listed.

        ``npoly`` = P >= 1: chi^2 is minimised over a continuum polynomial of P Chebyshev coefficients per (star, template) pair
        (``polycalc``'s basis on ``contfit.abscissa(obs_wave)``), and the dict gains ``coef`` [N, topk, P] (NaN where index is -1),
        ``positive`` bool [N, topk] (the polynomial is > 0 at every counting pixel; a template whose polynomial turns negative stays
        listed) and ``npoly``.  A star with fewer than P counting pixels, and a template that is zero at all of them, give NaN:
        a star without a counting pixel lists nothing, where ``npoly=0`` lists chi^2 = 0 for it."""
        P = check_npoly(npoly)
        if self.templates is None:
            raise RuntimeError("the bank is empty: call build(theta) or lattice(steps, ...) first")
        eng = self.predictor.anns.engine
        torch, dev, nobs = eng.torch, eng.device, len(self.obs_wave)
        f, w = self._device_inputs(flux, eflux, topk)
        N, M, k = f.shape[0], len(self), int(topk)
        if self._handle is not None and P > self._handle.max_poly:
            self.close()                                             # (the workspace grows only once a polynomial is asked for)
        if self._handle is None:
            self._handle = TMatchHandle(self.max_stars, M, dev, max_poly=_lib.TMATCH_MAX_POLY if P else 0)
        index = np.empty((N, k), dtype=np.int32)
        chisq = np.empty((N, k))
        every = np.empty((N, M)) if return_all else None
        if P:
            from .contfit import abscissa
            x = torch.as_tensor(abscissa(self.obs_wave)).to(dev)
            coef, flags = np.empty((N, k, P)), np.empty((N, k), dtype=np.int32)
        for s in range(0, N, self.max_stars):
            e_ = min(N, s + self.max_stars)
            if P:
                i_d, c_d, k_d, f_d, a_d = self._handle.match_poly(self.templates, f[s:e_], w[s:e_], x, P, k, n=nobs, return_all=return_all)
                coef[s:e_], flags[s:e_] = k_d.cpu().numpy(), f_d.cpu().numpy()
            else:
                i_d, c_d, a_d = self._handle.match(self.templates, f[s:e_], w[s:e_], k, n=nobs, return_all=return_all)
            index[s:e_], chisq[s:e_] = i_d.cpu().numpy(), c_d.cpu().numpy()
            if return_all:
                every[s:e_] = a_d.cpu().numpy()
        pars = np.where((index >= 0)[:, :, None], self.theta[np.maximum(index, 0)], np.nan)
        out = dict(index=index, chisq=chisq, pars=pars, npix=(w != 0.0).sum(dim=1).cpu().numpy())
        if P:
            out.update(coef=coef, positive=(flags & 1) != 0, npoly=P)
        if return_all:
            out["all"] = every
        return out

    def match_pairs(self, flux, eflux, topk=1, primaries=4, shortlist=None, return_all=False):
        """The ``topk`` PAIRS of templates (a, b) that fit each star best with both amplitudes free,
        chi^2 = min over (alpha, beta) of sum_p w_p (flux_p - alpha m_a - beta m_b)^2: starting points for ``OptFit.fit_binary``
        (``OptFit.fit_binary_from_bank`` runs it from them).  flux, eflux as ``match``'s.  The primary a runs over ``primaries`` <= 16
        templates per star, the secondary b over the whole bank.  ``shortlist`` int [N, primaries] names each star's primaries; by
        default it is ``match(topk=primaries, npoly=1)['index']``, the single templates that fit best with a free scale
        (``primaries`` <= 8 then), whose -1 slots are passed through.  In a shortlist of the caller's an index outside the bank and
        a template named twice for one star become -1.

        Returns a dict: ``index_a``, ``index_b`` int32 [N, topk] (-1: no such pair), ``chisq`` [N, topk] ascending (+inf there),
        ``scale`` = alpha + beta and ``ratio`` = beta / (alpha + beta) [N, topk] (NaN there) -- ``fit_binary``'s ``coef[:, 0]`` and
        ``ratio`` --, ``pars_a``, ``pars_b`` [N, topk, 8] the bank's theta rows, ``npix``, ``shortlist`` [N, primaries] as searched,
        ``single_chisq`` [N], the best one-template-and-scale chi^2 of the same pixels (what a binary's chi^2 is compared with; +inf
        if no template fits), and with ``return_all`` ``all`` [N, primaries, M], every pair's chi^2 (row j: primary
        ``shortlist[:, j]``).  THE HOST ORDERS EACH LISTED PAIR SO THAT A IS THE BRIGHTER: ``ratio`` <= 0.5, whichever of the two the
        shortlist held; the order of the list, ascending in (chi^2, slot of the shortlist, index of the other template), is the
        device's.

        A pair is left out (NaN in ``all``): the same template twice; a template that is not finite at a counting pixel; two
        templates that are collinear over the star's pixels (1 - cos^2 <= 2^-20); a fit with an amplitude that is not positive (one
        template fits as well); a pair that an earlier slot of the shortlist lists already.  A star without a counting pixel lists
        nothing.  No continuum polynomial beyond the constant scale.

        The stars are walked in blocks sized so that the moments' workspace on the device (16 bytes per star and template) stays
        under 256 MB, and never more than ``max_stars`` at a time."""
        if self.templates is None:
            raise RuntimeError("the bank is empty: call build(theta) or lattice(steps, ...) first")
        M = len(self)
        k, kA, sl = check_pair_args(topk, primaries, M, shortlist)
        eng = self.predictor.anns.engine
        torch, dev, nobs = eng.torch, eng.device, len(self.obs_wave)
        f, w = self._device_inputs(flux, eflux, k)
        N = f.shape[0]
        single = self.match(flux, eflux, topk=kA if sl is None else 1, npoly=1)
        if sl is None:
            sl = np.ascontiguousarray(single["index"], dtype=np.int32)
        elif sl.shape[0] != N:
            raise ValueError("shortlist must be [%d, %d], got %s" % (N, kA, sl.shape))
        block = int(max(1, min(self.max_stars, PAIR_WORKSPACE_BYTES // (16 * M))))
        h = self._pair_handle
        if h is not None and (h.max_primaries < kA or h.max_stars < min(block, N) or h.max_templates != M):
            h.close()
            h = self._pair_handle = None
        if h is None:
            h = self._pair_handle = TMatchHandle(block, M, dev, max_primaries=kA)
        idx_a, idx_b = np.empty((N, k), dtype=np.int32), np.empty((N, k), dtype=np.int32)
        chisq, amp = np.empty((N, k)), np.empty((N, k, 2))
        every = np.empty((N, kA, M)) if return_all else None
        cand = torch.as_tensor(sl).to(dev)
        for s in range(0, N, block):
            e_ = min(N, s + block)
            a_d, b_d, c_d, m_d, e_d = h.match_pairs(self.templates, f[s:e_], w[s:e_], cand[s:e_].contiguous(), k, n=nobs, return_all=return_all)
            idx_a[s:e_], idx_b[s:e_], chisq[s:e_], amp[s:e_] = a_d.cpu().numpy(), b_d.cpu().numpy(), c_d.cpu().numpy(), m_d.cpu().numpy()
            if return_all:
                every[s:e_] = e_d.cpu().numpy()
        swap = amp[:, :, 1] > amp[:, :, 0]                           # A is the brighter
        index_a, index_b = np.where(swap, idx_b, idx_a), np.where(swap, idx_a, idx_b)
        bright, faint = np.where(swap, amp[:, :, 1], amp[:, :, 0]), np.where(swap, amp[:, :, 0], amp[:, :, 1])
        scale = bright + faint
        listed = (index_a >= 0)[:, :, None]
        out = dict(index_a=index_a, index_b=index_b, chisq=chisq, scale=scale, ratio=faint / scale,
                   pars_a=np.where(listed, self.theta[np.maximum(index_a, 0)], np.nan), pars_b=np.where(listed, self.theta[np.maximum(index_b, 0)], np.nan),
                   npix=single["npix"], shortlist=sl, single_chisq=single["chisq"][:, 0].copy())
        if return_all:
            out["all"] = every
        return out

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self._handle.close()
            self._handle = None
        if getattr(self, "_pair_handle", None) is not None:
            self._pair_handle.close()
            self._pair_handle = None
