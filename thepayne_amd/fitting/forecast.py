"""Fisher forecasts for a spectrum: what precision on the stellar labels a spectrograph can reach at a given S/N.

``Forecast`` evaluates, for a grid of stars, the derivatives of the model spectrum ``getspec`` would return with respect to the
network's labels, the Fisher matrix F = J^T C^-1 J of those rows for a diagonal noise covariance C = diag(obs_eflux^2), and the
Cramer-Rao bounds sqrt(diag(F^-1)).  The network's Jacobian is a forward-mode pass through its dense layers
(payne_specjac_eval), the broadening and resampling that follow are linear in the flux and are applied to its rows by the
engine's own kernels (payne_smooth_batch), and the Fisher matrices are summed in fp64 on the device (payne_fisher_batch).

What is differentiated: the labels of the spectral network -- Teff, log(g), [Fe/H], [alpha/Fe] and, for a five-label network,
Vmic -- at each star's own Vrad, Vrot and Inst_R.  What is not: Vrad, Vrot, Inst_R, the coefficients of a blaze polynomial, and
everything photometric.  The Fisher matrix is therefore conditional on those parameters: the bounds are those of a fit in which
they are known.  A caller who has the derivative of the model with respect to any of them (by finite differences of ``getspec``,
say) passes it as ``extra_rows`` and obtains the joint matrix and the marginal bounds.  A continuum network and an LSF vector are
not supported (``PayneSpecPredict.getgrad`` explains why).
"""
import numpy as np

from ..predict._spec import PayneSpecPredict, fisher_batch, smooth_rows

__all__ = ["Forecast", "weights_from_errors", "crlb_from_fisher"]


def weights_from_errors(eflux):
    """w = 1 / eflux^2, and 0 where eflux is zero or not finite: those pixels do not count."""
    e = np.asarray(eflux, dtype=np.float64)
    w = np.zeros(e.shape)
    ok = np.isfinite(e) & (e != 0.0)
    w[ok] = 1.0 / e[ok] ** 2
    return w


def crlb_from_fisher(F):
    """sqrt(diag(inv(F))) per star for F [N, K, K] (numpy fp64 on the host); NaN for a star whose F is singular or not finite.
    The inverse is taken of F scaled to a unit diagonal (the labels' units differ by many orders of magnitude: K against dex), and
    F counts as singular when that scaled matrix has less than full numerical rank (numpy.linalg.matrix_rank)."""
    F = np.asarray(F, dtype=np.float64)
    out = np.full(F.shape[:2], np.nan)
    for i, Fi in enumerate(F):
        d = np.diag(Fi)
        if not np.all(np.isfinite(Fi)) or np.any(d <= 0.0):
            continue
        s = 1.0 / np.sqrt(d)
        C = Fi * np.outer(s, s)
        if np.linalg.matrix_rank(C) < C.shape[0]:
            continue
        v = np.diag(np.linalg.inv(C))
        out[i] = np.where(v > 0.0, np.sqrt(np.abs(v)), np.nan) * s
    return out


class Forecast(object):
    """Forecast(specANNpath, NNtype, obs_wave, obs_eflux): Fisher matrices and Cramer-Rao bounds on the observed grid ``obs_wave``
    with the per-pixel errors ``obs_eflux`` (in units of the model's flux: 1 / (S/N) for a normalised spectrum)."""

    def __init__(self, specANNpath, NNtype, obs_wave, obs_eflux, device=None, b_max=256):
        self.obs_wave = np.ascontiguousarray(obs_wave, dtype=np.float64)
        self.weights = weights_from_errors(obs_eflux)
        if self.weights.shape != self.obs_wave.shape:
            raise ValueError("obs_eflux and obs_wave differ in length")
        self.predictor = PayneSpecPredict(specANNpath, NNtype=NNtype, device=device, b_max=b_max)
        self.n_labels = self.predictor.anns.n_labels
        self._w_dev = None

    def jacobian(self, pars):
        """pars [N, 8] = Teff, logg, feh, afe, vrad, vrot, vmic, inst_R (getspec's columns; inst_R sigma-based, NaN or <= 0 for
        none) -> the derivatives of getspec's flux on obs_wave with respect to the D labels, a fp32 device tensor [N, D, nobs].
        NaN where obs_wave leaves the model's range."""
        P = self.predictor
        eng, D = P.anns.engine, self.n_labels
        torch = eng.torch
        pars = np.atleast_2d(np.asarray(pars, dtype=np.float64))
        if pars.shape[1] != 8:
            raise ValueError("pars must be [N, 8], got %s" % (pars.shape,))
        N = pars.shape[0]
        P._bind(self.obs_wave)
        out = torch.empty((N, D, len(self.obs_wave)), dtype=torch.float32, device=eng.device)
        step = max(1, eng.b_max // D)                                   # stars per call of the engine
        cols = [0, 1, 2, 3] + ([6] if D == 5 else [])
        for s in range(0, N, step):
            p = pars[s:s + step]
            _, jac = P._jacobian().eval(p[:, cols], want_y=False)
            th = np.full((len(p), D, eng.ncols), np.nan)
            th[:, :, :8] = p[:, None, :]
            out[s:s + len(p)] = smooth_rows(eng, jac.reshape(len(p) * D, -1), th.reshape(len(p) * D, -1), 2).reshape(len(p), D, -1)
        return out

    def fisher(self, pars, extra_rows=None):
        """F [N, K, K] (fp64 device tensor), K = D + M: the labels first, then the caller's ``extra_rows`` [N, M, nobs] (the
        derivatives of the same model spectrum with respect to M parameters of the caller's own)."""
        rows = self.jacobian(pars)
        torch = self.predictor.anns.engine.torch
        if extra_rows is not None:
            extra = torch.as_tensor(np.asarray(extra_rows, dtype=np.float32) if not isinstance(extra_rows, torch.Tensor) else extra_rows)
            extra = extra.to(device=rows.device, dtype=torch.float32)
            if extra.dim() != 3 or extra.shape[0] != rows.shape[0] or extra.shape[2] != rows.shape[2]:
                raise ValueError("extra_rows must be [N, M, nobs], got %s" % (tuple(extra.shape),))
            rows = torch.cat([rows, extra], dim=1)
        if self._w_dev is None or self._w_dev.device != rows.device:
            self._w_dev = torch.as_tensor(self.weights).to(rows.device)
        return fisher_batch(rows, self._w_dev)

    def crlb(self, pars, extra_rows=None):
        """The Cramer-Rao bounds [N, K] = sqrt(diag(inv(F))) (numpy fp64; the inverse is taken on the host).  A star whose F is
        singular gives NaN."""
        return crlb_from_fisher(self.fisher(pars, extra_rows=extra_rows).cpu().numpy())
