"""Payne/testing/testspec.py: checking a trained network file against the held-out test set stored in it, before the
network is trusted in a fit.  The reference evaluates the network on ``testlabels``, forms ``|testpred - prediction|`` and
plots the median of that matrix along both axes, over all test spectra and inside twelve label bins (testspec.py:91-374).

Here the predictions come from the forward pass the likelihood itself uses (payne_predict_batch, stage 0) and stay on the
device; every median is taken there by one payne_mad_stats call (csrc/k_mad.hip), exactly -- radix selection, no sort, no
floating-point sum.  ``TestSpec.stats`` returns the numbers; ``report`` (the reference's ``runtest``) returns them too and, where matplotlib is
installed, draws the reference's first three pages from them.  The later pages compare single spectra against the C3K grid
through readc3k and files that do not ship with either code; they are not built.
"""
from collections import OrderedDict

import numpy as np

from ..predict import predictspec

__all__ = ["TestSpec", "BINS", "label_bins"]

# (name, label column, lower edge exclusive | None, upper edge inclusive | None): testspec.py:125-208
BINS = (("Teff > 6500", 0, 6500.0, None), ("4500 < Teff <= 6500", 0, 4500.0, 6500.0), ("Teff <= 4500", 0, None, 4500.0),
        ("log(g) > 4.0", 1, 4.0, None), ("3.0 < log(g) <= 4.0", 1, 3.0, 4.0), ("log(g) <= 3.0", 1, None, 3.0),
        ("[Fe/H] > 0.0", 2, 0.0, None), ("-1.0 < [Fe/H] <= 0.0", 2, -1.0, 0.0), ("[Fe/H] <= -1.0", 2, None, -1.0),
        ("[a/Fe] > 0.3", 3, 0.3, None), ("0.0 < [a/Fe] <= 0.3", 3, 0.0, 0.3), ("[a/Fe] <= 0.0", 3, None, 0.0))


def label_bins(labels):
    """The reference's twelve row sets as an ordered mapping name -> bool[N]."""
    labels = np.asarray(labels, dtype=np.float64)
    out = OrderedDict()
    for name, col, lo, hi in BINS:
        x = labels[..., col]
        rows = np.ones(x.shape, dtype=bool)
        if lo is not None:
            rows &= x > lo
        if hi is not None:
            rows &= x <= hi
        out[name] = rows
    return out


class TestSpec(object):
    """Class for testing a Payne-learned NN using a testing dataset different from the training spectra
    (Payne/testing/testspec.py:25-70; the same signature and attributes)."""

    def __init__(self, NNfilename, NNtype='LinNet', c3kpath=None, ystnn=None, MISTpath=None,
                 continuum=False, flux=False, window1=[5150, 5200], window2=[5250, 5300]):
        self.NNfilename = NNfilename
        self.NNtype = NNtype
        self.NN = predictspec.ANN(nnpath=self.NNfilename, NNtype=self.NNtype, testing=True, verbose=True)
        self.wave = self.NN.wavelength
        self.resolution = self.NN.resolution
        self.c3kpath = c3kpath
        self.MISTpath = MISTpath
        self.ystnn = ystnn
        self.contbool = continuum
        self.fluxbool = flux
        self.window1 = window1
        self.window2 = window2

    def stats(self, testnum=None, rng=None):
        """The medians of ``|testpred - NN(testlabels)|`` along both axes.

        testnum : draw this many test spectra, ``rng.integers(0, len(testlabels), testnum)`` -- with replacement, as the
                  reference does (testspec.py:79-83); None: every test spectrum once.
        rng     : a numpy Generator (default: a fresh ``default_rng()``).

        ``testpred`` is rounded to fp32 first: the network's output is fp32 (in the reference as here), and the residual is
        the fp64 difference of the two fp32 values.  The predictions are made in chunks of the context's ``b_max`` into one
        device matrix and reduced there without a copy.  Returns a dict: ``wave`` [P], ``labels`` [N, n_labels] (the rows
        used), ``pixel_mad`` [P] (median over spectra at each pixel), ``spec_mad`` [N] (median over pixels of each spectrum)
        and ``bins``, an ordered mapping name -> {'rows': bool[N], 'pixel_mad': [P]} for the reference's twelve label bins
        (NaN where a bin is empty); a bin's per-spectrum medians are ``spec_mad[rows]``."""
        import torch
        from .. import _lib
        NN = self.NN
        labels_all, truth_all = np.asarray(NN.testlabels, dtype=np.float64), np.asarray(NN.testpred)
        if labels_all.ndim != 2 or truth_all.ndim != 2 or len(labels_all) != len(truth_all) or len(labels_all) < 1:
            raise ValueError("testlabels %s and testpred %s are not matrices of one (non-zero) length"
                             % (labels_all.shape, truth_all.shape))
        if testnum is not None:
            rng = np.random.default_rng() if rng is None else rng
            ind = rng.integers(low=0, high=len(labels_all), size=int(testnum))
            labels_all, truth_all = labels_all[ind], truth_all[ind]
        eng = NN.engine
        N, P = truth_all.shape
        if N < 1:
            raise ValueError("no test spectra drawn (testnum = %r)" % (testnum,))
        if P != eng.npix:
            raise ValueError("testpred has %d pixels, the network predicts %d" % (P, eng.npix))
        bins = label_bins(labels_all)
        groups = np.stack([np.ones(N, dtype=bool)] + list(bins.values())).astype(np.uint8)
        G = len(groups)
        matrix = 4 * N * P
        need = 2 * matrix + 8 * (G * P + N) + G * N + 8 * N * eng.ncols
        free = torch.cuda.mem_get_info(eng.device)[0]
        if need > free:
            raise ValueError("the prediction and test matrices (%d x %d fp32, %.2f GiB each) and the results need %.2f GiB on the "
                             "device; %.2f GiB are free (draw fewer spectra with testnum=)"
                             % (N, P, matrix / 2.0 ** 30, need / 2.0 ** 30, free / 2.0 ** 30))
        pred = eng.predict_batch(NN._theta(labels_all), stage=0)
        truth = torch.as_tensor(np.ascontiguousarray(truth_all, dtype=np.float32)).to(eng.device)
        groups_d = torch.as_tensor(groups).to(eng.device)
        pix = torch.empty((G, P), dtype=torch.float64, device=eng.device)
        row = torch.empty(N, dtype=torch.float64, device=eng.device)
        rc = eng.lib.payne_mad_stats(eng.device.index, pred.data_ptr(), pred.stride(0), truth.data_ptr(), truth.stride(0), N, P,
                                     groups_d.data_ptr(), G, pix.data_ptr(), row.data_ptr(), eng._stream())
        if rc == _lib.E_INVALID:
            raise ValueError("payne_mad_stats: invalid arguments")
        if rc != 0:
            raise RuntimeError("payne_mad_stats failed (%d)" % rc)
        pix = pix.cpu().numpy()
        out = OrderedDict(wave=np.asarray(self.wave), labels=labels_all, pixel_mad=pix[0], spec_mad=row.cpu().numpy(), bins=OrderedDict())
        for k, (name, rows) in enumerate(bins.items()):
            out['bins'][name] = {'rows': rows, 'pixel_mad': pix[1 + k]}
        return out

    def report(self, output='./test.pdf', testnum=None, rng=None):
        """Run the test on an already trained network (testspec.py:72-374): returns ``stats(testnum=...)`` and, where
        matplotlib imports, writes the reference's first three pages -- MAD against wavelength with its CDF, per-spectrum MAD
        histograms in the label bins, per-pixel MAD in the label bins -- to ``output`` (default './test.pdf')."""
        st = self.stats(testnum=testnum, rng=rng)
        try:
            import matplotlib
            matplotlib.use('AGG')
            from matplotlib.backends.backend_pdf import PdfPages
            import matplotlib.pyplot as plt
        except ImportError:
            print("TestSpec: matplotlib is not installed, no pages written (the numbers are in the returned dict)")
            return st
        with PdfPages(output) as pdf:
            for page in (self._page_wavelength, self._page_spectrum_hists, self._page_wavelength_bins):
                fig = page(plt, st)
                pdf.savefig(fig)
                plt.close(fig)
        print("TestSpec: wrote 3 pages to %s; skipped the C3K comparison pages (they need readc3k and grid files that do not ship)" % output)
        return st

    runtest = report                 # the reference's name for it (testspec.py:72)

    # -- the reference's pages, drawn from the numbers of stats() -------------------------------------------------
    histxrange = [-4.5, -1]
    _colors = ('C0', 'C3', 'C4')

    @staticmethod
    def _log10(a):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.log10(a)

    def _page_wavelength(self, plt, st):
        fig, ax = plt.subplots(nrows=2, ncols=1, constrained_layout=True, figsize=(8, 8))
        mad = self._log10(st['pixel_mad'])
        ax[0].scatter(st['wave'], mad, marker='.', s=5, ec='none')
        ax[1].hist(mad[np.isfinite(mad)], bins=50, cumulative=True, density=True, range=self.histxrange, histtype='step')
        ax[0].set_xlabel(r'$\lambda$')
        ax[0].set_ylabel('log(median MAD @ pixel)')
        ax[1].set_xlabel('log(median MAD @ pixel)')
        ax[1].set_ylabel('CDF (% of pixels)')
        return fig

    def _page_spectrum_hists(self, plt, st):
        fig, ax = plt.subplots(nrows=2, ncols=2, constrained_layout=True, figsize=(8, 8))
        for k, (name, b) in enumerate(st['bins'].items()):
            a = ax[k // 6, (k // 3) % 2]
            mad = self._log10(st['spec_mad'][b['rows']])
            a.hist(mad[np.isfinite(mad)], bins=25, color=self._colors[k % 3], range=self.histxrange, histtype='step', label=name,
                   density=False, lw=2.0, alpha=0.75)
            if k % 3 == 2:
                a.legend(fontsize=7, frameon=False)
        ax[1, 0].set_xlabel('log median MAD per spectrum')
        ax[1, 1].set_xlabel('log median MAD per spectrum')
        return fig

    def _page_wavelength_bins(self, plt, st):
        from scipy import stats
        fig, ax = plt.subplots(nrows=2, ncols=2, constrained_layout=True, figsize=(8, 8))
        wave = st['wave']
        for k, (name, b) in enumerate(st['bins'].items()):
            a = ax[k // 6, (k // 3) % 2]
            mad = self._log10(b['pixel_mad'])
            ok = np.isfinite(mad)
            if ok.any():
                a.scatter(wave[ok], mad[ok], marker='.', c=self._colors[k % 3], s=1, alpha=0.75, ec='none')
                bin_med, bin_edges, _ = stats.binned_statistic(wave[ok], mad[ok], statistic='median', bins=25)
                a.plot(bin_edges[1:] - (bin_edges[1] - bin_edges[0]) / 2, bin_med, lw=1.0, c=self._colors[k % 3], label=name)
            if k % 3 == 2:
                a.legend(fontsize=7, frameon=False)
        for a in ax.ravel():
            a.set_ylim(-4.5, -1.0)
        ax[1, 0].set_xlabel(r'$\lambda$')
        ax[1, 1].set_xlabel(r'$\lambda$')
        ax[0, 0].set_ylabel('log(median MAD @ pixel)')
        ax[1, 0].set_ylabel('log(median MAD @ pixel)')
        return fig
