"""Training the spectral emulator: mirrors Payne/train/trainspec.py (``TrainMod``, ``defmod``, ``slicebatch``).

``TrainMod`` takes the reference's keyword arguments and writes the file ``Payne.predict.predictspec.PayneSpecPredict(NNtype=...)``
and ``Payne.testing.testspec.TestSpec`` read.  One step (forward, ``MSELoss(reduction='sum')``, backward,
``torch.optim.RAdam(lr)`` with its defaults; trainspec.py:319,328,422-444) on ``SMLP`` or ``LinNet`` of NNmodels.py is five HIP
launches through ``payne_specmlp_train_step`` (csrc/k_specmlp_train.hip); the epoch loop, the learning-rate schedule
(``StepLR(100, 0.9)`` stepped once an epoch, :334,531) and the file stay here.  There is no host evaluation of the network.

Where this differs from the reference, on purpose:

* the grid.  The reference pulls spectra from the C3K / MIST libraries through ``readc3k``; those do not ship.  Here ``c3kpath``
  names a pre-pulled grid file, an ``.npz`` with ``spectra [M, npix]``, ``labels [M, D]``, ``label_names`` and ``wavelengths``
  (``thepayne_amd.synth.spec_grid`` writes one from a teacher network), already at the resolution it is to be learnt at;
  ``waverange`` selects its pixels, ``resolution`` is recorded in the file, ``xmin`` / ``xmax`` are the grid's label ranges and
  ``ymin`` / ``ymax`` its flux range.  ``mistpath`` and the label-range keywords are accepted and unused.
* the split is seeded (``seed``) and disjoint: one permutation of the grid; its first ``numtest`` models are the test set; every
  epoch draws ``numtrain`` training and ``numtrain`` validation models from the rest, without overlap.  The reference draws at
  random and excludes by label value.
* the validation batches are indexed by a permutation of their own.  The reference indexes them with the training loop's stale
  ``perm`` and ``t`` (trainspec.py:463), so that every one of its validation batches is the last training batch's index set.
* ``NNtype='ResNet'`` raises as ``nnio`` does: the reference's own ResNet cannot be constructed (NNmodels.py:38 vs :172).
* initial parameters are torch's ``nn.Linear`` defaults, U(+-1/sqrt(n_in)), drawn from a numpy generator on ``seed``; the
  container is ``.npz`` (``.h5`` where ``output`` ends in ``.h5`` and h5py is installed), rewritten whole after every epoch.
* extra keywords: ``seed`` (0), ``device``, ``verbose``.
"""
import ctypes as C
import sys
import traceback
from datetime import datetime

import numpy as np

from .. import _lib, nnio

fwhm_to_sigma = 2.0 * np.sqrt(2.0 * np.log(2.0))
NNTYPES = {"SMLP": _lib.SPECMLP_LEAKY, "LinNet": _lib.SPECMLP_SIGMOID}


def slicebatch(inlist, N):
    """trainspec.py:51-55: a list in batches of N elements; the last may be shorter."""
    return [inlist[ii:ii + N] for ii in range(0, len(inlist), N)]


def _check_type(NNtype):
    if NNtype not in NNTYPES:
        raise IOError("NNtype %r is not supported (the reference's ResNet cannot be constructed either: "
                      "NNmodels.py:38 vs :172)" % (NNtype,))


def layer_names(NNtype):
    _check_type(NNtype)
    return ["features.%d" % i for i in (0, 2, 4, 6)] if NNtype == "SMLP" else ["lin%d" % i for i in range(1, 7)]


def layer_widths(H1, H2, H3, D_out, NNtype):
    return [H1, H2, H3, D_out] if NNtype == "SMLP" else [H1, H1, H2, H2, H3, D_out]


def defmod(D_in, H1, H2, H3, D_out, xmin=None, xmax=None, NNtype='SMLP', seed=0):
    """trainspec.py:57-63: a new network, as the arrays of its state dict under ``model/<key>`` (+ ``xmin`` / ``xmax`` when
    given), every ``nn.Linear`` drawn as torch draws it: weight and bias U(+-1/sqrt(n_in))."""
    rng = np.random.default_rng(seed)
    arrs, n_in = {}, D_in
    for name, w in zip(layer_names(NNtype), layer_widths(H1, H2, H3, D_out, NNtype)):
        k = 1.0 / np.sqrt(n_in)
        arrs["model/%s.weight" % name] = rng.uniform(-k, k, (w, n_in)).astype(np.float32)
        arrs["model/%s.bias" % name] = rng.uniform(-k, k, w).astype(np.float32)
        n_in = w
    if xmin is not None:
        arrs["xmin"], arrs["xmax"] = np.asarray(xmin, dtype=np.float64), np.asarray(xmax, dtype=np.float64)
    return arrs


def arrays_to_layers(arrs, NNtype):
    return [(np.ascontiguousarray(arrs["model/%s.weight" % n], dtype=np.float32), np.ascontiguousarray(arrs["model/%s.bias" % n], dtype=np.float32))
            for n in layer_names(NNtype)]


def layers_to_arrays(layers, NNtype):
    arrs = {}
    for n, (w, b) in zip(layer_names(NNtype), layers):
        arrs["model/%s.weight" % n], arrs["model/%s.bias" % n] = w, b
    return arrs


def encode(labels, xmin, xmax):
    """NNmodels.py:109-113: (x - xmin) / (xmax - xmin) - 0.5 in fp64, cast to fp32."""
    return ((np.asarray(labels, dtype=np.float64) - xmin) / (xmax - xmin) - 0.5).astype(np.float32)


def lr_at(lr0, epoch):
    """The learning rate of epoch `epoch` (0 = the first) under StepLR(100, gamma=0.9) stepped once an epoch."""
    return lr0 * 0.9 ** (epoch // 100)


def _desc(layers, act):
    """(SpecmlpDesc over the arrays of `layers`, which must stay alive and be C-contiguous fp32)."""
    d = _lib.SpecmlpDesc()
    d.n_layers, d.act = len(layers), act
    for i, (w, b) in enumerate(layers):
        L = d.layers[i]
        L.n_out, L.n_in = w.shape
        L.w, L.b = w.ctypes.data, b.ctypes.data
    return d


class Trainer(object):
    """One network in training on the device: payne_specmlp_train_* behind tensors.  `layers`: [(W, b)] fp32, the initial
    parameters; rows arrive encoded."""

    def __init__(self, layers, NNtype='SMLP', lr=1e-4, max_rows=512, device=None, betas=(0.9, 0.999), eps=1e-8):
        import torch
        _check_type(NNtype)
        self._lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        self._shapes = [tuple(np.ascontiguousarray(a, dtype=np.float32) for a in L) for L in layers]
        self._act = NNTYPES[NNtype]
        self.D_in, self.D_out = self._shapes[0][0].shape[1], self._shapes[-1][0].shape[0]
        o = _lib.SpecmlpTrainOpts()
        o.lr, o.beta1, o.beta2, o.eps, o.max_rows = lr, betas[0], betas[1], eps, max_rows
        self.max_rows = max_rows
        self._handle = None
        h = C.c_void_p()
        rc = self._lib.payne_specmlp_train_create(self.device.index, C.byref(_desc(self._shapes, self._act)), C.byref(o), C.byref(h))
        if rc != 0:
            err = self._lib.payne_last_error(None).decode()
            raise (ValueError if rc in (_lib.E_UNSUPPORTED, _lib.E_INVALID) else RuntimeError)("payne_specmlp_train_create failed (%d): %s" % (rc, err))
        self._handle = h

    def _check(self, a, d, what):
        import torch
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != d or a.stride(1) != 1 or a.device != self.device:
            raise ValueError("%s: fp32 [N, %d] on %s with unit column stride" % (what, d, self.device))

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, fn, x, t, loss_out):
        import torch
        self._check(x, self.D_in, "x")
        self._check(t, self.D_out, "t")
        if x.shape[0] != t.shape[0]:
            raise ValueError("x and t differ in rows")
        if loss_out is not None and (loss_out.dtype != torch.float64 or loss_out.device != self.device):
            raise ValueError("loss_out: a float64 tensor on %s" % self.device)
        rc = fn(self._handle, x.data_ptr(), x.stride(0), t.data_ptr(), t.stride(0), x.shape[0],
                None if loss_out is None else loss_out.data_ptr(), self._stream())
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (fn.__name__, rc))

    def step(self, x, t, loss_out=None):
        """One forward / backward / RAdam update on the batch; the sum of squares before the update goes to loss_out[0]."""
        self._call(self._lib.payne_specmlp_train_step, x, t, loss_out)

    def loss(self, x, t, loss_out):
        """The sum of squares on (x, t) to loss_out[0]; nothing changes."""
        self._call(self._lib.payne_specmlp_train_loss, x, t, loss_out)

    def predict(self, x):
        """The network's output on the encoded rows x: fp32 [N, D_out] on the device."""
        import torch
        self._check(x, self.D_in, "x")
        y = torch.empty((x.shape[0], self.D_out), dtype=torch.float32, device=self.device)
        rc = self._lib.payne_specmlp_train_predict(self._handle, x.data_ptr(), x.stride(0), x.shape[0], y.data_ptr(), y.stride(0), self._stream())
        if rc != 0:
            raise RuntimeError("payne_specmlp_train_predict failed (%d)" % rc)
        return y

    def set_lr(self, lr):
        if self._lib.payne_specmlp_train_set_lr(self._handle, float(lr)) != 0:
            raise ValueError("learning rate %r" % (lr,))

    def _get(self, what):
        out = [tuple(np.empty_like(a) for a in L) for L in self._shapes]
        rc = self._lib.payne_specmlp_train_get(self._handle, what, C.byref(_desc(out, self._act)))
        if rc != 0:
            raise RuntimeError("payne_specmlp_train_get failed (%d)" % rc)
        return out

    def params(self):
        return self._get(_lib.SPECMLP_PARAMS)

    def grads(self):
        return self._get(_lib.SPECMLP_GRADS)

    @property
    def steps(self):
        return int(self._lib.payne_specmlp_train_steps(self._handle))

    def close(self):
        if self._handle is not None:
            self._lib.payne_specmlp_train_destroy(self._handle)
            self._handle = None

    def __del__(self):
        if getattr(self, "_handle", None) is not None and self._lib is not None:
            self.close()


def read_grid(path):
    """The pre-pulled grid file: (spectra fp32 [M, npix], labels fp64 [M, D], label names, wavelengths fp64 [npix])."""
    arrs = nnio.load_arrays(path)
    for k in ("spectra", "labels", "label_names", "wavelengths"):
        if k not in arrs:
            raise ValueError("%s: no %r (a grid file holds spectra, labels, label_names, wavelengths)" % (path, k))
    spectra, labels = np.asarray(arrs["spectra"], dtype=np.float32), np.asarray(arrs["labels"], dtype=np.float64)
    names = [s.decode("utf-8") if isinstance(s, bytes) else str(s) for s in arrs["label_names"]]
    wave = np.asarray(arrs["wavelengths"], dtype=np.float64)
    if spectra.ndim != 2 or labels.ndim != 2 or spectra.shape[0] != labels.shape[0] or spectra.shape[1] != len(wave) or labels.shape[1] != len(names):
        raise ValueError("%s: spectra %s, labels %s, %d label names, %d wavelengths do not fit together"
                         % (path, spectra.shape, labels.shape, len(names), len(wave)))
    return spectra, labels, names, wave


class TrainMod(object):
    """trainspec.TrainMod: the reference's keyword arguments, ``__call__``, ``run`` and ``train_mod``; see the module docstring."""

    def __init__(self, *arg, **kwargs):
        super(TrainMod, self).__init__()
        self.numtrain = kwargs.get('numtrain', 20000)
        self.numtest = kwargs.get('numtest', int(0.1 * self.numtrain))
        self.numsteps = kwargs.get('numsteps', int(1e+4))
        self.numepochs = kwargs.get('numepochs', 1)
        self.batchsize = kwargs.get('batchsize', self.numtrain)
        self.H1 = kwargs.get('H1', 256)
        self.H2 = kwargs.get('H2', 256)
        self.H3 = kwargs.get('H3', 256)
        self.label_i = list(kwargs.get('labels_in', ['teff', 'logg', 'feh', 'afe']))
        self.dividecont = kwargs.get('dividecont', True)
        resolution_fwhm = kwargs.get('resolution', 32000.0)
        self.resolution = resolution_fwhm * fwhm_to_sigma
        self.waverange = kwargs.get('waverange', [5150.0, 5300.0])
        self.restartfile = kwargs.get('restartfile', False)
        self.outfilename = kwargs.get('output', 'TESTOUT.h5')
        self.c3kpath = kwargs.get('c3kpath', None)
        self.mistpath = kwargs.get('mistpath', None)
        self.NNtype = kwargs.get('NNtype', 'SMLP')
        _check_type(self.NNtype)
        self.logplot = kwargs.get('logplot', False)
        self.lr = kwargs.get('lr', 1E-4)
        self.seed = int(kwargs.get('seed', 0))
        self.device = kwargs.get('device', None)
        self.verbose = kwargs.get('verbose', False)
        if self.c3kpath is None:
            raise IOError("c3kpath names the pre-pulled grid file (.npz: spectra, labels, label_names, wavelengths); the C3K / MIST "
                          "readers are not part of this build")
        self._read_grid()
        self.D_in, self.D_out = len(self.label_i), len(self.wavelengths)
        self._out = {
            'testpred': self.spectra[self.testind], 'testlabels': self.testlabels,
            'label_i': np.array([x.encode("ascii", "ignore") for x in self.label_i]),
            'wavelengths': self.wavelengths, 'resolution': np.array(self.resolution),
            'xmin': self.xmin, 'xmax': self.xmax, 'ymin': self.ymin, 'ymax': self.ymax}
        self._write()

    # ---- data ----
    def _read_grid(self):
        spectra, labels, names, wave = read_grid(self.c3kpath)
        missing = [x for x in self.label_i if x not in names]
        if missing:
            raise ValueError("%s holds the labels %s, not %s" % (self.c3kpath, names, missing))
        cols = [names.index(x) for x in self.label_i]
        pix = np.nonzero((wave >= self.waverange[0]) & (wave <= self.waverange[1]))[0]
        if len(pix) == 0:
            raise ValueError("no pixel of %s lies in waverange %s" % (self.c3kpath, list(self.waverange)))
        self.spectra = np.ascontiguousarray(spectra[:, pix])
        self.labels = np.ascontiguousarray(labels[:, cols])
        self.wavelengths = wave[pix]
        M = len(self.labels)
        if M < self.numtest + 2 * self.numtrain:
            raise ValueError("%s holds %d models; numtest + 2 numtrain = %d are needed" % (self.c3kpath, M, self.numtest + 2 * self.numtrain))
        self.xmin, self.xmax = self.labels.min(axis=0), self.labels.max(axis=0)
        self.ymin, self.ymax = np.array([self.spectra.min()], dtype=np.float64), np.array([self.spectra.max()], dtype=np.float64)
        order = np.random.default_rng(self.seed).permutation(M)
        self.testind, self.poolind = order[:self.numtest], order[self.numtest:]
        self.testlabels = self.labels[self.testind]
        self._x32 = encode(self.labels, self.xmin, self.xmax)       # the static label table, encoded once

    def epoch_sets(self, epoch):
        """(training indices, validation indices) of `epoch`: numtrain each, disjoint from each other and from the test set."""
        pick = np.random.default_rng([self.seed, 1, epoch]).permutation(len(self.poolind))[:2 * self.numtrain]
        return self.poolind[pick[:self.numtrain]], self.poolind[pick[self.numtrain:]]

    def pass_order(self, epoch, iter_i, which='train'):
        """The seeded permutation of the epoch's training (or validation) set for pass `iter_i`, a tensor on the training device;
        batch t is its elements [t * batchsize, (t + 1) * batchsize)."""
        import torch
        g = torch.Generator(device=self._torch_device())
        g.manual_seed(((self.seed * 1000003 + epoch) * 1000003 + iter_i) * 2 + (which == 'valid'))
        return torch.randperm(self.numtrain, generator=g, device=self._torch_device())

    def lr_of_epoch(self, epoch):
        return lr_at(self.lr, epoch)

    def _torch_device(self):
        import torch
        return torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)

    # ---- output ----
    def _write(self):
        if self.outfilename.endswith('.h5'):
            try:
                import h5py
            except ImportError:
                h5py = None
            if h5py is not None:
                with h5py.File(self.outfilename, 'w') as f:
                    for k, v in self._out.items():
                        f.create_dataset(k, data=v)
                self.outpath = self.outfilename
                return
        self.outpath = self.outfilename if self.outfilename.endswith('.npz') else self.outfilename.rsplit('.h5', 1)[0] + '.npz'
        np.savez(self.outpath, **self._out)

    # ---- the reference's entry points ----
    def __call__(self):
        try:
            return self.train_mod()
        except Exception as e:
            traceback.print_exc()
            print()
            raise e

    def run(self):
        tottimestart = datetime.now()
        net = self()
        if self.verbose:
            print('Finished Training at {0} ({1})'.format(datetime.now(), datetime.now() - tottimestart))
        return net

    def _initial_layers(self):
        if self.restartfile is not False and self.restartfile is not None:
            net = nnio.load_spec_net(self.restartfile, self.NNtype)
            layers = [(w, b) for w, b, act in net["layers"]]
            if layers[0][0].shape[1] != self.D_in or layers[-1][0].shape[0] != self.D_out:
                raise ValueError("restartfile maps %d labels to %d pixels, the grid asks for %d and %d"
                                 % (layers[0][0].shape[1], layers[-1][0].shape[0], self.D_in, self.D_out))
            return layers
        return arrays_to_layers(defmod(self.D_in, self.H1, self.H2, self.H3, self.D_out, NNtype=self.NNtype, seed=self.seed), self.NNtype)

    def train_mod(self):
        import torch
        starttime = datetime.now()
        dev = self._torch_device()
        nbatches = self.numtrain // self.batchsize
        if nbatches < 1:
            raise ValueError("numtrain (%d) is smaller than one batch of %d" % (self.numtrain, self.batchsize))
        trainer = Trainer(self._initial_layers(), NNtype=self.NNtype, lr=self.lr, max_rows=self.batchsize, device=dev)
        self.trainer, self.nbatches = trainer, nbatches
        x_all = torch.as_tensor(self._x32).to(dev)
        self.iter_arr, self.training_loss, self.validation_loss = [], [], []      # one entry per validation, (epoch, pass) in iter_arr
        self.lr_used = []
        train_d = torch.zeros(1, dtype=torch.float64, device=dev)
        valid_d = torch.zeros(nbatches, dtype=torch.float64, device=dev)
        for epoch_i in range(int(self.numepochs)):
            epochtime = datetime.now()
            trainind, validind = self.epoch_sets(epoch_i)
            X_train, Y_train = x_all[torch.as_tensor(trainind).to(dev)], torch.as_tensor(self.spectra[trainind]).to(dev)
            X_valid, Y_valid = x_all[torch.as_tensor(validind).to(dev)], torch.as_tensor(self.spectra[validind]).to(dev)
            self.lr_used.append(self.lr_of_epoch(epoch_i))
            trainer.set_lr(self.lr_used[-1])
            for iter_i in range(int(self.numsteps)):
                perm = self.pass_order(epoch_i, iter_i)
                for t in range(nbatches):
                    idx = perm[t * self.batchsize:(t + 1) * self.batchsize]
                    trainer.step(X_train[idx], Y_train[idx], train_d)
                if iter_i % 100 == 0:
                    perm_valid = self.pass_order(epoch_i, iter_i, 'valid')
                    for j in range(nbatches):
                        idx = perm_valid[j * self.batchsize:(j + 1) * self.batchsize]
                        trainer.loss(X_valid[idx], Y_valid[idx], valid_d[j:j + 1])
                    loss_data = float(train_d.cpu().numpy()[0])
                    loss_valid_data = float(np.sum(valid_d.cpu().numpy()) / nbatches)
                    self.iter_arr.append((epoch_i, iter_i))
                    self.training_loss.append(loss_data)
                    self.validation_loss.append(loss_valid_data)
                    if self.verbose and iter_i % 500 == 0:
                        print('--> Ep: {0:d} -- Iter {1:d}/{2:d} -- Train Loss: {3:.6f} -- Valid Loss: {4:.6f}'.format(
                            int(epoch_i + 1), int(iter_i + 1), int(self.numsteps), loss_data, loss_valid_data))
                        sys.stdout.flush()
            layers = trainer.params()
            self._out.update(layers_to_arrays(layers, self.NNtype))
            self._write()
            if self.verbose:
                print('Finished Epoch {0} @ {1} ({2})'.format(epoch_i + 1, datetime.now(), datetime.now() - epochtime))
        self._plot()
        self.elapsed = datetime.now() - starttime
        return [layers_to_arrays(trainer.params(), self.NNtype), trainer, self.elapsed]

    # ---- the loss figure: only where asked for and matplotlib is installed ----
    def _plot(self):
        if not self.logplot or not self.training_loss:
            return
        try:
            import matplotlib
            matplotlib.use('AGG')
            import matplotlib.pyplot as plt
        except ImportError:
            return
        fig, ax = plt.subplots(nrows=1, ncols=1)
        it = np.arange(len(self.training_loss))
        with np.errstate(divide='ignore', invalid='ignore'):
            ax.plot(it, np.log10(self.training_loss) - np.log10(self.D_out), ls='-', lw=1.0, alpha=0.75, c='C0', label='Training')
            ax.plot(it, np.log10(self.validation_loss) - np.log10(self.D_out), ls='-', lw=1.0, alpha=0.75, c='C3', label='Validation')
        ax.legend()
        ax.set_xlabel('Validation')
        ax.set_ylabel('log(Loss per pixel)')
        fig.savefig('{0}_loss.png'.format(self.outpath.rsplit('.', 1)[0]), dpi=150)
        plt.close(fig)
