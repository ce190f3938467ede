"""Training the photometric emulator: mirrors Payne/train/trainphot.py (``TrainMod``, ``EarlyStopping``, ``defmod``).

``TrainMod`` takes the reference's keyword arguments and writes the file ``Payne.predict.photANN_new.modpred`` reads.  One step
(forward in training mode, ``MSELoss(reduction='mean')``, backward, ``torch.optim.RAdam(lr)`` with its defaults;
trainphot.py:343,353,411-447) is three HIP launches through ``payne_lnmlp_train_step`` (csrc/k_lnmlp_train.hip); the epoch loop
stays here and reads one block of losses per epoch.  There is no host evaluation of the network.

Where this differs from the reference, on purpose:

* the split.  The reference builds three ``ReadPhot`` instances (test, train, valid), each of which shuffles the table with its
  own unseeded generator, so its three sets overlap.  Here ONE permutation, seeded by ``seed``, gives disjoint sets: the first
  ``rint((1 - trainper) n)`` models are the test set, the next 70 % of the rest the training set, the last 30 % the validation
  set.  ``normfactor`` is ``[mean, std]`` per label over the whole table before ``parrange`` cuts it, as ``ReadPhot`` has it.
* ``EarlyStopping(patience=50, min_delta=1e-4)`` is created once per run.  The reference creates it inside the epoch loop
  (trainphot.py:404), so its counter never passes 1 and its stopper cannot fire.
* the batches of an epoch come from a seeded device permutation (``epoch_order``), not from an unseeded ``RandomSampler``; the
  dropout mask is a counter-based function of (seed, step, layer, row, column) (``payne_lnmlp_dropout_mask``).
* initial parameters are torch's defaults (Linear weight and bias U(+-1/sqrt(n_in)), LayerNorm 1 / 0) drawn from a numpy
  generator on ``seed``.
* the model is also written after the last epoch, and the container is ``.npz`` (``.h5`` where ``output`` ends in ``.h5`` and
  h5py is installed), rewritten whole each time.
* extra keywords: ``seed`` (0), ``dropout`` (None = the type's own, MLP_v0 0.3 behind block 3, MLP_v1 0.01 behind block 2; a
  number overrides it, 0 switches it off), ``device``.
"""
import ctypes as C
import sys
import traceback
from datetime import datetime

import numpy as np

from .. import _lib, nnio
from ..predict import photANN_new as photANN

NNTYPES = photANN.NNTYPES
DROPOUT = {"MLP_v0": (2, 0.3), "MLP_v1": (1, 0.01)}               # (hidden block behind which d1 sits, its p): NNmodels_new.py:21,48


class EarlyStopping:
    """trainphot.py:50-75, unchanged."""

    def __init__(self, patience=100, min_delta=0.0, verbose=True):
        self.patience = patience
        self.min_delta = min_delta
        self.verbose = verbose
        self.counter = 0
        self.best_loss = np.inf
        self.should_stop = False

    def step(self, current_loss):
        if (self.best_loss - current_loss) > self.min_delta:
            self.best_loss = current_loss
            self.counter = 0
        else:
            self.counter += 1
            if self.verbose:
                print(f"... EarlyStopping: No improvement for {self.counter}/{self.patience} epochs")
            if self.counter >= self.patience:
                self.should_stop = True
        return self.should_stop


def layer_names(nntype):
    n_hidden, out_name = NNTYPES[nntype]
    return [("lin%d" % i, "ln%d" % i) for i in range(1, n_hidden + 1)] + [(out_name, None)]


def init_arrays(D_in, H1, H2, H3, D_out, NNtype='MLP_v0', seed=0):
    """A new network's arrays under the reference's key names, drawn as torch initialises nn.Linear and nn.LayerNorm."""
    if NNtype not in NNTYPES:
        raise ValueError("NNtype %r: one of %s" % (NNtype, sorted(NNTYPES)))
    rng = np.random.default_rng(seed)
    widths = [H1, H2, H3, H3, H3][:NNTYPES[NNtype][0]] + [D_out]
    arrs, n_in = {}, D_in
    for (lin, lnm), w in zip(layer_names(NNtype), widths):
        k = 1.0 / np.sqrt(n_in)
        arrs["model/mlp.%s.weight" % lin] = rng.uniform(-k, k, (w, n_in)).astype(np.float32)
        arrs["model/mlp.%s.bias" % lin] = rng.uniform(-k, k, w).astype(np.float32)
        if lnm is not None:
            arrs["model/mlp.%s.weight" % lnm] = np.ones(w, dtype=np.float32)
            arrs["model/mlp.%s.bias" % lnm] = np.zeros(w, dtype=np.float32)
        n_in = w
    return arrs


def defmod(D_in, H1, H2, H3, D_out, NNtype='MLP_v0', seed=0):
    """trainphot.py:77-81: a new network (what ``photANN_new.readNN`` returns)."""
    return photANN.LNMLP(init_arrays(D_in, H1, H2, H3, D_out, NNtype=NNtype, seed=seed), NNtype)


def layers_to_arrays(layers, nntype):
    arrs = {}
    for (lin, lnm), (w, b, g, be) in zip(layer_names(nntype), layers):
        arrs["model/mlp.%s.weight" % lin], arrs["model/mlp.%s.bias" % lin] = w, b
        if lnm is not None:
            arrs["model/mlp.%s.weight" % lnm], arrs["model/mlp.%s.bias" % lnm] = g, be
    return arrs


def _desc(layers):
    """(LnmlpDesc over the arrays of `layers`, which must stay alive and be C-contiguous fp32)."""
    d = _lib.LnmlpDesc()
    d.n_layers = len(layers)
    for i, (w, b, g, be) in enumerate(layers):
        L = d.layers[i]
        L.n_out, L.n_in = w.shape
        L.w, L.b = w.ctypes.data, b.ctypes.data
        L.ln_gain, L.ln_bias = (None, None) if g is None else (g.ctypes.data, be.ctypes.data)
    return d


class Trainer(object):
    """One network in training on the device: payne_lnmlp_train_* behind tensors.  `layers`: [(W, b, gain | None, beta | None)]
    fp32, the initial parameters; `dropout_p`: the probability behind every hidden block."""

    def __init__(self, layers, dropout_p, lr=1e-3, seed=0, max_rows=2048, device=None, betas=(0.9, 0.999), eps=1e-8):
        import torch
        self._lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self._shapes = [tuple(f32(a) for a in L) for L in layers]
        self.D_in, self.D_out = self._shapes[0][0].shape[1], self._shapes[-1][0].shape[0]
        o = _lib.LnmlpTrainOpts()
        o.lr, o.beta1, o.beta2, o.eps, o.seed, o.max_rows = lr, betas[0], betas[1], eps, seed, max_rows
        for i, p in enumerate(dropout_p):
            o.dropout_p[i] = p
        self.max_rows = max_rows
        self._handle = None
        h = C.c_void_p()
        rc = self._lib.payne_lnmlp_train_create(self.device.index, C.byref(_desc(self._shapes)), C.byref(o), C.byref(h))
        if rc != 0:
            err = self._lib.payne_last_error(None).decode()
            raise (ValueError if rc in (_lib.E_UNSUPPORTED, _lib.E_INVALID) else RuntimeError)("payne_lnmlp_train_create failed (%d): %s" % (rc, err))
        self._handle = h

    def _call(self, fn, x, t, loss_out):
        import torch
        for a, d in ((x, self.D_in), (t, self.D_out)):
            if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != d or a.stride(1) != 1 or a.device != self.device:
                raise ValueError("x / t: fp32 [N, %d] / [N, %d] on %s with unit column stride" % (self.D_in, self.D_out, self.device))
        if x.shape[0] != t.shape[0]:
            raise ValueError("x and t differ in rows")
        if loss_out is not None and (loss_out.dtype != torch.float64 or loss_out.device != self.device):
            raise ValueError("loss_out: a float64 tensor on %s" % self.device)
        rc = fn(self._handle, x.data_ptr(), x.stride(0), t.data_ptr(), t.stride(0), x.shape[0],
                None if loss_out is None else loss_out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (fn.__name__, rc))

    def step(self, x, t, loss_out=None):
        """One forward / backward / RAdam update on the batch; the loss before the update goes to loss_out[0] on the device."""
        self._call(self._lib.payne_lnmlp_train_step, x, t, loss_out)

    def loss(self, x, t, loss_out):
        """The loss in evaluation mode (no dropout, nothing changes) to loss_out[0]."""
        self._call(self._lib.payne_lnmlp_train_loss, x, t, loss_out)

    def _get(self, what):
        out = [tuple(None if a is None else np.empty_like(a) for a in L) for L in self._shapes]
        rc = self._lib.payne_lnmlp_train_get(self._handle, what, C.byref(_desc(out)))
        if rc != 0:
            raise RuntimeError("payne_lnmlp_train_get failed (%d)" % rc)
        return out

    def params(self):
        return self._get(_lib.LNMLP_PARAMS)

    def grads(self):
        return self._get(_lib.LNMLP_GRADS)

    @property
    def steps(self):
        return int(self._lib.payne_lnmlp_train_steps(self._handle))

    def close(self):
        if self._handle is not None:
            self._lib.payne_lnmlp_train_destroy(self._handle)
            self._handle = None

    def __del__(self):
        if getattr(self, "_handle", None) is not None and self._lib is not None:
            self.close()


def dropout_mask(seed, step, layer, n_rows, n_cols, p):
    """The mask of hidden block `layer` in step `step` (0 = a trainer's first) as uint8 [n_rows, n_cols]; host only."""
    out = np.empty((n_rows, n_cols), dtype=np.uint8)
    rc = _lib.load().payne_lnmlp_dropout_mask(seed, step, layer, n_rows, n_cols, p, out.ctypes.data)
    if rc != 0:
        raise ValueError("payne_lnmlp_dropout_mask: bad arguments")
    return out


class TrainMod(object):
    """trainphot.TrainMod: the reference's keyword arguments, ``__call__``, ``run`` and ``train_mod``; see the module docstring."""

    def __init__(self, *arg, **kwargs):
        super(TrainMod, self).__init__()
        self.verbose = kwargs.get('verbose', False)
        self.logplot = kwargs.get('logplot', True)
        self.trainper = kwargs.get('trainper', 0.9)
        self.numepochs = kwargs.get('numepochs', 10000)
        self.batchsize = kwargs.get('batchsize', 2048)
        self.lr = kwargs.get('lr', 1E-3)
        self.NNtype = kwargs.get('NNtype', 'MLP_v0')
        if self.NNtype not in NNTYPES:
            raise ValueError("NNtype %r: one of %s" % (self.NNtype, sorted(NNTYPES)))
        self.H1 = kwargs.get('H1', 256)
        self.H2 = kwargs.get('H2', 256)
        self.H3 = kwargs.get('H3', 256)
        self.label_i = list(kwargs.get('label_i', ['teff', 'logg', 'feh', 'afe', 'av', 'rv']))
        self.label_o = list(kwargs.get('label_o', [
            'roman_wfi_f062', 'roman_wfi_f087', 'roman_wfi_f106', 'roman_wfi_f129', 'roman_wfi_f146', 'roman_wfi_f158',
            'roman_wfi_f184', 'roman_wfi_f213']))
        self.D_in = len(self.label_i)
        self.D_out = len(self.label_o)
        defaultparrange = ({
            'Teff': [0.0, 1000000.0],
            'logg': [-2.0, 6.0],
            'FeH': [-10.0, 10.0],
            'aFe': [-10.0, 10.0],
            'Av': [-1.0, 100.0],
            'Rv': [2.0, 6.0],
            })
        self.parrange = kwargs.get('parrange', defaultparrange)
        self.restartfile = kwargs.get('restartfile', None)
        self.outfilename = kwargs.get('output', 'TESTOUT.h5')
        self.modpath = kwargs.get('modpath', './cwc_models.h5')
        self.norm = kwargs.get('norm', True)
        self.seed = int(kwargs.get('seed', 0))
        self.dropout = kwargs.get('dropout', None)
        self.device = kwargs.get('device', None)
        self._read_grid()
        self._out = {
            'testlabels_in': self.test_labelsin, 'testlabels_out': self.test_labelsout,
            'label_i': np.array([x.encode("ascii", "ignore") for x in self.label_i]),
            'label_o': np.array([x.encode("ascii", "ignore") for x in self.label_o])}
        if self.norm:
            for kk in self.label_i:
                self._out['norm_i/%s' % kk] = np.array(self.normfactor[kk])
            for kk in self.label_o:
                self._out['norm_o/%s' % kk] = np.array(self.normfactor[kk])
        self._write()

    # ---- data ----
    def _read_grid(self):
        """ReadPhot (Payne/utils/readKorg.py:22-175) for the three sets at once: the table, normfactor, parrange, one split."""
        tab = nnio.load_arrays(self.modpath)
        pars = tab['parameters']
        if pars.dtype.names is None:
            raise ValueError("%s: 'parameters' is not a record array" % self.modpath)

        def column(ll):
            if ll in pars.dtype.names:
                return np.asarray(pars[ll], dtype=np.float64)
            f = ll.split('_')[-1]
            ss = ll.replace('_' + f, '')
            return np.asarray(tab[ss][f], dtype=np.float64)
        cols = {ll: column(ll) for ll in self.label_i + self.label_o}
        normfactor = {ll: [np.mean(c), np.std(c)] for ll, c in cols.items()}
        sel = np.ones(len(pars), dtype=bool)
        if self.parrange is not None:
            for ll in self.label_i:
                if ll in self.parrange.keys():
                    sel &= (cols[ll] >= self.parrange[ll][0]) & (cols[ll] <= self.parrange[ll][1])
        index = np.nonzero(sel)[0]
        index = index[np.random.default_rng(self.seed).permutation(len(index))]
        n = len(index)
        n_test = int(np.rint((1.0 - self.trainper) * n))
        rest = index[n_test:]
        n_train = int(np.rint(0.7 * len(rest)))
        self.testind, self.trainind, self.validind = index[:n_test], rest[:n_train], rest[n_train:]
        self.normfactor = normfactor if self.norm else None
        x = np.stack([cols[ll] for ll in self.label_i], axis=1)
        y = np.stack([cols[ll] for ll in self.label_o], axis=1)
        self.test_labelsin = x[self.testind].T.astype(np.float32)       # [D_in, n_test], not normalised (trainphot.py:159-188)
        self.test_labelsout = y[self.testind].T.astype(np.float32)
        if self.norm:
            x = (x - np.array([normfactor[ll][0] for ll in self.label_i])) / np.array([normfactor[ll][1] for ll in self.label_i])
            y = (y - np.array([normfactor[ll][0] for ll in self.label_o])) / np.array([normfactor[ll][1] for ll in self.label_o])
        self._x32, self._y32 = x.astype(np.float32), y.astype(np.float32)

    def set_data(self, which):
        """(x, t) of 'train', 'valid' or 'test' as the network is given them: fp32 numpy, normalised when norm is set."""
        ind = {'train': self.trainind, 'valid': self.validind, 'test': self.testind}[which]
        return self._x32[ind], self._y32[ind]

    def epoch_order(self, epoch, which='train'):
        """The seeded permutation of the 'train' (or 'valid') set for `epoch`, a tensor on the training device; batch i is
        its elements [i * batchsize, (i + 1) * batchsize), the tail is dropped."""
        import torch
        n = len({'train': self.trainind, 'valid': self.validind}[which])
        g = torch.Generator(device=self._torch_device())
        g.manual_seed((self.seed * 1000003 + epoch) * 2 + (which == 'valid'))
        return torch.randperm(n, generator=g, device=self._torch_device())

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

    def dropout_p(self):
        n_hidden = NNTYPES[self.NNtype][0]
        block, p = DROPOUT[self.NNtype]
        out = [0.0] * n_hidden
        out[block] = float(p if self.dropout is None else self.dropout)
        return out

    # ---- the reference's entry points ----
    def __call__(self, dryrun=False):
        try:
            return self.train_mod(dryrun=dryrun)
        except Exception as e:
            traceback.print_exc()
            print()
            raise e

    def run(self, dryrun=False):
        tottimestart = datetime.now()
        net = self(dryrun=dryrun)
        if self.verbose:
            print('Finished Training at {0} ({1})'.format(datetime.now(), datetime.now() - tottimestart))
        return net

    def train_mod(self, dryrun=False):
        import torch
        starttime = datetime.now()
        if self.restartfile is not None:
            model = photANN.readNN(self.restartfile, nntype=self.NNtype)
            if model.D_in != self.D_in or model.D_out != self.D_out:
                raise ValueError("restartfile maps %d labels to %d bands, label_i / label_o ask for %d and %d"
                                 % (model.D_in, model.D_out, self.D_in, self.D_out))
        else:
            model = defmod(self.D_in, self.H1, self.H2, self.H3, self.D_out, NNtype=self.NNtype, seed=self.seed)
        dev = self._torch_device()
        trainer = Trainer(model.layers, self.dropout_p(), lr=self.lr, seed=self.seed, max_rows=self.batchsize, device=dev)
        self.trainer = trainer
        if dryrun:
            return [model, trainer, datetime.now() - starttime]

        xt, yt = (torch.as_tensor(a).to(dev) for a in self.set_data('train'))
        xv, yv = (torch.as_tensor(a).to(dev) for a in self.set_data('valid'))
        nbatches, nvalid = xt.shape[0] // self.batchsize, xv.shape[0] // self.batchsize
        self.nbatches, self.nvalid = nbatches, nvalid
        if nbatches < 1:
            raise ValueError("the training set (%d models) is smaller than one batch of %d" % (xt.shape[0], self.batchsize))
        fig = self._figure()
        self.batchloss_arr, self.batchloss_std, self.batchloss_med = [], [], []
        self.validloss_arr, self.validloss_std, self.validloss_med = [], [], []
        self.running_loss, self.running_valid = [], []              # per batch, one row per epoch
        early_stopper = EarlyStopping(patience=50, min_delta=1e-4, verbose=self.verbose)
        losses = torch.zeros(nbatches + nvalid, dtype=torch.float64, device=dev)
        triggerstop = False
        for epoch in range(self.numepochs):
            epochtime = datetime.now()
            order = self.epoch_order(epoch, 'train')
            for ii in range(nbatches):
                idx = order[ii * self.batchsize:(ii + 1) * self.batchsize]
                trainer.step(xt[idx], yt[idx], losses[ii:ii + 1])
            order = self.epoch_order(epoch, 'valid')
            for ii in range(nvalid):
                idx = order[ii * self.batchsize:(ii + 1) * self.batchsize]
                trainer.loss(xv[idx], yv[idx], losses[nbatches + ii:nbatches + ii + 1])
            block = losses.cpu().numpy()                             # the epoch's one read
            running_loss, running_valid = block[:nbatches].copy(), block[nbatches:].copy()
            self.running_loss.append(running_loss)
            self.running_valid.append(running_valid)
            batch_loss = np.sum(running_loss) / len(running_loss)
            self.batchloss_arr.append(batch_loss)
            self.batchloss_std.append(np.std(running_loss) / len(running_loss))
            self.batchloss_med.append(np.median(running_loss) / len(running_loss))
            if nvalid > 0:
                valid_loss = np.sum(running_valid) / len(running_valid)
                self.validloss_arr.append(valid_loss)
                self.validloss_std.append(np.std(running_valid) / len(running_valid))
                self.validloss_med.append(np.median(running_valid) / len(running_valid))
            else:                                                   # (the reference divides by zero here)
                valid_loss = np.nan
                self.validloss_arr.append(np.nan)
                self.validloss_std.append(np.nan)
                self.validloss_med.append(np.nan)
            triggerstop = bool(early_stopper.step(valid_loss))
            self._plot(fig, epoch)
            last = epoch + 1 == self.numepochs
            if ((epoch > 0) and (epoch % 10 == 0)) or triggerstop or last:
                model = self._save(trainer)
                if self.verbose:
                    print(f'... Epoch: {epoch+1} / {self.numepochs} - Training log(Loss): {np.log10(batch_loss):.5f} - '
                          f'Validation log(Loss): {np.log10(valid_loss):.5f} - LR: {self.lr:.2e} - Epoch Time: {(datetime.now()-epochtime)}')
                    sys.stdout.flush()
            if triggerstop:
                if self.verbose:
                    print('... Early Stopping Triggered')
                break
        self._close_figure(fig)
        self.stopped_early = triggerstop
        self.elapsed = datetime.now() - starttime
        return model

    def _save(self, trainer):
        arrs = layers_to_arrays(trainer.params(), self.NNtype)
        self._out.update(arrs)
        self._write()
        return photANN.LNMLP(arrs, self.NNtype)

    # ---- the loss figure: only where matplotlib is installed ----
    def _figure(self):
        if not self.logplot:
            return None
        try:
            import matplotlib
            matplotlib.use('AGG')
            import matplotlib.pyplot as plt
        except ImportError:
            return None
        fig, ax = plt.subplots(nrows=3, ncols=1, figsize=(7, 10), layout='constrained')
        for a, lab in zip(ax, ('log(Loss per model)', 'log(Std Residual)', 'log(Med Residual)')):
            a.set_ylabel(lab)
            a.set_xlim(0, self.numepochs)
        ax[2].set_xlabel('Epoch')
        return fig, ax, plt

    def _plot(self, fig, epoch):
        if fig is None:
            return
        f, ax, _ = fig
        with np.errstate(divide='ignore', invalid='ignore'):
            for a, tr, va in zip(ax, (self.batchloss_arr, self.batchloss_std, self.batchloss_med),
                                 (self.validloss_arr, self.validloss_std, self.validloss_med)):
                for line in list(a.lines):
                    line.remove()
                a.plot(np.arange(epoch + 1), np.log10(tr), ls='-', lw=0.5, alpha=0.5, c='C0', label='Training')
                a.plot(np.arange(epoch + 1), np.log10(va), ls='-', lw=0.5, alpha=0.5, c='C3', label='Validation')
        f.savefig('{0}_loss.png'.format(self.outpath.rsplit('.', 1)[0]), dpi=150)

    def _close_figure(self, fig):
        if fig is not None:
            fig[2].close(fig[0])
