"""The current photometric emulator: mirrors Payne/predict/photANN_new.py (``readNN``, ``ANN``, ``modpred``).

One network maps ``[teff, logg, feh, afe, av, rv]`` to every band at once through Linear -> LayerNorm -> SiLU blocks
(``MLP_v0``: five blocks and ``lin6``; ``MLP_v1``: three blocks and ``linout``; Payne/train/NNmodels_new.py, written by
trainphot.py; the dropout layers are the identity in ``eval()``).  The forward pass is one launch of payne_lnmlp_kernel
(csrc/k_lnmlp.hip) for all rows; there is no host evaluation.  Files are the native ``.npz`` container with the reference's
HDF5 key names (``model/mlp.lin1.weight`` ..., ``label_i``, ``label_o``, ``norm_i/<label>``, ``norm_o/<label>``), or the
``.h5`` file itself where h5py is installed (nnio).

``ANN.eval`` takes what the reference's takes (a list, a 1-D array, an ``[N, D_in]`` array; returned: squeezed fp32 numpy) and,
for batches, a device tensor, which is answered by a device tensor without a host round trip."""
import ctypes as C

import numpy as np

from .. import _lib, nnio

NNTYPES = {"MLP_v0": (5, "lin6"), "MLP_v1": (3, "linout")}       # hidden blocks, the output layer's name


class LNMLP(object):
    """One network on the host (what ``readNN`` returns) and, from the first ``forward`` on, on the device."""

    def __init__(self, arrs, nntype):
        if nntype not in NNTYPES:
            raise ValueError("nntype %r: one of %s" % (nntype, sorted(NNTYPES)))
        n_hidden, out_name = NNTYPES[nntype]
        other = [v[1] for k, v in NNTYPES.items() if k != nntype][0]
        key = lambda k: "model/mlp." + k
        if key(out_name + ".weight") not in arrs:
            raise KeyError("%s has no %s: not an %s file%s" % ("the network file", key(out_name + ".weight"), nntype,
                                                               " (it has %s)" % other if key(other + ".weight") in arrs else ""))
        if key(other + ".weight") in arrs:
            raise KeyError("the network file has %s: not an %s file" % (key(other + ".weight"), nntype))
        f32 = lambda k: np.ascontiguousarray(arrs[key(k)], dtype=np.float32)
        self.nntype = nntype
        self.layers = []                                          # (weight [n_out, n_in], bias, ln gain | None, ln bias | None)
        for i in range(1, n_hidden + 1):
            self.layers.append((f32("lin%d.weight" % i), f32("lin%d.bias" % i), f32("ln%d.weight" % i), f32("ln%d.bias" % i)))
        self.layers.append((f32(out_name + ".weight"), f32(out_name + ".bias"), None, None))
        for i, (w, b, g, be) in enumerate(self.layers):
            n_out, n_in = w.shape
            if b.shape != (n_out,) or (g is not None and (g.shape != (n_out,) or be.shape != (n_out,))):
                raise ValueError("layer %d: bias / LayerNorm shapes do not match the weight %s" % (i + 1, w.shape))
            if i and n_in != self.layers[i - 1][0].shape[0]:
                raise ValueError("layer %d takes %d inputs, the layer before gives %d" % (i + 1, n_in, self.layers[i - 1][0].shape[0]))
        # the widths as readNN infers them
        self.D_in = self.layers[0][0].shape[1]
        self.H1, self.H2, self.H3 = (self.layers[i][1].shape[0] for i in range(3))
        self.D_out = self.layers[-1][1].shape[0]
        self._norm = None
        self._handle = None
        self._keep = None
        self._lib = None
        self.device = None

    def set_norm(self, norm_i, norm_o):
        """(mid, std) per input and per output label, applied in fp64 as ``ANN.eval`` does; before the first ``forward``."""
        if self._handle is not None:
            raise RuntimeError("the network is already on the device")
        ni, no = np.asarray(norm_i, dtype=np.float64), np.asarray(norm_o, dtype=np.float64)
        if ni.shape != (self.D_in, 2) or no.shape != (self.D_out, 2):
            raise ValueError("norm_i / norm_o: one (mid, std) pair per label")
        self._norm = tuple(np.ascontiguousarray(a) for a in (ni[:, 0], ni[:, 1], no[:, 0], no[:, 1]))

    def to_device(self, device=None):
        import torch
        if self._handle is not None:
            return self
        self._lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        desc = _lib.LnmlpDesc()
        desc.n_layers = len(self.layers)
        ptr = lambda a: None if a is None else a.ctypes.data
        for i, (w, b, g, be) in enumerate(self.layers):
            L = desc.layers[i]
            L.n_out, L.n_in = w.shape
            L.w, L.b, L.ln_gain, L.ln_bias = ptr(w), ptr(b), ptr(g), ptr(be)
        if self._norm is not None:
            desc.in_mid, desc.in_std, desc.out_mid, desc.out_std = (ptr(a) for a in self._norm)
        h = C.c_void_p()
        rc = self._lib.payne_lnmlp_create(self.device.index, C.byref(desc), C.byref(h))
        if rc == _lib.E_UNSUPPORTED:
            raise ValueError("payne_lnmlp_create: the network is outside the kernel's limits (D_in <= 32, widths <= 512, "
                             "2 to 8 linear layers): %s" % self._lib.payne_last_error(None).decode())
        if rc != 0:
            raise RuntimeError("payne_lnmlp_create failed (%d): %s" % (rc, self._lib.payne_last_error(None).decode()))
        self._handle = h
        return self

    def forward(self, x):
        """x: fp64 [N, D_in], numpy or a tensor (moved to the network's device) -> fp32 device tensor [N, D_out]."""
        import torch
        self.to_device()
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float64)
        if x.dim() != 2 or x.shape[1] != self.D_in:
            raise ValueError("x must be [N, %d], got %s" % (self.D_in, tuple(x.shape)))
        if x.stride(1) != 1 or x.stride(0) < self.D_in:
            x = x.contiguous()
        N = x.shape[0]
        y = torch.empty((N, self.D_out), dtype=torch.float32, device=self.device)
        rc = self._lib.payne_lnmlp_eval(self._handle, x.data_ptr(), x.stride(0), N, y.data_ptr(), y.stride(0),
                                        torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError("payne_lnmlp_eval failed (%d)" % rc)
        return y

    __call__ = forward

    def eval(self):
        return self

    def __del__(self):
        if getattr(self, "_handle", None) is not None and self._lib is not None:
            self._lib.payne_lnmlp_destroy(self._handle)
            self._handle = None


def readNN(nnpath, nntype='MLP_v0'):
    """The network of `nnpath` (a file, or its arrays as a dict) with the widths inferred from the arrays."""
    arrs = nnpath if isinstance(nnpath, dict) else nnio.load_arrays(nnpath)
    return LNMLP(arrs, nntype)


def _labels(a):
    return np.array([x.decode('utf-8') if isinstance(x, bytes) else str(x) for x in np.asarray(a).ravel()])


class ANN(object):
    """photANN_new.ANN: ``label_i``, ``label_o``, with norm=True ``norm_i`` / ``norm_o``, and ``eval``."""

    def __init__(self, nnpath=None, **kwargs):
        super(ANN, self).__init__()
        self.verbose = kwargs.get('verbose', False)
        if nnpath is not None:
            self.nnpath = nnpath
        else:
            raise IOError('... Must provide a path to the ANN model')
        self.norm = kwargs.get('norm', False)
        if self.verbose:
            print('... Reading in {0}'.format(self.nnpath))
        self.nntype = kwargs.get('nntype', 'MLP_v0')              # (the reference's default 'MLP' cannot be read by its own readNN)
        if self.nntype not in NNTYPES:
            raise ValueError("nntype %r: one of %s" % (self.nntype, sorted(NNTYPES)))
        arrs = nnpath if isinstance(nnpath, dict) else nnio.load_arrays(nnpath)
        self.model = readNN(arrs, nntype=self.nntype)
        self.label_i = _labels(arrs['label_i'])
        self.label_o = _labels(arrs['label_o'])
        if len(self.label_i) != self.model.D_in or len(self.label_o) != self.model.D_out:
            raise ValueError("label_i / label_o do not match the network's %d inputs and %d outputs" % (self.model.D_in, self.model.D_out))
        if self.norm:
            self.norm_i = [np.asarray(arrs['norm_i/{0}'.format(kk)], dtype=np.float64) for kk in self.label_i]
            self.norm_o = [np.asarray(arrs['norm_o/{0}'.format(kk)], dtype=np.float64) for kk in self.label_o]
            self.model.set_norm([n[:2] for n in self.norm_i], [n[:2] for n in self.norm_o])
        self._device = kwargs.get('device', None)

    def eval(self, x):
        try:
            import torch
            is_tensor = isinstance(x, torch.Tensor)
        except ImportError:                                       # (only the loader runs without torch)
            is_tensor = False
        if is_tensor:                                             # the batch path: stays on the device
            y = self.model.forward(x.reshape(1, -1) if x.dim() == 1 else x)
            return y.squeeze()
        x_i = np.array(x, dtype=np.float64)                       # a copy: the caller's array is not changed
        if x_i.ndim not in (1, 2):
            raise ValueError("x must be one set of parameters or an [N, %d] array" % self.model.D_in)
        inputD = 1 if x_i.ndim == 1 else x_i.shape[0]
        y = self.model.forward(x_i.reshape(inputD, self.model.D_in))
        return np.asarray(y.cpu().numpy() if hasattr(y, "cpu") else y, dtype=np.float32).squeeze()


class modpred(object):
    """photANN_new.modpred: ``modpararr``, ``pred(inpars)`` and ``getPhot(pars)``."""

    def __init__(self, nnpath=None, nntype='MLP_v0', norm=False, **kwargs):
        super(modpred, self).__init__()
        if nnpath is not None:
            self.nnpath = nnpath
        else:
            raise IOError('... Must provide a path to the ANN model')
        self.norm = norm
        self.anns = ANN(nnpath=self.nnpath, nntype=nntype, norm=self.norm, **kwargs)
        self.modpararr = self.anns.label_o

    def pred(self, inpars):
        return self.anns.eval(inpars)

    def getPhot(self, pars):
        """{input label: value(s)} followed by {output label: prediction(s)}: scalars for a 1-D `pars`, columns for [N, D_in]."""
        pars = np.array(pars, dtype=np.float64)
        pred = np.atleast_1d(self.pred(pars))
        out = {}
        one = pars.ndim == 1
        if not one:
            pred = pred.reshape(pars.shape[0], -1)
        for ii, kk in enumerate(self.anns.label_i):
            out[kk] = pars[ii] if one else pars[:, ii]
        for ii, kk in enumerate(self.anns.label_o):
            out[kk] = pred[ii] if one else pred[:, ii]
        return out
