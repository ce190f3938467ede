"""LinNet / SMLP predictor: mirrors Payne/predict/predictspec.py (ANN, PayneSpecPredict)."""
import numpy as np

from .. import nnio
from ._spec import PayneSpecPredict as _Base, SpecANN, speedoflight  # noqa: F401


class ANN(SpecANN):
    """``ANN(nnpath, NNtype=...)`` of predictspec.py:29-74.  ``testing=True`` also reads the held-out test set the training
    run stored in the file (predictspec.py:51-54): ``testlabels`` [N, n_labels], ``testpred`` [N, npix] and, where the file has
    ``testpred_medflux``, ``testmedflux``."""

    def __init__(self, nnpath=None, **kwargs):
        testing = kwargs.get('testing', False)
        arrs = nnpath
        if testing and not isinstance(nnpath, dict):
            arrs = nnio.load_arrays(nnpath)                       # the file is read once, for the network and the test set
        super(ANN, self).__init__(arrs, kwargs.get('NNtype', 'LinNet'),
                                  **{k: v for k, v in kwargs.items() if k in ('b_max', 'device')})
        self.nnpath = nnpath
        self.inlabels = ['teff', 'logg', 'feh', 'afe'][:self.n_labels]
        if testing:
            for key in ('testlabels', 'testpred'):
                if key not in arrs:
                    raise KeyError("%r is not in the network file: it was written without a test set" % (key,))
            self.testlabels = np.asarray(arrs['testlabels'])
            self.testpred = np.asarray(arrs['testpred'])
            if 'testpred_medflux' in arrs:
                self.testmedflux = np.asarray(arrs['testpred_medflux'])


class PayneSpecPredict(_Base):
    default_NNtype = "LinNet"
