"""Gradient and natural-gradient Laplace FDICA on MI355X -- drop-in for `bss.fdica.GradLaplaceFDICA` and
`bss.fdica.NaturalGradLaplaceFDICA` of the reference (src/bss/fdica.py:8-301).

One iteration is ONE sweep over X on the device: y = W x in registers, the score y / max(|y|, eps), the N x M
cross-moment per bin, and a per-bin step; the data term of the loss rides on the same sweep.  After
the loop `solve_permutation` (fdica.py:106-138) runs on the device too: the bins in ascending order of their
correlation, one N x N matrix per bin for the N! candidates.  float64, one utterance, 2 <= n_channels <= 8.  There is no
CPU fallback.
"""
import numpy as np

from .._device import to_numpy, torch  # noqa: F401
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList
from .. import _lib
from .iva import GradSteps, IVAbase

EPS = 1e-12


class FDICAbase(DeviceState):
    """reference: fdica.py:8-141"""

    demix_filter = DeviceArray("W", complex_=True)

    def __init__(self, callbacks=None, recordable_loss=True, eps=EPS, *, dtype='float64', device=None):
        if callbacks is not None:
            if callable(callbacks):
                callbacks = [callbacks]
            self.callbacks = callbacks
        else:
            self.callbacks = None
        self.eps = eps

        self.input = None
        self.criterion = None
        self.recordable_loss = recordable_loss
        if self.recordable_loss:
            self.loss = LazyLossList()  # a list; entries are materialised from HBM on first read
        else:
            self.loss = None

        self.dtype = dtype
        self.device = device
        self._engine = None
        self._estimation = None

    _Wd = IVAbase._Wd
    estimation = IVAbase.estimation
    separate = IVAbase.separate  # y = W x on the device (fdica.py:92-104)

    def __repr__(self) -> str:
        s = "FDICA("
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        raise NotImplementedError("Implement 'update' function")

    def solve_permutation(self):
        """fdica.py:106-138 on the device; the rows of `demix_filter` are permuted in place.  `permutation_order`
        (n_bins,) and `permutation` (n_bins, n_sources) keep what was chosen (device tensors, int32)."""
        order, perm = self._engine.fdica_solve_permutation(self._X[0], self._Wd[0], self._ws, eps=self.eps)
        self.permutation_order, self.permutation = order, perm
        self._touch("W")
        self._estimation = None

    def compute_negative_loglikelihood(self):
        raise NotImplementedError("Implement 'compute_negative_loglikelihood' function.")


class GradFDICAbase(GradSteps, FDICAbase):
    """reference: fdica.py:144-201"""

    _MODEL = _lib.GRADBSS_FDICA
    _MAX_BINS = 1 << 16  # assx_fdica_solve_permutation ranks the bins by counting

    def __init__(self, lr=1e-1, reference_id=0, callbacks=None, recordable_loss=True, eps=EPS, *, dtype='float64',
                 device=None):
        super().__init__(callbacks=callbacks, recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)
        self._require_float64(dtype, complex_ok=True)

        self.lr = lr
        self.reference_id = reference_id

    def __call__(self, input, iteration=100, **kwargs):
        """
        Args:
            input (n_channels, n_bins, n_frames)
        Returns:
            output (n_channels, n_bins, n_frames)
        """
        self.input = input

        self._reset(**kwargs)
        self._loop(iteration)

        self.solve_permutation()

        return self._output(input, True)

    def __repr__(self) -> str:
        s = "GradFDICA("
        s += "lr={lr}"
        s += ")"

        return s.format(**self.__dict__)

    def compute_negative_loglikelihood(self):
        raise NotImplementedError("Implement 'compute_negative_loglikelihood' function.")


class GradLaplaceFDICA(GradFDICAbase):
    """reference: fdica.py:203-247"""
    _NATURAL = False
    _OWN_STEPS = ("update_once", "compute_negative_loglikelihood", "_record_loss")

    def __init__(self, lr=1e-1, reference_id=0, callbacks=None, recordable_loss=True, eps=EPS, *, dtype='float64',
                 device=None):
        super().__init__(lr=lr, reference_id=reference_id, callbacks=callbacks, recordable_loss=recordable_loss, eps=eps,
                         dtype=dtype, device=device)

    def update_once(self):
        """fdica.py:207-231: W <- W - lr ((1/T) sum_t phi x^H - W^-H)."""
        self._grad_update()

    def __repr__(self) -> str:
        s = "GradLaplaceFDICA("
        s += "lr={lr}"
        s += ")"

        return s.format(**self.__dict__)

    def compute_negative_loglikelihood(self):
        """fdica.py:240-247.  Syncs to return a Python float."""
        return self._grad_loss()


class NaturalGradLaplaceFDICA(GradFDICAbase):
    """reference: fdica.py:249-301"""
    _NATURAL = True
    _OWN_STEPS = ("update_once", "compute_negative_loglikelihood", "_record_loss")

    def __init__(self, lr=1e-1, reference_id=0, is_holonomic=True, callbacks=None, recordable_loss=True, eps=EPS, *,
                 dtype='float64', device=None):
        super().__init__(lr=lr, reference_id=reference_id, callbacks=callbacks, recordable_loss=recordable_loss, eps=eps,
                         dtype=dtype, device=device)

        self.is_holonomic = is_holonomic

    def __repr__(self) -> str:
        s = "GradLaplaceFDICA("
        s += "lr={lr}"
        s += ", is_holonomic={is_holonomic}"
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        """fdica.py:263-292: W <- W - lr ((1/T) sum_t phi y^H - I) W."""
        if not self.is_holonomic:
            raise NotImplementedError("only suports for is_holonomic = True")
        self._grad_update()

    def compute_negative_loglikelihood(self):
        """fdica.py:294-301.  Syncs to return a Python float."""
        return self._grad_loss()
