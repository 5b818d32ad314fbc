"""Non-negative tensor factorisation on MI355X -- drop-in for `algorithm.ntf.EUCNTF` of the reference
(src/algorithm/ntf.py:8-102).

Same constructor, `ntf(target, iteration=100) -> (partitioning.copy(), basis.copy(), activation.copy())` for a target
of shape (n_channels, n_bins, n_frames), `partitioning` / `basis` / `activation` / `target` / `loss` / `n_basis`
attributes.  `update_once()` and `compute_loss()` run as HIP kernels (include/assx.h: assx_ntf_update / assx_ntf_loss);
the loop of `update()` is one call of assx_ntf_iterate.  There is no CPU fallback.
"""
import numpy as np

from .._device import to_numpy
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList

EPS = 1e-12


class NTFbase(DeviceState):
    """reference: ntf.py:8-48.  Kept as it is there: `update` takes the target, draws the three factors from the global
    RNG on every call (no warm start, no keyword attributes), and `loss`, created once by the constructor, gets one
    entry per iteration and none before the loop."""
    partitioning = DeviceArray("Z", complex_=False)
    basis = DeviceArray("T", complex_=False)
    activation = DeviceArray("V", complex_=False)

    N_BASIS_MAX = 64
    N_CHANNELS_MAX = 32

    def __init__(self, n_basis=2, eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            n_basis: number of basis
            recordable_loss: extension: False skips the criterion, `loss` then stays empty.
        """
        self._require_float64(dtype)

        self.n_basis = n_basis
        self.loss = LazyLossList()
        self.recordable_loss = recordable_loss

        self.eps = eps

        self.dtype = 'float64'
        self.device = device
        self._engine = None

    def __call__(self, *args, **kwargs):
        self.update(*args, **kwargs)
        Z, T, V = self.partitioning, self.basis, self.activation

        return Z.copy(), T.copy(), V.copy()

    def _reset(self, target):
        """Everything of ntf.py:27-35 before the loop: the refusals first, then the device, then the three draws."""
        n_basis = self._require_n_basis()
        shape = self._shape_of(target)
        if len(shape) not in (3, 4):
            raise ValueError("target must be (n_channels, n_bins, n_frames), got {} dims".format(len(shape)))
        n_channels, n_bins, n_frames = shape[-3:]
        if not 1 <= n_channels <= self.N_CHANNELS_MAX:
            raise ValueError("n_channels must be in [1, {}], got {}".format(self.N_CHANNELS_MAX, n_channels))
        if n_bins < 1 or n_frames < 1 or (len(shape) == 4 and shape[0] < 1):
            raise ValueError("target must not be empty, got shape {}".format(shape))

        self.target = target

        eng = self._ensure_engine()
        self._batched = len(shape) == 4
        self._X = self._upload(target, eng.prec.real)
        B = int(self._X.shape[0])
        self._ws = eng.ntf_workspace(B, n_channels, n_bins, n_frames, n_basis)

        lead = (B,) if self._batched else ()
        self.partitioning = np.random.rand(*(lead + (n_channels, n_basis)))
        self.basis = np.random.rand(*(lead + (n_bins, n_basis)))
        self.activation = np.random.rand(*(lead + (n_basis, n_frames)))

    def update(self, target, iteration=100):
        self._reset(target)

        for idx in range(iteration):
            self.update_once()

            if self.recordable_loss:
                loss = self.compute_loss()
                self.loss.append(loss if self._batched else loss.sum())

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' method")

    def compute_loss(self):
        raise NotImplementedError("Implement 'compute_loss' method")


class EUCNTF(NTFbase):
    """reference: ntf.py:50-102.  float64, 1 <= n_basis <= 64, 1 <= n_channels <= 32.  Extensions: a batched target
    (B, n_channels, n_bins, n_frames) whose draws carry a leading B, a torch device tensor as target, `reconstruct()`
    and `recordable_loss`."""

    def __init__(self, n_basis, eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

    def __call__(self, *args, **kwargs):
        return super().__call__(*args, **kwargs)

    def _model(self):
        return self._dev("Z", False), self._dev("T", False), self._dev("V", False)

    _OWN_STEPS = ("update", "update_once", "compute_loss")

    def update(self, target, iteration=100):
        if not self._fast_loop_ok():  # the rule: DeviceState._fast_loop_ok; the loop is assx_ntf_iterate
            return super().update(target, iteration=iteration)

        self._reset(target)
        if iteration > 0:
            self._iterate_block(iteration, ("Z", "T", "V"), lambda loss: self._engine.ntf_iterate(
                iteration, self._X, *self._model(), self._ws, eps=self.eps, loss=loss))

    def update_once(self):
        Z, T, V = self._model()
        self._engine.ntf_update(self._X, Z, T, V, self._ws, eps=self.eps)
        self._touch("Z", "T", "V")

    def compute_loss(self):
        """sum (X - X_hat)^2: a float64 scalar, or (B,) for a batched target."""
        Z, T, V = self._model()
        return self._unbatch(to_numpy(self._engine.ntf_loss(self._X, Z, T, V, self._ws), np.float64))

    def reconstruct(self):
        """Extension: sum_k partitioning * basis * activation, (n_channels, n_bins, n_frames)."""
        return self._unbatch(to_numpy(self._engine.ntf_reconstruct(*self._model()), np.float64))
