"""Positive semidefinite tensor factorisation on MI355X -- drop-in for `algorithm.psdtf.LDPSDTF` of the reference
(src/algorithm/psdtf.py:12-176).

Same constructor, `psdtf(target, iteration=100, **kwargs) -> (basis.copy(), activation.copy())` for a target of shape
(n_bins, n_bins, n_frames), `basis` (n_bins, n_bins, n_basis) / `activation` (n_basis, n_frames) / `target` / `loss`
attributes, warm start through `hasattr`.  `update_once()` and its parts run as HIP kernels (include/assx.h (f9):
assx_psdtf_*); the loop of `update()` is one call of assx_psdtf_iterate.  There is no CPU fallback.
"""
import numpy as np

from .. import _lib
from .._device import to_numpy, torch
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList

EPS = 1e-12


class PSDTFbase(DeviceState):
    """reference: psdtf.py:12-86.  Kept as it is there: keyword arguments of the call become attributes, `basis` and
    `activation` are drawn from the global RNG unless they exist (diagonal bases from rand(n_basis, n_bins), then
    rand(n_basis, n_frames)), the trace normalisation runs inside `_reset`, and `loss`, created once by the constructor,
    gets one entry per iteration and none before the loop."""
    basis = DeviceArray("V", complex_=False)
    activation = DeviceArray("H", complex_=False)

    N_BINS_MAX = 64
    N_BASIS_MAX = 64
    SYMMETRY_RTOL = 1e-12  # |X - X^T| <= this times max|X|, or the target is refused

    def __init__(self, n_basis=2, normalize=True, eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            n_basis: number of basis
            recordable_loss: extension: False skips the criterion, `loss` then stays empty.
        """
        self._require_float64(dtype)

        self.n_basis = n_basis
        self.normalize = normalize
        self.loss = LazyLossList()
        self.recordable_loss = recordable_loss

        self.eps = eps

        self.dtype = 'float64'
        self.device = device
        self._engine = None

    def __call__(self, target, iteration=100, **kwargs):
        """
        Args:
            target <np.ndarray>: (n_bins, n_bins, n_frames), real symmetric in its first two axes
            iteration <int>: Default: 100
        """
        self.target = target

        self._reset(**kwargs)

        self.update(iteration=iteration)

        V, H = self.basis, self.activation

        return V.copy(), H.copy()

    def _reset(self, **kwargs):
        """Everything of psdtf.py:36-67: the refusals first, then the device, the draws and the normalisation."""
        assert self.target is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        target = self.target
        name = type(self).__name__
        n_basis = self._require_n_basis()
        is_tensor = isinstance(target, torch.Tensor)
        if (target.is_complex() if is_tensor else np.iscomplexobj(target)):
            raise ValueError("{} supports real targets only".format(name))
        shape = self._shape_of(target)
        if len(shape) not in (3, 4):
            raise ValueError("target must be (n_bins, n_bins, n_frames), got {} dims".format(len(shape)))
        n_bins, n_bins2, n_frames = shape[-3:]
        if n_bins != n_bins2:
            raise ValueError("target must be square in its first two axes, got shape {}".format(shape))
        if not 1 <= n_bins <= self.N_BINS_MAX:
            raise ValueError("n_bins must be in [1, {}], got {}".format(self.N_BINS_MAX, n_bins))
        if n_frames < 1 or (len(shape) == 4 and shape[0] < 1):
            raise ValueError("target must not be empty, got shape {}".format(shape))
        # symmetric to rounding: a covariance built by a product may differ from its transpose in the last bits
        t = target if is_tensor else np.asarray(target)
        skew = float(abs(t - (t.transpose(-3, -2) if is_tensor else np.swapaxes(t, -3, -2))).max())
        if not skew <= self.SYMMETRY_RTOL * float(abs(t).max()):
            raise ValueError("{} supports targets that are symmetric in their first two axes only (to {:g} of the "
                             "largest entry)".format(name, self.SYMMETRY_RTOL))
        batched = len(shape) == 4
        lead = (shape[0],) if batched else ()
        a = self._check_warm_start_array("basis", lead + (n_bins, n_bins, n_basis))
        if a is not None and not np.array_equal(a, np.swapaxes(a, -3, -2)):
            raise ValueError("{} supports symmetric bases only".format(name))
        self._check_warm_start_array("activation", lead + (n_basis, n_frames))

        self.is_complex = False

        eng = self._ensure_engine()
        self._batched = batched
        Xd = self._upload(target, eng.prec.real).permute(0, 3, 1, 2)  # (B, T, M, M)
        self._X = ((Xd + Xd.transpose(2, 3)) / 2).contiguous()  # exactly symmetric; an exactly symmetric target is unchanged
        B = int(self._X.shape[0])
        self._ws = eng.psdtf_workspace(B, n_bins, n_frames, n_basis)
        self._status = eng.new_status(B)

        def draw_basis():
            V = np.random.rand(*(lead + (n_basis, n_bins)))  # should be positive semi-definite
            V = V[..., :, np.newaxis] * np.eye(n_bins)
            return np.ascontiguousarray(np.moveaxis(V, -3, -1))

        # basis before activation from the global RNG (psdtf.py:47-59)
        self._keep_or_draw('basis', draw_basis, np.float64)
        self._keep_or_draw('activation', lambda: np.random.rand(*(lead + (n_basis, n_frames))), np.float64)

        if self.normalize:
            V, H = self._model()
            eng.psdtf_normalize(V, H)
            self._touch("V", "H")

    def _model(self):
        """(V (B, K, M, M) contiguous, H (B, K, T)) on the device.  The attribute keeps the reference's (M, M, K) shape: its
        device entry is a permuted view of the matrix-contiguous tensor the kernels work on."""
        v = self._dev("V", False)
        p = v.permute(0, 3, 1, 2)
        if not p.is_contiguous():
            p = p.contiguous()
            self.__dict__["_arrays"]["V"].dev = p.permute(0, 2, 3, 1)
        return p, self._dev("H", False)

    # what DeviceState._check_status raises here: numpy.linalg.cholesky's text, and the eigen-solves can run out of sweeps
    _SINGULAR_TEXT = "Matrix is not positive definite"
    _STATUS_RAISES = _lib.STATUS_SINGULAR | _lib.STATUS_NOT_CONVERGED

    def update(self, iteration=100):
        for idx in range(iteration):
            self.update_once()

            if self.recordable_loss:
                loss = self.compute_loss()
                self.loss.append(loss if self._batched else loss.sum())
        self._check_status()

    def update_once(self):
        raise NotImplementedError("Implement `update_once` method.")

    def compute_loss(self):
        raise NotImplementedError("Implement `compute_loss` method.")


class LDPSDTF(PSDTFbase):
    """reference: psdtf.py:88-176 ("Beyond NMF: Time-Domain Audio Source Separation without Phase Reconstruction", ISMIR
    2013).  float64, real symmetric targets, 1 <= n_bins <= 64, 1 <= n_basis <= 64.  Extensions: a batched target
    (B, n_bins, n_bins, n_frames) whose draws carry a leading B, a torch device tensor as target, `compute_loss()`,
    `reconstruct()` and `recordable_loss`.  A matrix that is not positive definite where the method needs one raises
    numpy.linalg.LinAlgError at the end of `update()` (and of `compute_loss()` / `reconstruct()`), not in the middle.  A
    target that is symmetric to rounding is symmetrised on upload, (X + X^T) / 2."""

    def __init__(self, n_basis=2, algorithm='mm', normalize=True, eps=EPS, *, dtype='float64', device=None,
                 recordable_loss=True):
        super().__init__(n_basis=n_basis, normalize=normalize, eps=eps, dtype=dtype, device=device,
                         recordable_loss=recordable_loss)

        self.algorithm = algorithm

    _OWN_STEPS = ("update", "update_once", "update_once_mm", "update_basis_mm", "update_activation_mm", "compute_loss")

    def _fast_loop_ok(self):
        """DeviceState's rule, and assx_psdtf_iterate is the MM loop."""
        return super()._fast_loop_ok() and self.algorithm == 'mm'

    def update(self, iteration=100):
        if not self._fast_loop_ok():
            return super().update(iteration=iteration)

        if iteration > 0:
            self._iterate_block(iteration, ("V", "H"), lambda loss: self._engine.psdtf_iterate(
                iteration, self._X, *self._model(), self._ws, eps=self.eps, normalize=self.normalize, loss=loss,
                status=self._status))
        self._check_status()

    def update_once(self):
        if self.algorithm == 'mm':
            self.update_once_mm()
        elif self.algorithm == 'em':
            raise NotImplementedError
        else:
            raise ValueError("Not support {} based update.".format(self.algorithm))

        if self.normalize:
            V, H = self._model()
            self._engine.psdtf_normalize(V, H)
            self._touch("V", "H")

    def update_once_mm(self):
        self.update_basis_mm()
        self.update_activation_mm()

    def update_basis_mm(self):
        V, H = self._model()
        self._engine.psdtf_update_basis(self._X, V, H, self._ws, eps=self.eps, status=self._status)
        self._touch("V")

    def update_activation_mm(self):
        V, H = self._model()
        self._engine.psdtf_update_activation(self._X, V, H, eps=self.eps, status=self._status)
        self._touch("H")

    def compute_loss(self):
        """The log-det divergence of to_PSD(sum_k H V_k) from the target, summed over the frames: a float64 scalar, or (B,)
        for a batched target."""
        V, H = self._model()
        loss = to_numpy(self._engine.psdtf_loss(self._X, V, H, self._ws, eps=self.eps, status=self._status), np.float64)
        self._check_status()
        return self._unbatch(loss)

    def reconstruct(self):
        """Extension: sum_k activation * basis, (n_bins, n_bins, n_frames), without to_PSD."""
        Xh = to_numpy(self._engine.psdtf_reconstruct(*self._model()).permute(0, 2, 3, 1), np.float64)
        self._check_status()
        return self._unbatch(Xh)
