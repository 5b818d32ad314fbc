"""Independent positive semidefinite tensor analysis on MI355X -- drop-in for `bss.ipsdta.GaussIPSDTA` and
`bss.ipsdta.tIPSDTA` of the reference with author='Kondo' (src/bss/ipsdta.py:22-355, 510-688, 820-1081, 1083-1762).

Same constructor and call, `ipsdta(input, iteration=100, **kwargs) -> output` for an input of shape (n_channels, n_bins,
n_frames), the attributes `demix_filter` (n_bins, n_sources, n_channels), `basis`, `activation` (n_sources, n_basis,
n_frames), `estimation`, `loss`, warm start through `hasattr`, callbacks before the loop and after every iteration.  `basis`
has the reference's two layouts: one array (n_sources, n_blocks, n_neighbors, n_neighbors, n_basis) when n_blocks divides
n_bins, the tuple (low, high) otherwise.  The MM source model, the VCD spatial model and the loss run as HIP kernels
(include/assx.h (f10): assx_ipsdta_*, (f11): assx_tipsdta_* for the Student-t model); without callbacks the loop is one
call of the model's `iterate` entry point.  There is no CPU fallback.  What the two models share lives in `_BlockDiagonalIPSDTA`, between the
abstract `IPSDTAbase` and the models.

As in the reference, the constructor overwrites its `spatial_iteration` argument with the default of 10 (ipsdta.py:186-190:
the defaults are written after the argument, only `n_blocks` and `spatial_iteration` given as extra keywords -- which Python
refuses for the latter -- would survive); a different number of sweeps is given at the call, `ipsdta(input,
spatial_iteration=2)`, whose keywords become attributes, or by assignment.
"""
import numpy as np

from .. import _lib
from .._device import to_device, to_numpy, torch
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList, append_loss

EPS = 1e-12

__authors_ipsdta__ = ['ikeshita', 'kondo']

__kwargs_kondo_ipsdta__ = {
    'n_blocks': 1024,
    'spatial_iteration': 10
}


def _pack(basis):
    """the reference's basis (array or (low, high)) -> ((N, K, P) packed for the kernels, [(blocks, block size)])"""
    arrs = basis if isinstance(basis, (tuple, list)) else (basis,)
    parts, shapes = [], []
    for a in arrs:
        a = np.asarray(a)
        if a.ndim != 5 or a.shape[2] != a.shape[3]:
            raise ValueError("basis must be (n_sources, n_blocks, n_neighbors, n_neighbors, n_basis), got {}".format(a.shape))
        N, n, nb, _, K = a.shape
        parts.append(np.transpose(a, (0, 4, 1, 2, 3)).reshape(N, K, n * nb * nb))
        shapes.append((n, nb))
    return np.ascontiguousarray(np.concatenate(parts, axis=2), dtype=np.complex128), shapes


def _unpack(packed, shapes):
    N, K, _ = packed.shape
    out, o = [], 0
    for n, nb in shapes:
        part = packed[:, :, o:o + n * nb * nb].reshape(N, K, n, nb, nb)
        out.append(np.ascontiguousarray(np.transpose(part, (0, 2, 3, 4, 1))))
        o += n * nb * nb
    return out[0] if len(out) == 1 else tuple(out)


class IPSDTAbase(DeviceState):
    """reference: ipsdta.py:22-153.  The device side: `demix_filter`, `activation` and `estimation` live in HBM and
    materialise as NumPy arrays on demand; `basis` is kept packed for the kernels and materialises in the reference's
    layout (a fresh array: an edit takes effect when the attribute is assigned, not through an in-place write)."""
    demix_filter = DeviceArray("W", complex_=True)
    activation = DeviceArray("H", complex_=False)
    estimation = DeviceArray("Y", complex_=True)
    _basis_packed = DeviceArray("U", complex_=True)

    N_CHANNELS_MIN, N_CHANNELS_MAX = 2, 8
    N_BASIS_MAX = 64
    BLOCK_MAX = 8

    def __init__(self, n_basis=10, normalize=True, callbacks=None, reference_id=0, recordable_loss=True, eps=EPS, *,
                 dtype='float64', device=None):
        self._require_float64(dtype)
        if callbacks is not None:
            if callable(callbacks):
                callbacks = [callbacks]
            self.callbacks = callbacks
        else:
            self.callbacks = None
        self.reference_id = reference_id
        self.eps = eps

        self.n_basis = n_basis
        self.normalize = normalize

        self.input = None
        self.recordable_loss = recordable_loss
        if self.recordable_loss:
            self.loss = LazyLossList()
        else:
            self.loss = None

        self.dtype = 'float64'
        self.device = device
        self._engine = None

    # ---- basis: packed on the device, the reference's layout outside ---------------------------------------------------
    @property
    def basis(self):
        if not self._has("U"):
            raise AttributeError("'{}' object has no attribute 'basis'".format(type(self).__name__))
        packed = self._basis_packed
        cache = self.__dict__.get("_basis_cache")
        if cache is None or cache[0] is not packed:
            cache = (packed, _unpack(np.asarray(packed), self._basis_shapes))
            self.__dict__["_basis_cache"] = cache
        return cache[1]

    @basis.setter
    def basis(self, value):
        packed, shapes = _pack(value)
        self._basis_shapes = shapes
        self._basis_packed = packed

    @basis.deleter
    def basis(self):
        del self._basis_packed

    def __repr__(self):
        s = "IPSDTA("
        s += "n_basis={n_basis}"
        s += ", normalize={normalize}"
        s += ")"

        return s.format(**self.__dict__)

    def separate(self, input, demix_filter):
        """
        Args:
            input (n_channels, n_bins, n_frames):
            demix_filter (n_bins, n_sources, n_channels):
        Returns:
            output (n_channels, n_bins, n_frames):
        """
        eng = self._ensure_engine()
        X = to_device(input, torch.complex128, eng.dev).unsqueeze(0)
        W = to_device(demix_filter, torch.complex128, eng.dev).unsqueeze(0)
        return to_numpy(eng.demix(X, W)[0], np.complex128)

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' method.")

    def compute_negative_loglikelihood(self):
        raise NotImplementedError("Implement `compute_negative_loglikelihood` method.")


class _BlockDiagonalIPSDTA(IPSDTAbase):
    """What GaussIPSDTA and tIPSDTA (author='Kondo') share: the reset with its refusals, warm start, the call, the stepwise
    methods and the fast loop.  A model names the prefix of its Engine methods (`_OPS`) and what they take beyond the Gauss
    ones (`_model_kwargs`)."""
    _OPS = None  # the prefix of the model's Engine methods

    def _op(self, name):
        return getattr(self._engine, self._OPS + name)

    def _model_kwargs(self):
        """what the model's Engine methods take beyond the Gauss ones"""
        return {}

    def _check_author(self):
        if self.author.lower() == 'ikeshita':
            raise NotImplementedError("author='Ikeshita' is not implemented on the GPU; only author='Kondo' is")
        if self.author.lower() not in __authors_ipsdta__:
            raise ValueError("Not support {}'s IPSDTA".format(self.author))

    def _check_model(self):
        """the model's own refusals, before a device is touched"""

    def __call__(self, input, iteration=100, **kwargs):
        """
        Args:
            input (n_channels, n_bins, n_frames)
        Returns:
            output (n_channels, n_bins, n_frames)
        """
        self.input = input

        self._reset(**kwargs)

        if self.recordable_loss and len(self.loss) == 0:
            append_loss(self.loss, self._loss_device(), False)

        self._run_callbacks()

        if self._fast_loop_ok():  # the rule: DeviceState._fast_loop_ok; the loop is the model's `iterate` entry point
            if iteration > 0:
                self._iterate_block(iteration, ("W", "U", "H"), lambda loss: self._op("iterate")(
                    iteration, self.spatial_iteration, self._X, *self._model(), self._ws, self.n_blocks, eps=self.eps,
                    normalize=self.normalize, loss=None if loss is None else loss.view(-1), status=self._status,
                    **self._model_kwargs()), B=1)
        else:
            for idx in range(iteration):
                self.update_once()

                if self.recordable_loss:
                    append_loss(self.loss, self._loss_device(), False)

                self._run_callbacks()
        self._check_status()

        eng = self._engine
        W = self._dev("W", True)
        X = self._X.unsqueeze(0)
        scale = eng.projection_back_scale(X, W, ref=int(self.reference_id), status=self._status)
        self._check_status()
        self._set_dev("Y", eng.demix(X, W, scale=scale))

        return self.estimation

    _OWN_STEPS = ("update_once", "update_source_model", "update_source_model_mm", "update_basis_mm",
                  "update_activation_mm", "update_spatial_model", "update_spatial_model_vcd", "normalize_psdtf",
                  "normalize_psdtf_block_diagonal", "compute_negative_loglikelihood",
                  "compute_negative_loglikelihood_block_diagonal")

    def _run_callbacks(self):
        if self.callbacks is not None:
            self._check_status()
            for callback in self.callbacks:
                callback(self)

    def _reset(self, **kwargs):
        assert self.input is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        self._check_author()
        self._reset_block_diagonal(**kwargs)

    def _reset_block_diagonal(self, **kwargs):
        """ipsdta.py:248-313: the refusals first, then the device, the draws in the reference's order and the
        normalisation."""
        name = type(self).__name__
        n_basis, n_blocks = self.n_basis, self.n_blocks
        X = self.input
        is_tensor = isinstance(X, torch.Tensor)
        if not (X.is_complex() if is_tensor else np.iscomplexobj(X)):
            raise ValueError("{} needs a complex input (n_channels, n_bins, n_frames)".format(name))
        shape = self._shape_of(X)
        if len(shape) != 3:
            raise ValueError("input must be (n_channels, n_bins, n_frames), got {} dims".format(len(shape)))
        n_channels, n_bins, n_frames = shape
        n_sources = n_channels  # n_channels == n_sources
        if not self.N_CHANNELS_MIN <= n_channels <= self.N_CHANNELS_MAX:
            raise ValueError("n_channels must be in [{}, {}], got {}".format(self.N_CHANNELS_MIN, self.N_CHANNELS_MAX,
                                                                            n_channels))
        if n_bins < 1 or n_frames < 1:
            raise ValueError("input must not be empty, got shape {}".format(shape))
        self._require_n_basis()
        if not isinstance(n_blocks, (int, np.integer)) or not 1 <= n_blocks <= n_bins:
            raise ValueError("n_blocks must be an int in [1, n_bins = {}], got {!r}".format(n_bins, n_blocks))
        if not isinstance(self.spatial_iteration, (int, np.integer)) or self.spatial_iteration < 0:
            raise ValueError("spatial_iteration must be an int >= 0, got {!r}".format(self.spatial_iteration))
        n_basis, n_blocks = int(n_basis), int(n_blocks)
        n_neighbors = n_bins // n_blocks
        n_remains = n_bins % n_blocks
        if n_neighbors + (n_remains > 0) > self.BLOCK_MAX:
            raise ValueError("blocks of at most {} bins are supported, n_bins = {} in n_blocks = {} gives {}".format(
                self.BLOCK_MAX, n_bins, n_blocks, n_neighbors + (n_remains > 0)))
        if not 0 <= int(self.reference_id) < n_channels:
            raise ValueError("reference_id must be in [0, {}), got {!r}".format(n_channels, self.reference_id))
        self._check_model()

        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames
        self.n_blocks, self.n_neighbors = n_blocks, n_neighbors
        self.n_remains = n_remains
        shapes = [(n_blocks - n_remains, n_neighbors)] + ([(n_remains, n_neighbors + 1)] if n_remains > 0 else [])

        if hasattr(self, 'demix_filter'):
            W = np.array(self.demix_filter, dtype=np.complex128)
            if W.shape != (n_bins, n_sources, n_channels):
                raise ValueError("demix_filter has shape {}, the input needs {}".format(W.shape,
                                                                                     (n_bins, n_sources, n_channels)))
        else:
            W = np.tile(np.eye(n_sources, n_channels, dtype=np.complex128), reps=(n_bins, 1, 1))
        if hasattr(self, 'basis'):
            packed, got = _pack(self.basis)
            if got != shapes or packed.shape[:2] != (n_sources, n_basis):
                raise ValueError("basis does not fit n_sources = {}, n_basis = {}, n_bins = {} in n_blocks = {}".format(
                    n_sources, n_basis, n_bins, n_blocks))
        else:
            packed = None
        if hasattr(self, 'activation'):
            H = np.array(self.activation, dtype=np.float64)
            if H.shape != (n_sources, n_basis, n_frames):
                raise ValueError("activation has shape {}, the input needs {}".format(H.shape,
                                                                                   (n_sources, n_basis, n_frames)))
        else:
            H = None

        self.is_complex = True
        eng = self._ensure_engine()
        self._X = to_device(X, torch.complex128, eng.dev)
        self._ws = self._op("workspace")(n_channels, n_bins, n_frames, n_basis, n_blocks, **self._model_kwargs())
        self._status = eng.new_status(1)

        self.demix_filter = W
        self._set_dev("Y", eng.demix(self._X.unsqueeze(0), self._dev("W", True)))

        if packed is None:
            # real diagonals in complex storage: U_low draws, then U_high draws (one draw without remains)
            draws = [np.random.rand(n_sources, n_basis, n, nb) for n, nb in shapes]
            self.basis = tuple(np.ascontiguousarray((d[..., np.newaxis] * np.eye(nb, dtype=np.complex128))
                                                    .transpose(0, 2, 3, 4, 1)) for d, (n, nb) in zip(draws, shapes))
        else:
            self._basis_shapes = shapes
            self._basis_packed = packed
        self.activation = np.random.rand(n_sources, n_basis, n_frames) if H is None else H

        if self.normalize:
            self.normalize_psdtf()

    def _model(self):
        """(W (F, M, M), U (N, K, P), H (N, K, T)) on the device"""
        return self._dev("W", True)[0], self._dev("U", True)[0], self._dev("H", False)[0]

    def update_once(self):
        self.update_source_model()

        cls = type(self)
        if cls.update_spatial_model is not _BlockDiagonalIPSDTA.update_spatial_model \
                or cls.update_spatial_model_vcd is not _BlockDiagonalIPSDTA.update_spatial_model_vcd:
            for spatial_idx in range(self.spatial_iteration):
                self.update_spatial_model()
            return

        # all sweeps in one call: R^-1 (and Q in the Gauss model) depend on the source model alone and are computed once
        W, U, H = self._model()
        self._op("update_spatial")(self._X, W, U, H, self._ws, self.n_blocks, n_sweeps=self.spatial_iteration, eps=self.eps,
                                   status=self._status, **self._model_kwargs())
        self._touch("W")

    def update_source_model(self):
        algorithm_source = self.algorithm_source

        if algorithm_source == 'mm':
            self.update_source_model_mm()
        else:
            raise NotImplementedError("Not support {}'s IPSDTA.".format(self.author))

        if self.normalize:
            self.normalize_psdtf()

    def update_spatial_model(self):
        algorithm_spatial = self.algorithm_spatial

        if algorithm_spatial == 'vcd':
            self.update_spatial_model_vcd()
        else:
            raise NotImplementedError("Not support {}-based spatial model updates.".format(algorithm_spatial))

    def update_source_model_mm(self):
        self.update_basis_mm()
        self.update_activation_mm()

    def update_basis_mm(self):
        W, U, H = self._model()
        self._op("update_basis")(self._X, W, U, H, self._ws, self.n_blocks, eps=self.eps, status=self._status,
                                 **self._model_kwargs())
        self._touch("U")

    def update_activation_mm(self):
        W, U, H = self._model()
        self._op("update_activation")(self._X, W, U, H, self._ws, self.n_blocks, eps=self.eps, status=self._status,
                                      **self._model_kwargs())
        self._touch("H")

    def update_spatial_model_vcd(self):
        """one VCD sweep"""
        W, U, H = self._model()
        self._op("update_spatial")(self._X, W, U, H, self._ws, self.n_blocks, n_sweeps=1, eps=self.eps, status=self._status,
                                   **self._model_kwargs())
        self._touch("W")

    def normalize_psdtf(self):
        self.normalize_psdtf_block_diagonal()

    def normalize_psdtf_block_diagonal(self):
        _, U, H = self._model()
        self._engine.ipsdta_normalize(U, H, self.n_bins, self.n_blocks)
        self._touch("U", "H")

    def _loss_device(self):
        W, U, H = self._model()
        return self._op("loss")(self._X, W, U, H, self._ws, self.n_blocks, eps=self.eps, status=self._status,
                                **self._model_kwargs())

    def compute_negative_loglikelihood(self):
        return self.compute_negative_loglikelihood_block_diagonal()

    def compute_negative_loglikelihood_block_diagonal(self):
        loss = np.float64(self._loss_device().item())
        self._check_status()
        return loss


class GaussIPSDTA(_BlockDiagonalIPSDTA):
    """reference: ipsdta.py:155-1081 with author='Kondo' ("Convergence-Guaranteed Independent Positive Semidefinite Tensor
    Analysis Based on Student's t Distribution", ICASSP 2020, for the MM and VCD updates).  float64 / complex128, one
    utterance, 2 <= n_channels <= 8 with n_sources = n_channels, 1 <= n_basis <= 64, 1 <= n_blocks <= n_bins, blocks of at
    most 8 bins; anything else raises ValueError before a kernel is launched.  author='Ikeshita' (EM and fixed-point) is not
    implemented.  A block that is not positive definite where the method inverts it raises numpy.linalg.LinAlgError at the
    end of the call (and of the stand-alone steps), not in the middle."""
    _OPS = "ipsdta_"

    def __init__(self, n_basis=10, spatial_iteration=None, normalize=True, callbacks=None, reference_id=0, author='Kondo',
                 recordable_loss=True, eps=EPS, dtype='float64', device=None, **kwargs):
        """
        Args:
            n_basis <int>: Number of basis matrices
            callbacks <callable> or <list<callable>>:
            reference_id <int>: Reference microphone index
            author <str>: 'Kondo' ('Ikeshita' raises NotImplementedError)
        """
        super().__init__(n_basis=n_basis, normalize=normalize, callbacks=callbacks, reference_id=reference_id,
                         recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)

        self.spatial_iteration = spatial_iteration
        self.author = author

        if author.lower() in __authors_ipsdta__:
            if author.lower() == 'ikeshita':
                raise NotImplementedError("author='Ikeshita' (EM source model, fixed-point spatial model) is not implemented "
                                          "on the GPU; only author='Kondo' is")
            if set(kwargs) - set(__kwargs_kondo_ipsdta__) != set():
                raise ValueError("Invalid keywords.")
            for key in __kwargs_kondo_ipsdta__.keys():
                setattr(self, key, __kwargs_kondo_ipsdta__[key])
            self.algorithm_source = 'mm'
            self.algorithm_spatial = 'vcd'
            for key in kwargs.keys():
                setattr(self, key, kwargs[key])
        else:
            raise ValueError("Not support {}'s IPSDTA".format(author))

    def __repr__(self):
        s = "Gauss-IPSDTA("
        s += "n_basis={n_basis}"
        s += ", normalize={normalize}"
        s += ", algorithm(source)={algorithm_source}"
        s += ", algorithm(spatial)={algorithm_spatial}"
        if self.author.lower() in __authors_ipsdta__:
            s += ", n_blocks={n_blocks}"
        s += ", author={author}"
        s += ")"

        return s.format(**self.__dict__)


class tIPSDTA(_BlockDiagonalIPSDTA):
    """reference: ipsdta.py:1083-1762 ("Convergence-Guaranteed Independent Positive Semidefinite Tensor Analysis Based on
    Student's t Distribution", ICASSP 2020): GaussIPSDTA's envelope, refusals and stepwise methods, with every update
    weighted per (source, frame) through the degree of freedom `nu` (finite and > 0).  The kernels are assx_tipsdta_* of
    include/assx.h (f11); the normalisation is the Gauss one.  Any author but 'Kondo' raises ValueError, as in the
    reference."""
    _OPS = "tipsdta_"

    def __init__(self, n_basis=10, nu=1, spatial_iteration=None, normalize=True, callbacks=None, reference_id=0, author='Kondo',
                 recordable_loss=True, eps=EPS, dtype='float64', device=None, **kwargs):
        """
        Args:
            nu <float>: Degree of freedom
            author <str>: 'Kondo'
        """
        super().__init__(n_basis=n_basis, normalize=normalize, callbacks=callbacks, reference_id=reference_id,
                         recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)

        self.nu = nu
        self.spatial_iteration = spatial_iteration
        self.author = author

        if author.lower() == 'kondo':
            if set(kwargs) - set(__kwargs_kondo_ipsdta__) != set():
                raise ValueError("Invalid keywords.")
            for key in __kwargs_kondo_ipsdta__.keys():
                setattr(self, key, __kwargs_kondo_ipsdta__[key])
            self.algorithm_source = 'mm'
            self.algorithm_spatial = 'vcd'
        else:
            raise ValueError("Not support {}'s IPSDTA".format(author))

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

    def _model_kwargs(self):
        return {"nu": float(self.nu)}

    def _check_author(self):
        if self.author.lower() != 'kondo':
            raise ValueError("Not support {}'s IPSDTA".format(self.author))

    def _check_model(self):
        nu = self.nu
        if isinstance(nu, bool) or not isinstance(nu, (int, float, np.integer, np.floating)) or not 0 < nu < np.inf:
            raise ValueError("nu must be a finite number > 0, got {!r}".format(nu))

    def __repr__(self):
        s = "t-IPSDTA("
        s += "n_basis={n_basis}"
        s += ", nu={nu}"
        s += ", normalize={normalize}"
        s += ", algorithm(source)={algorithm_source}"
        s += ", algorithm(spatial)={algorithm_spatial}"
        if self.author.lower() in __authors_ipsdta__:
            s += ", n_blocks={n_blocks}"
        s += ", author={author}"
        s += ")"

        return s.format(**self.__dict__)
