"""NMF by multiplicative updates on MI355X -- drop-in for `algorithm.nmf.EUCNMF / KLNMF / ISNMF / tNMF / CauchyNMF`
of the reference (/root/reference/src/algorithm/nmf.py:10-56, 150-600).

Same constructors, `nmf(target, iteration=100, **kwargs) -> (basis.copy(), activation.copy())`,
`basis` / `activation` / `loss` attributes.  `update_once()` and the per-iteration loss run as HIP
kernels (include/assx.h: assx_nmf_update / assx_nmf_loss); there is no CPU fallback.

`ComplexEUCNMF` (nmf.py:58-114, 597-676) returns `(basis.copy(), activation.copy(), phase.copy())` and runs on
assx_cnmf_update / assx_cnmf_iterate.

`MultichannelISNMF` (nmf.py:116-148, 678-815), multichannel IS-NMF on a tensor of Hermitian covariance matrices, returns
`(spatial.copy(), basis.copy(), activation.copy())` and runs on assx_covnmf_* (include/assx.h (f12)).
"""
import numpy as np

from .._device import to_device, to_numpy, torch
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList, append_loss
from .. import _lib
from ..ops import Engine

EPS = 1e-12

__metrics__ = ['EUC', 'KL', 'IS']


class NMFbase(DeviceState):
    basis = DeviceArray("T", complex_=False)
    activation = DeviceArray("V", complex_=False)

    _KIND = None

    def __init__(self, n_basis=2, eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            n_basis: number of basis
            recordable_loss: extension (the reference always evaluates the criterion after every update,
                nmf.py:48-53): False skips that pass, `loss` then stays empty.
        """

        self.n_basis = n_basis
        self.loss = LazyLossList()  # a list; entries are materialised from HBM on first read
        self.recordable_loss = recordable_loss

        self.eps = eps
        self.domain = 2

        self.dtype = dtype
        self.device = device
        self._engine = None

    def __call__(self, target, iteration=100, **kwargs):
        self.target = target

        self._reset(**kwargs)

        self.update(iteration=iteration)

        T, V = self.basis, self.activation

        return T.copy(), V.copy()

    def _reset(self, **kwargs):
        assert self.target is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        if self._engine is None:
            self._engine = Engine(dtype=self.dtype, device=self.device)
        eng = self._engine

        n_basis = self.n_basis
        target = self.target
        ndim = len(self._shape_of(target))
        if ndim not in (2, 3):
            raise ValueError("target must be (n_bins, n_frames), got {} dims".format(ndim))
        self._batched = ndim == 3
        self._X = self._upload(target, eng.prec.real)
        B, n_bins, n_frames = (int(s) for s in self._X.shape)

        # NMF never warm-starts: fresh draws from the global RNG, basis first (nmf.py:36-43)
        lead = (B,) if self._batched else ()
        self.basis = np.random.rand(*(lead + (n_bins, n_basis)))
        self.activation = np.random.rand(*(lead + (n_basis, n_frames)))

    def _kind_code(self):
        if self._KIND is None:
            raise NotImplementedError("Implement 'update_once' function")
        return self._KIND

    def _kind_param(self):
        return 0.0

    _OWN_STEPS = ("update", "update_once", "_record_loss")

    def _record_loss(self):
        loss = self._engine.nmf_loss(self._kind_code(), self._X, self._dev("T", False), self._dev("V", False),
                                     domain=self.domain, eps=self.eps, param=self._kind_param())
        append_loss(self.loss, loss, self._batched)

    def update(self, iteration=100):
        if iteration > 1 and self._fast_loop_ok():  # the rule: DeviceState._fast_loop_ok
            # the first update through update_once(): it validates `algorithm` / `domain` and raises exactly what the
            # reference raises; the remaining ones are enqueued by the library (same entry points, same order)
            self.update_once()
            if self.recordable_loss:
                self._record_loss()
            n = iteration - 1
            self._iterate_block(n, ("T", "V"), lambda loss: self._engine.nmf_iterate(
                n, self._kind_code(), self._X, self._dev("T", False), self._dev("V", False), domain=self.domain,
                eps=self.eps, param=self._kind_param(), loss=loss))
            return

        for idx in range(iteration):
            self.update_once()

            if self.recordable_loss:
                self._record_loss()

    def update_once(self):
        self._engine.nmf_update(self._kind_code(), self._X, self._dev("T", False), self._dev("V", False),
                                domain=self.domain, eps=self.eps, param=self._kind_param())
        self._touch("T", "V")


class EUCNMF(NMFbase):
    """reference: nmf.py:150-207"""
    _KIND = _lib.NMF_EUC

    def __init__(self, n_basis=2, domain=2, algorithm='mm', eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            n_basis: number of basis
        """
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

        assert 1 <= domain <= 2, "1 <= `domain` <= 2 is not satisfied."
        assert algorithm == 'mm', "algorithm must be 'mm'."

        self.domain = domain
        self.algorithm = algorithm

    def update_once(self):
        if self.algorithm == 'mm':
            self.update_once_mm()
        else:
            raise ValueError("Not support {} based update.".format(self.algorithm))

    def update_once_mm(self):
        NMFbase.update_once(self)

    _OWN_STEPS = NMFbase._OWN_STEPS + ("update_once_mm",)


class KLNMF(NMFbase):
    """reference: nmf.py:209-266"""
    _KIND = _lib.NMF_KL

    def __init__(self, n_basis=2, domain=2, algorithm='mm', eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            K: number of basis
        """
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

        assert 1 <= domain <= 2, "1 <= `domain` <= 2 is not satisfied."
        assert algorithm == 'mm', "algorithm must be 'mm'."

        self.domain = domain
        self.algorithm = algorithm

    def update_once(self):
        if self.algorithm == 'mm':
            self.update_once_mm()
        else:
            raise ValueError("Not support {} based update.".format(self.algorithm))

    def update_once_mm(self):
        NMFbase.update_once(self)

    _OWN_STEPS = NMFbase._OWN_STEPS + ("update_once_mm",)


class ISNMF(NMFbase):
    """reference: nmf.py:268-356"""
    _KIND = _lib.NMF_IS_MM

    def __init__(self, n_basis=2, domain=2, algorithm='mm', eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            K: number of basis
            algorithm: 'mm': MM algorithm based update
        """
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

        assert 1 <= domain <= 2, "1 <= `domain` <= 2 is not satisfied."

        self.domain = domain
        self.algorithm = algorithm

    def _kind_code(self):
        return _lib.NMF_IS_ME if self.algorithm == 'me' else _lib.NMF_IS_MM

    def update_once(self):
        if self.algorithm == 'mm':
            self.update_once_mm()
        elif self.algorithm == 'me':
            self.update_once_me()
        else:
            raise ValueError("Not support {} based update.".format(self.algorithm))

    def update_once_mm(self):
        NMFbase.update_once(self)

    def update_once_me(self):
        assert self.domain == 2, "Only domain = 2 is supported."
        NMFbase.update_once(self)

    _OWN_STEPS = NMFbase._OWN_STEPS + ("update_once_mm", "update_once_me")


class tNMF(NMFbase):
    """reference: nmf.py:358-429 (Student's t NMF, MM update; domain 2 only)"""
    _KIND = _lib.NMF_T

    def __init__(self, n_basis=2, nu=1e+3, domain=2, algorithm='mm', eps=EPS, *, dtype='float64', device=None,
                 recordable_loss=True):
        """
        Args:
            K: number of basis
            algorithm: 'mm': MM algorithm based update
        """
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

        assert 1 <= domain <= 2, "1 <= `domain` <= 2 is not satisfied."

        self.nu = nu
        self.domain = domain
        self.algorithm = algorithm

    def _kind_param(self):
        return float(self.nu)

    def update_once(self):
        if self.algorithm == 'mm':
            self.update_once_mm()
        else:
            raise ValueError("Not support {} based update.".format(self.algorithm))

    def update_once_mm(self):
        assert self.domain == 2, "`domain` is expected 2."
        NMFbase.update_once(self)

    _OWN_STEPS = NMFbase._OWN_STEPS + ("update_once_mm",)


class CauchyNMF(NMFbase):
    """reference: nmf.py:431-600 ('naive-multipricative', 'mm', 'me', 'mm_fast'; domain 2 only)"""
    _ALGORITHMS = {'naive-multipricative': _lib.NMF_CAUCHY_NAIVE, 'mm': _lib.NMF_CAUCHY_MM,
                   'me': _lib.NMF_CAUCHY_ME, 'mm_fast': _lib.NMF_CAUCHY_MM_FAST}

    def __init__(self, n_basis, domain=2, algorithm='naive-multipricative', eps=EPS, *, dtype='float64', device=None,
                 recordable_loss=True):
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

        assert domain == 2, "Only `domain` = 2 is supported."

        self.domain = domain
        self.algorithm = algorithm

    def _kind_code(self):
        if self.algorithm not in self._ALGORITHMS:
            raise ValueError("Not support {} based update.".format(self.algorithm))
        return self._ALGORITHMS[self.algorithm]

    def update_once(self):
        if self.algorithm == 'naive-multipricative':
            self.update_once_naive()
        elif self.algorithm == 'mm':
            self.update_once_mm()
        elif self.algorithm == 'me':
            self.update_once_me()
        elif self.algorithm == 'mm_fast':
            self.update_once_mm_fast()
        else:
            raise ValueError("Not support {} based update.".format(self.algorithm))

    def _update_once_checked(self):
        assert self.domain == 2, "Only 'domain' = 2 is supported."
        NMFbase.update_once(self)

    update_once_naive = update_once_mm = update_once_me = update_once_mm_fast = _update_once_checked

    _OWN_STEPS = NMFbase._OWN_STEPS + ("update_once_naive", "update_once_mm", "update_once_me", "update_once_mm_fast")


class ComplexNMFbase(DeviceState):
    """reference: nmf.py:58-114.  `phase` holds the angles (n_bins, n_basis, n_frames), as in the reference."""
    basis = DeviceArray("T", complex_=False)
    activation = DeviceArray("V", complex_=False)
    phase = DeviceArray("Phi", complex_=False)

    N_BASIS_MAX = 64

    def __init__(self, n_basis=2, regularizer=0.1, eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            n_basis: number of basis
            recordable_loss: extension: False skips the criterion, `loss` then stays empty.
        """
        self._require_float64(dtype, complex_ok=True)

        self.n_basis = n_basis
        self.regularizer = regularizer
        self.loss = LazyLossList()
        self.recordable_loss = recordable_loss

        self.eps = eps

        self.dtype = 'float64'
        self.device = device
        self._engine = None

    def __call__(self, target, iteration=100, **kwargs):
        self.target = target

        self._reset(**kwargs)

        self.update(iteration=iteration)

        T, V = self.basis, self.activation
        Phi = self.phase

        return T.copy(), V.copy(), Phi.copy()

    def _reset(self, **kwargs):
        assert self.target is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        n_basis = self._require_n_basis()
        target = self.target
        ndim = len(self._shape_of(target))
        if ndim not in (2, 3):
            raise ValueError("target must be (n_bins, n_frames), got {} dims".format(ndim))

        eng = self._ensure_engine()
        self._batched = ndim == 3
        self._X = self._upload(target, eng.prec.cplx)
        B, n_bins, n_frames = (int(s) for s in self._X.shape)
        self._ws = eng.cnmf_workspace(B, n_bins, n_frames, n_basis)

        # no warm start: three draws from the global RNG, in the reference's order (nmf.py:92-94)
        lead = (B,) if self._batched else ()
        self.basis = np.random.rand(*(lead + (n_bins, n_basis)))
        self.activation = np.random.rand(*(lead + (n_basis, n_frames)))
        self.phase = 2 * np.pi * np.random.rand(*(lead + (n_bins, n_basis, n_frames)))

    def init_phase(self):
        """nmf.py:96-101: every basis starts from the target's phase.  A NumPy target is handled on the host, like the
        reference's; a device tensor stays on the device."""
        n_basis = self.n_basis
        target = self.target

        if isinstance(target, torch.Tensor):
            phase = torch.angle(self._X)
            self._set_dev("Phi", phase.unsqueeze(2).expand(-1, -1, n_basis, -1).contiguous())
        else:
            phase = np.angle(target)
            self.phase = np.tile(phase[..., np.newaxis, :], reps=(1,) * (phase.ndim - 1) + (n_basis, 1))

    def _model(self):
        return self._dev("T", False), self._dev("V", False), self._dev("Phi", False)

    def reconstruct(self):
        """Extension: sum_k basis * activation * exp(1j * phase), (n_bins, n_frames) complex -- what the reference's
        users form next (egs/nmf-example/cnmf)."""
        return self._unbatch(to_numpy(self._engine.cnmf_reconstruct(*self._model()), np.complex128))

    def update(self, iteration=100):
        for idx in range(iteration):
            self.update_once()

            if self.recordable_loss:
                self._record_loss()

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' method")


class ComplexEUCNMF(ComplexNMFbase):
    """reference: nmf.py:597-676 (Kameoka's complex NMF).  float64, 1 <= n_basis <= 64.  `Beta` is derived from `basis`
    and `activation` whenever it is read or used (the reference stores it and recomputes it after every update).  The
    recorded loss is sum |sum_k T V exp(i Phi) - X|^2; the reference's own list multiplies by the angle Phi itself
    (nmf.py:620), see DESIGN.md section 11."""

    def __init__(self, n_basis=2, regularizer=0.1, p=1, eps=EPS, *, dtype='float64', device=None, recordable_loss=True):
        """
        Args:
            n_basis: number of basis
        """
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device, recordable_loss=recordable_loss)

        self.regularizer, self.p = regularizer, p

    def _reset(self, **kwargs):
        super()._reset(**kwargs)

        self.init_phase()
        self.update_beta()

    @property
    def Beta(self):
        return self._unbatch(to_numpy(self._engine.cnmf_beta(self._dev("T", False), self._dev("V", False), eps=self.eps),
                                      np.float64))

    def update_beta(self):
        """nmf.py:669-676.  Nothing to do: Beta is a function of basis and activation, formed where it is used."""

    _OWN_STEPS = ("update", "update_once", "update_beta", "_record_loss")

    def _record_loss(self):
        T, V, Phi = self._model()
        loss = self._engine.cnmf_loss(self._X, T, V, Phi, self._ws, eps=self.eps)
        append_loss(self.loss, loss, self._batched)

    def update(self, iteration=100):
        if iteration > 0 and self._fast_loop_ok():  # the rule: DeviceState._fast_loop_ok; the loop is assx_cnmf_iterate
            self._iterate_block(iteration, ("T", "V", "Phi"), lambda loss: self._engine.cnmf_iterate(
                iteration, self._X, *self._model(), self._ws, regularizer=self.regularizer, p=self.p, eps=self.eps,
                loss=loss))
            return

        super().update(iteration=iteration)

    def update_once(self):
        T, V, Phi = self._model()
        self._engine.cnmf_update(self._X, T, V, Phi, self._ws, regularizer=self.regularizer, p=self.p, eps=self.eps)
        self._touch("T", "V", "Phi")

        self.update_beta()


class MultichannelNMFbase(DeviceState):
    """reference: nmf.py:116-148.  Keyword arguments of the call become attributes; `loss`, created once by the
    constructor, is never cleared between calls."""

    N_BASIS_MAX = 64

    def __init__(self, n_basis=2, eps=EPS, *, dtype='float64', device=None):
        """
        Args:
            n_basis: number of basis
        """
        self._require_float64(dtype, complex_ok=True)

        self.n_basis = n_basis
        self.loss = LazyLossList()

        self.eps = eps

        self.dtype = 'float64'
        self.device = device
        self._engine = None

    def __call__(self, target, iteration=100, **kwargs):
        self.target = target

        self._reset(**kwargs)

        self.update(iteration=iteration)

    def _reset(self, **kwargs):
        assert self.target is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

    def update(self, iteration=100):
        raise NotImplementedError("Implement `update` method.")

    def update_once(self):
        raise NotImplementedError("Implement `update_once` method.")


class MultichannelISNMF(MultichannelNMFbase):
    """reference: nmf.py:678-815 ("Multichannel Extensions of Non-Negative Matrix Factorization With Complex-Valued
    Data"), multichannel IS-NMF on a tensor of Hermitian covariance matrices: target[f,t] ~ sum_k basis[f,k]
    activation[k,t] spatial[f,k].  float64 / complex128, one target (n_bins, n_frames, n_channels, n_channels),
    2 <= n_channels <= 8, 1 <= n_basis <= 64.  `update_once()` and its parts run as HIP kernels (include/assx.h (f12):
    assx_covnmf_*); the loop of `update()` is one call of assx_covnmf_iterate.  There is no CPU fallback.

    Not to be confused with bss.mnmf.MultichannelISNMF (Sawada's MNMF with a latent assignment, on a mixture
    (n_channels, n_bins, n_frames)).  Deviations from the reference: `spatial` is always complex128 (the reference
    starts it as a real identity), and there is no `criterion` attribute (the loss is computed on the device; it needs a
    positive-definite target).  The target and `spatial` are read as Hermitian matrices.  A point whose model
    covariance is not positive definite where the method inverts it raises numpy.linalg.LinAlgError at the end of the
    call, not in the middle."""
    spatial = DeviceArray("H", complex_=True)
    basis = DeviceArray("T", complex_=False)
    activation = DeviceArray("V", complex_=False)

    N_CHANNELS_MIN, N_CHANNELS_MAX = 2, 8

    def __init__(self, n_basis=10, normalize=True, eps=EPS, *, dtype='float64', device=None):
        """
        Args:
            n_basis
            eps <float>: Machine epsilon
        """
        super().__init__(n_basis=n_basis, eps=eps, dtype=dtype, device=device)

        self.normalize = normalize

    def __call__(self, target, iteration=100, **kwargs):
        """
        Args:
            target <np.ndarray>: (n_bins, n_frames, n_channels, n_channels), complex Hermitian
            iteration <int>: Default: 100
        Returns:
            spatial (n_bins, n_basis, n_channels, n_channels), basis (n_bins, n_basis), activation (n_basis, n_frames)
        """
        self.target = target

        self._reset(**kwargs)

        self.update(target, iteration=iteration)

        H, T, V = self.spatial, self.basis, self.activation

        return H.copy(), T.copy(), V.copy()

    def _reset(self, **kwargs):
        """Everything of nmf.py:705-728: the refusals first, then the device and the draws."""
        super()._reset(**kwargs)

        target = self.target
        name = type(self).__name__
        n_basis = self._require_n_basis()
        is_tensor = isinstance(target, torch.Tensor)
        if not (target.is_complex() if is_tensor else np.iscomplexobj(target)):
            raise ValueError("{} supports complex targets only".format(name))
        shape = self._shape_of(target)
        if len(shape) != 4:
            raise ValueError("target must be (n_bins, n_frames, n_channels, n_channels), got {} dims".format(len(shape)))
        n_bins, n_frames, n_channels, _n_channels = shape
        if _n_channels != n_channels:
            raise ValueError("target must be square in its last two axes, got shape {}".format(shape))
        if not self.N_CHANNELS_MIN <= n_channels <= self.N_CHANNELS_MAX:
            raise ValueError("n_channels must be in [{}, {}], got {}".format(self.N_CHANNELS_MIN, self.N_CHANNELS_MAX,
                                                                             n_channels))
        if n_bins < 1 or n_frames < 1:
            raise ValueError("target must not be empty, got shape {}".format(shape))
        self._check_warm_start_array("spatial", (n_bins, n_basis, n_channels, n_channels), real=False)
        self._check_warm_start_array("basis", (n_bins, n_basis))
        self._check_warm_start_array("activation", (n_basis, n_frames))

        self.n_bins, self.n_frames = n_bins, n_frames
        self.n_channels = n_channels

        eng = self._ensure_engine()
        self._batched = False
        self._X = to_device(target, torch.complex128, eng.dev).contiguous()
        self._ws = eng.covnmf_workspace(n_channels, n_bins, n_frames, n_basis)
        self._status = eng.new_status(1)

        # identity spatial matrices, then basis before activation from the global RNG (nmf.py:714-726)
        self._keep_or_draw('spatial', lambda: np.tile(np.eye(n_channels, dtype=np.complex128),
                                                      reps=(n_bins, n_basis, 1, 1)), np.complex128)
        self._keep_or_draw('basis', lambda: np.random.rand(n_bins, n_basis), np.float64)
        self._keep_or_draw('activation', lambda: np.random.rand(n_basis, n_frames), np.float64)

    def _model(self):
        """(T (F,K), V (K,T), H (F,K,M,M)) on the device: the tensors of the attributes without their leading axis."""
        return self._dev("T", False)[0], self._dev("V", False)[0], self._dev("H", True)[0]

    _OWN_STEPS = ("update", "update_once", "update_basis", "update_activation", "update_spatial", "reconstruct",
                  "_record_loss")

    def _record_loss(self):
        T, V, H = self._model()
        loss = self._engine.covnmf_loss(self._X, T, V, H, self._ws, eps=self.eps, status=self._status)
        append_loss(self.loss, loss, False)

    def update(self, target=None, iteration=100):
        """nmf.py:730-736; `target` is accepted as there and, as there, the model's own target is what is used."""
        if self._fast_loop_ok():  # the rule: DeviceState._fast_loop_ok; the loop is assx_covnmf_iterate
            if iteration > 0:
                self._iterate_block(iteration, ("T", "V", "H"), lambda loss: self._engine.covnmf_iterate(
                    iteration, self._X, *self._model(), self._ws, normalize=self.normalize, eps=self.eps, loss=loss,
                    status=self._status), B=1)
        else:
            for idx in range(iteration):
                self.update_once()

                self._record_loss()
        self._check_status()

    def update_once(self):
        self.update_basis()
        self.update_activation()
        self.update_spatial()

    def update_basis(self):
        T, V, H = self._model()
        self._engine.covnmf_update_basis(self._X, T, V, H, self._ws, eps=self.eps, status=self._status)
        self._touch("T")

    def update_activation(self):
        T, V, H = self._model()
        self._engine.covnmf_update_activation(self._X, T, V, H, self._ws, eps=self.eps, status=self._status)
        self._touch("V")

    def update_spatial(self):
        T, V, H = self._model()
        self._engine.covnmf_update_spatial(self._X, T, V, H, self._ws, normalize=self.normalize, eps=self.eps,
                                           status=self._status)
        self._touch("H")

    def reconstruct(self):
        """sum_k spatial * basis * activation, (n_bins, n_frames, n_channels, n_channels) complex."""
        return to_numpy(self._engine.covnmf_reconstruct(*self._model()), np.complex128)
