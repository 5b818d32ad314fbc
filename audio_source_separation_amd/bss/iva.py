"""AuxIVA (Laplace / Gauss, iterative projection) on MI355X -- drop-in for `bss.iva.AuxLaplaceIVA`
and `bss.iva.AuxGaussIVA` of the reference (/root/reference/src/bss/iva.py:22-128, 289-802).

One iteration = two passes over X on the device:
  pass A  r_n(t) from y = W x (iva.py:489-491 / 722-724) -- the same pass yields the data term of the
          negative log-likelihood for the current filters (iva.py:604-619 / 783-802), so recording the
          loss costs no extra pass;
  pass B  weighted covariance (iva.py:493-499) + IP sweep (iva.py:500-518).
`algorithm_spatial='ISS'` (iva.py:525-542, 758-775) shares both passes: the rank-1 updates are applied to W through
quadratic forms of the same covariances (Y = W X is linear in W), so `demix_filter` stays available in the loop.
`algorithm_spatial in {'IP2', 'pairwise'}` (iva.py:544-599) is on the HIP path for AuxLaplaceIVA; AuxGaussIVA raises
NotImplementedError for it exactly like the reference (iva.py:777-778).  There is no CPU fallback.

`GradLaplaceIVA` and `NaturalGradLaplaceIVA` (iva.py:130-287) are the gradient baselines: two sweeps over X per iteration
too (r_n(t), then the N x M cross-moment of the score with x or y per bin) and a per-bin step, in csrc/assx_gradbss.hip
(DESIGN.md section 18); float64, one utterance, 2 <= n_channels <= 8.  `GradSteps` holds what they share with the FDICA
classes of bss/fdica.py.

`ProxLaplaceIVA` (iva.py:831-904) is IVA by primal-dual splitting on `PDSBSSbase` (bss/prox.py): a dual variable as large as
the separated signal, a per-bin SVD and a frame-wise group shrinkage across all bins, in csrc/assx_pdsbss.hip (DESIGN.md
section 19).
"""
import numpy as np

from .._device import to_device, to_numpy, torch
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList
from .. import _lib
from .prox import PDSBSSbase

EPS = 1e-12
THRESHOLD = 1e+12

__algorithms_spatial__ = ['IP', 'IVA', 'ISS', 'IPA', 'pairwise', 'IP1', 'IP2']


class IVAbase(DeviceState):
    """reference: iva.py:22-128"""

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
        self.recordable_loss = recordable_loss
        if self.recordable_loss:
            self.loss = LazyLossList()  # a list; entries are materialised from HBM on first read
        else:
            self.loss = None

        self.dtype = dtype
        self.device = device
        self._engine = None
        self._estimation = None

    def _reset(self, **kwargs):
        assert self.input is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        eng = self._ensure_engine()
        ndim = len(self._shape_of(self.input))
        if ndim not in (3, 4):
            raise ValueError("input must be (n_channels, n_bins, n_frames), got {} dims".format(ndim))
        self._batched = ndim == 4
        self._X = self._upload(self.input, eng.prec.cplx)
        B, n_channels, n_bins, n_frames = (int(s) for s in self._X.shape)
        self._status = eng.new_status(B)
        n_sources = n_channels  # n_channels == n_sources (iva.py:47)

        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames

        if not hasattr(self, 'demix_filter'):
            W = torch.eye(n_sources, n_channels, dtype=eng.prec.cplx, device=eng.dev)
            self._set_dev("W", W.repeat(B, n_bins, 1, 1).contiguous())
        self._estimation = None

    @property
    def _Wd(self):
        return self._dev("W", True)

    @property
    def estimation(self):
        if self._estimation is None:
            if getattr(self, "_X", None) is None:
                raise AttributeError("'{}' object has no attribute 'estimation'".format(type(self).__name__))
            self._estimation = self._unbatch(to_numpy(self._engine.demix(self._X, self._Wd), np.complex128))
        return self._estimation

    @estimation.setter
    def estimation(self, value):
        self._estimation = value

    def __repr__(self):
        s = "IVA("
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' function")

    def separate(self, input, demix_filter):
        """y = W x on the device (iva.py:105-117)."""
        eng = self._ensure_engine()
        X = to_device(input, eng.prec.cplx, eng.dev)
        W = to_device(demix_filter, eng.prec.cplx, eng.dev)
        batched = X.dim() == 4
        if not batched:
            X = X.unsqueeze(0)
        if W.dim() == 2:
            W = W.expand(X.shape[2], -1, -1)
        if W.dim() == 3:
            W = W.unsqueeze(0).expand(X.shape[0], -1, -1, -1)
        Y = eng.demix(X.contiguous(), W.contiguous())
        if isinstance(input, torch.Tensor):
            return Y if batched else Y[0]
        Y = to_numpy(Y, np.complex128)
        return Y if batched else Y[0]

    def compute_demix_filter(self, estimation, input):
        """W = Y X^H (X X^H)^{-1} per bin (iva.py:119-125): the least-squares demixing filter that maps `input`
        onto `estimation`.  (n_sources, n_bins, n_frames) x (n_channels, n_bins, n_frames) -> (n_bins, n_sources,
        n_channels); NumPy in -> NumPy out, device tensors in -> device tensor out; a leading utterance axis is kept."""
        eng = self._ensure_engine()
        Y = to_device(estimation, eng.prec.cplx, eng.dev)
        X = to_device(input, eng.prec.cplx, eng.dev)
        if Y.shape != X.shape:
            raise ValueError("estimation {} and input {} must have the same shape (n_sources == n_channels)".format(tuple(Y.shape), tuple(X.shape)))
        batched = X.dim() == 4
        if not batched:
            X, Y = X.unsqueeze(0), Y.unsqueeze(0)
        status = eng.new_status(X.shape[0])
        W = eng.compute_demix_filter(Y.contiguous(), X.contiguous(), status=status)
        if int(status.max().item()) & _lib.STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        if isinstance(input, torch.Tensor) and isinstance(estimation, torch.Tensor):
            return W if batched else W[0]
        W = to_numpy(W, np.complex128)
        return W if batched else W[0]

    def compute_negative_loglikelihood(self):
        raise NotImplementedError("Implement 'compute_negative_loglikelihood' function.")


class GradSteps:
    """What the gradient models share -- GradIVAbase below and GradFDICAbase (bss/fdica.py): the refusals of `_reset`, one
    update, the loss, and the loop as one library call.  float64, one utterance, 2..8 channels."""

    _MODEL = None    # _lib.GRADBSS_IVA / _lib.GRADBSS_FDICA
    _NATURAL = None  # False: gradient form, True: natural-gradient form; None: a base class without kernels
    _MAX_BINS = None  # FDICA: what the permutation solver takes

    def _reset(self, **kwargs):
        assert self.input is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        # refusals, before a device is touched
        name = type(self).__name__
        self._require_float64(self.dtype, complex_ok=True)
        self.dtype = 'float64'
        shape = self._shape_of(self.input)
        if len(shape) != 3:
            raise ValueError("{} takes one utterance (n_channels, n_bins, n_frames), got {} dims".format(name, len(shape)))
        if not (self.input.is_complex() if isinstance(self.input, torch.Tensor) else np.iscomplexobj(self.input)):
            raise ValueError("{} takes a complex input".format(name))
        n_channels, n_bins, n_frames = shape
        if not 2 <= n_channels <= 8:
            raise ValueError("{} supports 2 <= n_channels <= 8, got n_channels={}".format(name, n_channels))
        if n_bins < 1 or n_frames < 1:
            raise ValueError("{}: empty input {}".format(name, shape))
        if self._MAX_BINS is not None and n_bins > self._MAX_BINS:
            raise ValueError("{} supports n_bins <= {}, got n_bins={}".format(name, self._MAX_BINS, n_bins))
        if n_channels * n_bins * n_frames >= 1 << 28:
            raise ValueError("{}: the input must stay below 4 GiB in complex128".format(name))
        lr = self.lr
        if isinstance(lr, (bool, np.bool_)) or not isinstance(lr, (int, float, np.integer, np.floating)) \
                or not np.isfinite(lr):
            raise ValueError("lr must be a finite real number, got {!r}".format(lr))
        ref = self.reference_id
        if isinstance(ref, (bool, np.bool_)) or not isinstance(ref, (int, np.integer)) or not 0 <= ref < n_channels:
            raise ValueError("reference_id must be an int in [0, {}), got {!r}".format(n_channels, ref))
        self._check_warm_start_array('demix_filter', (n_bins, n_channels, n_channels), real=False)

        eng = self._ensure_engine()
        self._batched = False
        self._X = self._upload(self.input, torch.complex128)
        self._status = eng.new_status(1)
        n_sources = n_channels  # n_channels == n_sources (iva.py:47, fdica.py:35)

        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames

        if not hasattr(self, 'demix_filter'):
            W = torch.eye(n_sources, n_channels, dtype=torch.complex128, device=eng.dev)
            self._set_dev("W", W.repeat(1, n_bins, 1, 1).contiguous())
        self._estimation = None
        self._ws = eng.gradbss_workspace(n_channels, n_bins, n_frames)

    def _fast_loop_ok(self):
        """DeviceState's rule, and what assx_gradbss_iterate knows: a model with kernels, the holonomic natural form."""
        return super()._fast_loop_ok() and self._NATURAL is not None and getattr(self, "is_holonomic", True)

    def _run_fast_loop(self, iteration):
        eng = self._engine
        self._iterate_block(iteration + 1, ("W",), lambda loss: eng.gradbss_iterate(
            iteration, self._MODEL, self._NATURAL, self._X[0], self._Wd[0], self._ws, lr=self.lr, eps=self.eps, loss=loss,
            status=self._status))
        self._estimation = None

    def _loop(self, iteration):
        """The loop of the reference's __call__ (iva.py:153-170, fdica.py:162-179)."""
        if iteration > 0 and self._fast_loop_ok():
            # nothing observes the model between iterations: the whole loop is ONE call into the library
            # (assx_gradbss_iterate enqueues the kernels of the loop below in the same order: bit-identical)
            self._run_fast_loop(iteration)
            return

        if self.recordable_loss:
            self._record_loss()

        if self.callbacks is not None:
            for callback in self.callbacks:
                callback(self)

        for idx in range(iteration):
            self.update_once()

            if self.recordable_loss:
                self._record_loss()

            if self.callbacks is not None:
                for callback in self.callbacks:
                    callback(self)

    def _grad_update(self):
        self._engine.gradbss_update(self._MODEL, self._NATURAL, self._X[0], self._Wd[0], self._ws, lr=self.lr,
                                    eps=self.eps, status=self._status)
        self._touch("W")
        self._estimation = None

    def _loss_device(self):
        return self._engine.gradbss_loss(self._MODEL, self._X[0], self._Wd[0], self._ws)

    def _record_loss(self):
        """Append the current loss without a host sync (the value stays in HBM until `loss` is read)."""
        if isinstance(self.loss, LazyLossList) and self._own("compute_negative_loglikelihood"):
            self.loss.append_device(self._loss_device(), False)
        else:
            self.loss.append(self.compute_negative_loglikelihood())

    def _own(self, name):
        """whether method `name` is still the model's own (the model: the first class that declares `_OWN_STEPS`)"""
        owner = next(c for c in type(self).__mro__ if "_OWN_STEPS" in vars(c))
        return getattr(type(self), name) is getattr(owner, name, None)

    def _grad_loss(self):
        loss = self._loss_device()
        return np.float64(loss.item())

    def _output(self, input, projection_back):
        eng = self._engine
        scale = None
        if projection_back:
            scale = eng.projection_back_scale(self._X, self._Wd, self.reference_id, self._status)
        Y = eng.demix(self._X, self._Wd, scale=scale)
        self._check_status()

        output = self._unbatch(Y if isinstance(input, torch.Tensor) else to_numpy(Y, np.complex128))
        self.estimation = output

        return output


class GradIVAbase(GradSteps, IVAbase):
    """reference: iva.py:130-194"""

    _MODEL = _lib.GRADBSS_IVA

    def __init__(self, lr=1e-1, reference_id=0, callbacks=None, apply_projection_back=True, recordable_loss=True, eps=EPS,
                 *, dtype='float64', device=None):
        super().__init__(callbacks=callbacks, recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)
        self._require_float64(dtype, complex_ok=True)

        self.lr = lr
        self.reference_id = reference_id
        self.apply_projection_back = apply_projection_back

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

        return self._output(input, self.apply_projection_back)

    def __repr__(self):
        s = "GradIVA("
        s += "lr={lr}"
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' function")

    def compute_negative_loglikelihood(self):
        raise NotImplementedError("Implement 'compute_negative_loglikelihood' function.")


class GradLaplaceIVA(GradIVAbase):
    """reference: iva.py:196-241"""
    _NATURAL = False
    _OWN_STEPS = ("update_once", "compute_negative_loglikelihood", "_record_loss")

    def __repr__(self):
        s = "NaturalGradIVA("
        s += "lr={lr}"
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        """iva.py:207-233: W <- W - lr ((1/T) sum_t phi x^H - W^-H)."""
        self._grad_update()

    def compute_negative_loglikelihood(self):
        """iva.py:235-241.  Syncs to return a Python float."""
        return self._grad_loss()


class NaturalGradLaplaceIVA(GradIVAbase):
    """reference: iva.py:243-287"""
    _NATURAL = True
    _OWN_STEPS = ("update_once", "compute_negative_loglikelihood", "_record_loss")

    def __repr__(self):
        s = "NaturalGradLaplaceIVA("
        s += "lr={lr}"
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        """iva.py:254-279: W <- W - lr ((1/T) sum_t phi y^H - I) W."""
        self._grad_update()

    def compute_negative_loglikelihood(self):
        """iva.py:281-287.  Syncs to return a Python float."""
        return self._grad_loss()


class AuxIVAbase(IVAbase):
    """reference: iva.py:289-386"""

    _KIND = None
    _NAME = "AuxIVA"

    def __init__(self, algorithm_spatial='IP', reference_id=0, callbacks=None, apply_projection_back=True,
                 recordable_loss=True, eps=EPS, threshold=THRESHOLD, *, dtype='float64', device=None):
        super().__init__(callbacks=callbacks, recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)

        self.algorithm_spatial = algorithm_spatial
        self.reference_id = reference_id
        self.apply_projection_back = apply_projection_back
        self.threshold = threshold

        if not self.algorithm_spatial in __algorithms_spatial__:
            raise ValueError("Not support {} based spatial updates.".format(self.algorithm_spatial))

        if self.algorithm_spatial in ['pairwise', 'IP2']:
            self.update_pair = None

    def _require_supported(self):
        if self._KIND is None:
            raise NotImplementedError("Implement 'update_once' function.")
        if self.algorithm_spatial in ('pairwise', 'IP2') and self._KIND == _lib.IVA_GAUSS:
            raise NotImplementedError("In progress...")  # iva.py:777-778
        if self.algorithm_spatial not in ('IP', 'IP1', 'ISS', 'pairwise', 'IP2'):
            raise NotImplementedError("algorithm_spatial='{}' is not on the HIP path (no CPU fallback is provided).".format(self.algorithm_spatial))

    def _reset(self, **kwargs):
        super()._reset(**kwargs)
        self._require_supported()
        self._r = None       # r_n(t) of the CURRENT filters; None = stale
        self._r_src = None
        self._loss_dev = None

    def _refresh_weights(self, with_loss):
        """Pass A: r (and the loss of the current filters when asked) in one sweep over X."""
        self._r, self._loss_dev = self._engine.auxiva_weights(self._X, self._Wd, self._KIND, eps=self.eps,
                                                             with_loss=with_loss)
        self._r_src = self._Wd  # the filters these weights belong to (a host-side assignment replaces the tensor)

    def __call__(self, input, iteration=100, **kwargs):
        """
        Args:
            input (n_channels, n_bins, n_frames)
        Returns:
            output (n_channels, n_bins, n_frames)
        """
        self.input = input

        self._reset(**kwargs)

        if iteration > 0 and self._fast_loop_ok():
            # nothing observes the model between iterations: the whole loop is ONE call into the library
            # (assx_auxiva_iterate enqueues the same entry points in the same order: bit-identical to the loop below)
            self._run_fast_loop(iteration)
        else:
            if self.recordable_loss:
                self._record_loss()

            if self.callbacks is not None:
                for callback in self.callbacks:
                    callback(self)

            for idx in range(iteration):
                if self.algorithm_spatial in ['pairwise', 'IP2']:
                    self._select_update_pair()

                self.update_once()

                if self.recordable_loss:
                    self._record_loss()

                if self.callbacks is not None:
                    for callback in self.callbacks:
                        callback(self)

        eng = self._engine
        scale = None
        if self.apply_projection_back:
            scale = eng.projection_back_scale(self._X, self._Wd, self.reference_id, self._status)
        Y = eng.demix(self._X, self._Wd, scale=scale)
        self._check_status()

        output = self._unbatch(Y if isinstance(input, torch.Tensor) else to_numpy(Y, np.complex128))
        self.estimation = output

        return output

    # ---- the loop of __call__ as one library call (iva.py:420-441) ---------------------------------------------
    _OWN_STEPS = ("update_once", "update_once_ip", "update_once_iss", "update_once_pairwise", "_spatial_update",
                  "_record_loss", "_refresh_weights", "_select_update_pair")

    def _fast_loop_ok(self):
        """DeviceState's rule, and what assx_auxiva_iterate knows: a model with kernels, a spatial update on the HIP path."""
        return super()._fast_loop_ok() and self._KIND is not None \
            and self.algorithm_spatial in ('IP', 'IP1', 'ISS', 'pairwise', 'IP2')

    def _run_fast_loop(self, iteration):
        eng = self._engine
        B, N, T = int(self._X.shape[0]), self.n_sources, self.n_frames
        spatial, pair = _lib.SPATIAL_IP, (0, 1)
        if self.algorithm_spatial == 'ISS':
            spatial = _lib.SPATIAL_ISS
        elif self.algorithm_spatial in ['pairwise', 'IP2']:
            self._require_supported()
            self._select_update_pair()  # the pair of the first iteration; the library advances it like iva.py:370-382
            spatial, pair = _lib.SPATIAL_IP2, self.update_pair
        r = eng.empty((B, N, T))
        loss = self._iterate_block(iteration + 1, ("W",), lambda loss: eng.auxiva_iterate(
            iteration, self._KIND, self._X, self._Wd, r, eps=self.eps, threshold=self.threshold, status=self._status,
            loss=loss, spatial=spatial, pair=pair))
        if spatial == _lib.SPATIAL_IP2:
            self.update_pair = ((pair[0] + iteration - 1) % N, (pair[1] + iteration - 1) % N)
        self._estimation = None
        if loss is not None:  # r and the last loss entry belong to the final filters
            self._r, self._r_src, self._loss_dev = r, self._Wd, loss[iteration]
        else:
            self._r = self._loss_dev = None

    def __repr__(self):
        s = self._NAME + "("
        s += "algorithm_spatial={algorithm_spatial}"
        s += ")"

        return s.format(**self.__dict__)

    def update_once(self):
        if self.algorithm_spatial in ['IP', 'IP1']:
            self.update_once_ip()
        elif self.algorithm_spatial == 'ISS':
            self.update_once_iss()
        elif self.algorithm_spatial in ['pairwise', 'IP2']:
            self.update_once_pairwise()
        else:
            self._require_supported()

    def update_once_ip(self):
        """iva.py:481-523 / 714-757: weights from the current estimate, covariance, IP sweep."""
        self._spatial_update(_lib.SPATIAL_IP)

    def update_once_iss(self):
        """iva.py:525-542 / 758-775: weights from the current estimate, covariance, ISS sweep."""
        self._spatial_update(_lib.SPATIAL_ISS)

    def update_once_pairwise(self):
        """iva.py:544-599: pairwise update of rows `update_pair`."""
        self._require_supported()
        self._spatial_update(_lib.SPATIAL_IP2, pair=self.update_pair)

    def _select_update_pair(self):
        """(0,1), (1,2), ..., (N-1,0)   (iva.py:370-382)."""
        n_sources = self.n_sources

        if self.update_pair is None:
            m, n = 0, 1
        else:
            m, n = self.update_pair
            m, n = m + 1, n + 1
            m, n = m % n_sources, n % n_sources

        self.update_pair = m, n

    def _spatial_update(self, spatial, pair=(0, 1)):
        if self._r is None or self._r_src is not self._Wd:
            self._refresh_weights(with_loss=False)
        self._engine.auxiva_spatial_update(self._X, self._Wd, self._r, eps=self.eps, threshold=self.threshold,
                                           status=self._status, spatial=spatial, pair=pair)
        self._touch("W")
        self._estimation = None
        self._r = None
        self._loss_dev = None

    def _record_loss(self):
        """Append the current loss without a host sync (the value stays in HBM until `loss` is read)."""
        if self._r is None or self._loss_dev is None or self._r_src is not self._Wd:
            self._refresh_weights(with_loss=True)
        if isinstance(self.loss, LazyLossList):
            self.loss.append_device(self._loss_dev, self._batched)
        else:
            self.loss.append(to_numpy(self._loss_dev, np.float64) if self._batched else np.float64(self._loss_dev.item()))

    def compute_negative_loglikelihood(self):
        """iva.py:604-619 / 783-802.  Rides on the r_n(t) pass; syncs to return a Python float."""
        if self._r is None or self._loss_dev is None or self._r_src is not self._Wd:
            self._refresh_weights(with_loss=True)
        self._check_status()
        if self._batched:
            return to_numpy(self._loss_dev, np.float64)
        return np.float64(self._loss_dev.item())


class AuxLaplaceIVA(AuxIVAbase):
    """reference: iva.py:388-619"""
    _KIND = _lib.IVA_LAPLACE
    _NAME = "AuxLaplaceIVA"


class AuxGaussIVA(AuxIVAbase):
    """reference: iva.py:621-802"""
    _KIND = _lib.IVA_GAUSS
    _NAME = "AuxGaussIVA"


class ProxLaplaceIVA(PDSBSSbase):
    """reference: iva.py:831-904"""

    _PENALTY = _lib.PDSBSS_LAPLACE
    _OWN_STEPS = PDSBSSbase._OWN_STEPS

    def __init__(self, regularizer=1, step_prox_logdet=1e+0, step_prox_penalty=1e+0, step=1e+0, reference_id=0,
                 callbacks=None, apply_projection_back=True, recordable_loss=True, eps=EPS, *, dtype='float64', device=None):
        super().__init__(regularizer=regularizer, step_prox_logdet=step_prox_logdet, step_prox_penalty=step_prox_penalty,
                         step=step, callbacks=callbacks, recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)

        self.reference_id = reference_id
        self.apply_projection_back = apply_projection_back

    def __call__(self, input, iteration, **kwargs):
        """
        Args:
            input (n_channels, n_bins, n_frames)
            iteration <int>
        Returns:
            output (n_channels, n_bins, n_frames)
        """
        self.input = input

        self._reset(**kwargs)
        self._loop(iteration)

        return self._output(input, self.apply_projection_back)

    def __repr__(self):
        s = "ProxLaplaceIVA("
        s += "regularizer={regularizer}, step_prox_logdet={step_prox_logdet}, step_prox_penalty={step_prox_penalty}"
        s += ", step={step}"
        s += ")"

        return s.format(**self.__dict__)

    def prox_penalty(self, z, mu=1):
        """iva.py:867-889 on a dense (n_bins, n_sources, n_frames) array or device tensor: C max(0, 1 - mu / den) z with
        den[n,t] = sqrt(sum_f |z|^2), mu where it is <= 0.  NumPy in, NumPy out; tensor in, tensor out."""
        eng = self._ensure_engine()
        zd = to_device(z, torch.complex128, eng.dev).contiguous()
        if zd.dim() != 3:
            raise ValueError("prox_penalty: expected z (n_bins, n_sources, n_frames), got {}".format(tuple(zd.shape)))
        F, N, T = (int(d) for d in zd.shape)
        ws = self._ws if (F, N, T) == (getattr(self, "n_bins", None), getattr(self, "n_sources", None),
                                       getattr(self, "n_frames", None)) else eng.pdsbss_workspace(N, F, T)
        out = eng.pdsbss_prox_group(zd, ws, C=float(self.regularizer), mu=float(mu), penalty=self._PENALTY)
        if isinstance(z, torch.Tensor):
            return out
        return to_numpy(out, np.complex128)

    def compute_penalty(self):
        """iva.py:891-904: C sum_{n,t} sqrt(sum_f |y[n,f,t]|^2).  Syncs to return a Python float."""
        return np.float64(self._loss_terms()[1][0].item())
