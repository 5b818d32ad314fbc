"""Blind source separation by the primal-dual splitting algorithm on MI355X -- drop-in for `bss.prox.PDSBSSbase` of the
reference (src/bss/prox.py:13-201; Yatabe & Kitamura, "Determined blind source separation via proximal
splitting algorithm").  `ProxLaplaceIVA` (bss/iva.py) is the model built on it.

The reference states the iteration with scipy.sparse, as one block-diagonal operator with a block per (bin, source).  Here it
is dense per-bin algebra in csrc/assx_pdsbss.hip: the dual `y` is an (n_bins, n_sources, n_frames)
array in HBM, the operator norm stays on the device, and an unmodified model without callbacks runs its whole loop as one
library call.  A subclass with a `prox_penalty` of its own -- the reference's extension point -- or with any other step
overridden keeps the Python loop, in which `update_once` is composed of the four stage entry points and calls
`self.prox_logdet` / `self.prox_penalty`.  float64, one utterance, 2 <= n_channels <= 8.  There is no CPU fallback.
"""
import numpy as np

from .._device import to_device, to_numpy, torch
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList
from .. import _lib

EPS = 1e-12


class PDSBSSbase(DeviceState):
    """reference: prox.py:13-201"""

    demix_filter = DeviceArray("W", complex_=True)
    y = DeviceArray("y", complex_=True)

    _PENALTY = None  # the library's code of the model's penalty; None: a model whose prox_penalty the library does not know
    _OWN_STEPS = ("separate", "prox_logdet", "prox_penalty", "compute_penalty", "compute_negative_logdet",
                  "compute_negative_loglikelihood", "update_once", "_record_loss")
    _STATUS_RAISES = _lib.STATUS_SINGULAR | _lib.STATUS_NOT_CONVERGED

    def __init__(self, regularizer=1, step_prox_logdet=1e+0, step_prox_penalty=1e+0, step=1e+0, callbacks=None,
                 recordable_loss=True, eps=EPS, *, dtype='float64', device=None):
        """
        Args:
            regularizer <float>: Coefficient of source model penalty
            step_prox_logdet <float>: step size parameter `mu1`
            step_prox_penalty <float>: step size parameter `mu2`
            step <float>: relaxation `alpha`
        """
        self._require_float64(dtype, complex_ok=True)
        self.regularizer = regularizer
        self.step_prox_logdet, self.step_prox_penalty = step_prox_logdet, step_prox_penalty
        self.step = step

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
        self._X = None

    # ---- refusals, upload, the operator norm -------------------------------------------------------------------------
    def _reference_id(self):
        return getattr(self, "reference_id", 0)

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
        if n_channels * n_bins * n_frames >= 1 << 28:
            raise ValueError("{}: the input must stay below 4 GiB in complex128".format(name))
        for attr, positive in (("regularizer", False), ("step_prox_logdet", True), ("step_prox_penalty", True),
                               ("step", False)):
            v = getattr(self, attr)
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(v) or (positive and not v > 0):
                raise ValueError("{} must be a finite real number{}, got {!r}".format(attr, " > 0" if positive else "", v))
        ref = self._reference_id()
        if isinstance(ref, (bool, np.bool_)) or not isinstance(ref, (int, np.integer)) or not 0 <= ref < n_channels:
            raise ValueError("reference_id must be an int in [0, {}), got {!r}".format(n_channels, ref))
        self._check_warm_start_array('demix_filter', (n_bins, n_channels, n_channels), real=False)

        eng = self._ensure_engine()
        self._batched = False
        self._X = self._upload(self.input, torch.complex128)
        self._status = eng.new_status(1)
        n_sources = n_channels  # n_channels == n_sources (prox.py:52)

        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames

        if not hasattr(self, 'demix_filter'):
            W = torch.eye(n_sources, n_channels, dtype=torch.complex128, device=eng.dev)
            self._set_dev("W", W.repeat(1, n_bins, 1, 1).contiguous())
        self._estimation = None
        self._ws = eng.pdsbss_workspace(n_channels, n_bins, n_frames)
        # prox.py:67-79: the largest singular value of the block operator, on the device, and a dual that is zero again
        self._norm = eng.pdsbss_operator_norm(self._X[0], self._ws, status=self._status)
        self._set_dev("y", torch.zeros((1, n_bins, n_sources, n_frames), dtype=torch.complex128, device=eng.dev))

    @property
    def _Wd(self):
        return self._dev("W", True)

    @property
    def _yd(self):
        return self._dev("y", True)

    @property
    def norm(self):
        """The operator norm that X is divided by (prox.py:74).  Syncs to return a Python float."""
        if getattr(self, "_norm", None) is None:
            raise AttributeError("'{}' object has no attribute 'norm'".format(type(self).__name__))
        return float(self._norm.item())

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

    def _check_status(self):
        flags = int(self._status.max().item()) & self._STATUS_RAISES
        if flags:
            self._status.zero_()
            if flags & _lib.STATUS_NOT_CONVERGED:
                raise np.linalg.LinAlgError("SVD did not converge")
            raise np.linalg.LinAlgError(self._SINGULAR_TEXT)

    # ---- the loop ----------------------------------------------------------------------------------------------------
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

        return self._output(input, False)

    def _fast_loop_ok(self):
        """DeviceState's rule, and what assx_pdsbss_iterate knows: a penalty of the library's."""
        return super()._fast_loop_ok() and self._PENALTY is not None

    def _steps(self):
        return dict(C=float(self.regularizer), mu1=float(self.step_prox_logdet), mu2=float(self.step_prox_penalty),
                    alpha=float(self.step))

    def _run_fast_loop(self, iteration):
        eng = self._engine
        self._iterate_block(iteration + 1, ("W", "y"), lambda loss: eng.pdsbss_iterate(
            iteration, self._X[0], self._norm, self._Wd[0], self._yd[0], self._ws, loss=loss, status=self._status,
            penalty=self._PENALTY, **self._steps()))
        self._estimation = None

    def _loop(self, iteration):
        """The loop of the reference's __call__ (prox.py:92-103): a loss before the loop on every call, callbacks after
        each iteration and not before the loop."""
        if iteration > 0 and self._fast_loop_ok():
            # nothing observes the model between iterations: the whole loop is ONE call into the library
            # (assx_pdsbss_iterate gives the bits of assx_pdsbss_update and assx_pdsbss_loss called in turn)
            self._run_fast_loop(iteration)
            return

        if self.recordable_loss:
            self._record_loss()

        for idx in range(iteration):
            self.update_once()

            if self.recordable_loss:
                self._record_loss()

            if self.callbacks is not None:
                for callback in self.callbacks:
                    callback(self)

    def _as_dev(self, a, shape):
        """what a (possibly overridden) prox returned, as a contiguous complex128 device tensor of `shape`"""
        t = to_device(a, torch.complex128, self._engine.dev).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("{}: a prox returned shape {}, expected {}".format(type(self).__name__, tuple(t.shape), shape))
        return t

    def update_once(self):
        """prox.py:110-135, composed of the four stage entry points; the prox steps go through the methods."""
        eng = self._engine
        mu1, mu2, alpha = float(self.step_prox_logdet), float(self.step_prox_penalty), float(self.step)
        X, W, y = self._X[0], self._Wd[0], self._yd[0]

        G = eng.pdsbss_adjoint(X, self._norm, y, self._ws)
        W_tilde = self._as_dev(self.prox_logdet(W - mu1 * mu2 * G, mu1), W.shape)  # update demix_filter
        z = eng.pdsbss_forward(X, self._norm, y, (2 * W_tilde - W).contiguous())
        y_tilde = z - self._as_dev(self.prox_penalty(z, 1 / mu2), z.shape)
        y = alpha * y_tilde + (1 - alpha) * y
        W = alpha * W_tilde + (1 - alpha) * W

        self._set_dev("y", y.unsqueeze(0).contiguous())
        self._set_dev("W", W.unsqueeze(0).contiguous())
        self._estimation = None

    def separate(self, input, demix_filter):
        """y = W x on the device (prox.py:137-149): (n_channels, n_bins, n_frames), (n_bins, n_sources, n_channels)."""
        eng = self._ensure_engine()
        X = to_device(input, torch.complex128, eng.dev)
        W = to_device(demix_filter, torch.complex128, eng.dev)
        if X.dim() != 3 or tuple(W.shape) != (X.shape[1], X.shape[0], X.shape[0]):
            raise ValueError("separate: expected input (M,F,T) and demix_filter (F,M,M), got {} and {}".format(
                tuple(X.shape), tuple(W.shape)))
        Y = eng.demix(X.unsqueeze(0).contiguous(), W.unsqueeze(0).contiguous())[0]
        if isinstance(input, torch.Tensor):
            return Y
        return to_numpy(Y, np.complex128)

    def prox_logdet(self, demix_filter, mu=1):
        """prox.py:151-179 on a dense (n_bins, n_sources, n_channels) array or device tensor: per bin U h(S) V^H of the
        SVD, h(s) = (s + sqrt(s^2 + 4 mu)) / 2.  NumPy in, NumPy out; tensor in, tensor out."""
        eng = self._ensure_engine()
        W = to_device(demix_filter, torch.complex128, eng.dev).contiguous()
        status = getattr(self, "_status", None)
        if status is None:
            status = self._status = eng.new_status(1)
        out = eng.pdsbss_prox_logdet(W, float(mu), status=status)
        if isinstance(demix_filter, torch.Tensor):
            return out
        self._check_status()
        return to_numpy(out, np.complex128)

    def prox_penalty(self, z, mu=1):
        raise NotImplementedError("Implement `prox_penalty` method")

    def compute_penalty(self):
        """
        Returns:
            loss <float>
        """
        raise NotImplementedError("Implement `compute_penalty` method in subclass")

    def _own(self, *names):
        """whether the methods are still the model's own (the model: the first class that declares `_OWN_STEPS`)"""
        owner = next(c for c in type(self).__mro__ if "_OWN_STEPS" in vars(c))
        return all(getattr(type(self), n) is getattr(owner, n, None) for n in names)

    def _loss_terms(self):
        """(loss (1,), terms (2,)) of the filters as they stand, on the device"""
        eng = self._engine
        terms = eng.empty((2,), dtype=torch.float64)
        loss = eng.pdsbss_loss(self._X[0], self._Wd[0], self._ws, C=float(self.regularizer), terms=terms)
        return loss, terms

    def _record_loss(self):
        """Append the current loss; without a host sync while every term is the model's own and `loss` can hold it."""
        if isinstance(self.loss, LazyLossList) and self._PENALTY is not None \
                and self._own("compute_negative_loglikelihood", "compute_penalty", "compute_negative_logdet"):
            self.loss.append_device(self._loss_terms()[0], False)
        else:
            self.loss.append(self.compute_negative_loglikelihood())

    def compute_negative_loglikelihood(self):
        """prox.py:191-194.  Syncs to return a Python float."""
        if self._PENALTY is not None and self._own("compute_penalty", "compute_negative_logdet"):
            return np.float64(self._loss_terms()[0].item())
        loss = self.compute_penalty() + self.compute_negative_logdet()

        return loss

    def compute_negative_logdet(self):
        """prox.py:196-201: - sum_f ln|det W_f|."""
        return np.float64(self._loss_terms()[1][1].item())

    def _output(self, input, projection_back):
        eng = self._engine
        scale = None
        if projection_back:
            scale = eng.projection_back_scale(self._X, self._Wd, self._reference_id(), self._status)
        Y = eng.demix(self._X, self._Wd, scale=scale)
        self._check_status()

        output = self._unbatch(Y if isinstance(input, torch.Tensor) else to_numpy(Y, np.complex128))
        self.estimation = output

        return output
