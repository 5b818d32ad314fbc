"""Independent deeply learned matrix analysis on MI355X -- drop-in for `sss.idlma` of the reference
(src/sss/idlma.py:10-246; Makishima et al., "Independent deeply learned matrix analysis for determined
audio source separation").

The source model is the caller's torch module and runs as it is, under `torch.no_grad()`, on the device tensor and on
torch's current stream.  Everything around it is csrc/assx_idlma.hip: the network's float32 input
straight from X and W, the float32 arithmetic NumPy applies to the network's output, the spatial update, the projection
back and the loss.  An unmodified model without a callback issues ONE library call per iteration (assx_idlma_step) next to
the network's forward pass; nothing is copied to the host and nothing synchronises inside the loop.  With a callback or an
overridden step the loop runs the public methods, which give the same bits.  float64 state, one utterance,
2 <= n_channels <= 8, n_frames >= n_channels.  There is no CPU fallback: the network's parameters must live on the model's GPU.

`update_space_model` (the free function) is the spatial update alone for a caller-supplied source model.
"""
import numpy as np

from .._device import to_device, to_numpy, torch
from .._state import DeviceArray, DeviceState
from .._loss import LazyLossList, append_loss
from .. import _lib
from ..algorithm.projection_back import _engine

EPS = 1e-12
THRESHOLD = 1e+12


def update_space_model(input, demix_filter, dnn_output, domain=2, eps=EPS, threshold=THRESHOLD, *, dtype='float64',
                       device=None):
    """
    Args:
        input (n_channels, n_bins, n_frames) complex: mixture STFT
        demix_filter (n_bins, n_sources, n_channels) complex: current W (not modified)
        dnn_output (n_sources, n_bins, n_frames) real >= 0: the source model's output; R = dnn_output**(2/domain)
    Returns:
        demix_filter (n_bins, n_sources, n_channels) after one IP sweep (idlma.py:196-208).
        NumPy in -> NumPy out; device tensors in -> device tensor out; a leading utterance axis is allowed on all three.
    """
    eng = _engine(dtype, device)
    X = to_device(input, eng.prec.cplx, eng.dev)
    W = to_device(demix_filter, eng.prec.cplx, eng.dev)
    R = to_device(dnn_output, eng.prec.real, eng.dev)
    batched = X.dim() == 4
    if not batched:
        X, W, R = X.unsqueeze(0), W.unsqueeze(0), R.unsqueeze(0)
    if tuple(R.shape) != tuple(X.shape) or tuple(W.shape) != (X.shape[0], X.shape[2], X.shape[1], X.shape[1]):
        raise ValueError("shapes do not match: input {}, demix_filter {}, dnn_output {}".format(
            tuple(X.shape), tuple(W.shape), tuple(R.shape)))
    W = W.contiguous().clone()
    status = eng.new_status(X.shape[0])
    eng.idlma_space_update(X.contiguous(), W, R.contiguous(), domain=domain, eps=eps, threshold=threshold, status=status)
    if int(status.max().item()) & _lib.STATUS_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")
    if isinstance(input, torch.Tensor) and isinstance(demix_filter, torch.Tensor):
        return W if batched else W[0]
    W = to_numpy(W, np.complex128)
    return W if batched else W[0]


class IDLMAbase(DeviceState):
    """reference: idlma.py:10-87"""

    demix_filter = DeviceArray("W", complex_=True)

    def __init__(self, normalize=True, callback=None, dnn_flooring=1e-5, eps=EPS, *, dtype='float64', device=None):
        self._require_float64(dtype)
        self.callback = callback
        self.eps = eps
        self.input = None
        self.loss = LazyLossList()  # a list; entries are materialised from HBM on first read

        self.normalize = normalize
        self.dnn_flooring = dnn_flooring

        self.dtype = dtype
        self.device = device
        self._engine = None
        self._estimation = None
        self._X = None
        self._dnn_out = None

    # ---- refusals, before a device or the RNG is touched ------------------------------------------------------------
    def _check_normalize(self):
        pass

    def _check_dnn(self):
        dnn = self.dnn
        if dnn is None:
            raise ValueError("{} needs the source model: pass dnn=<torch.nn.Module> to the call".format(type(self).__name__))
        if not callable(dnn) or not hasattr(dnn, "parameters"):
            raise ValueError("dnn must be a torch.nn.Module, got {!r}".format(type(dnn).__name__))
        p = next(iter(dnn.parameters()), None)
        if p is None:
            raise ValueError("dnn has no parameters: its device cannot be told (the reference reads next(dnn.parameters()))")
        want = None if self.device is None else torch.device(self.device)
        if p.device.type != 'cuda' or (want is not None and want.index is not None and p.device.index != want.index):
            raise ValueError("the parameters of dnn are on {}, the model runs on {}: move the network to the GPU (there is "
                             "no CPU fallback)".format(p.device, "the current GPU" if want is None else want))
        return p.device

    def _reset(self, dnn=None, **kwargs):
        assert self.input is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])
        self.dnn = dnn

        name = type(self).__name__
        self._require_float64(self.dtype)
        self.dtype = 'float64'
        shape = self._shape_of(self.input)
        if len(shape) != 3:
            raise ValueError("{} takes one utterance (n_channels, n_bins, n_frames), got {} dims".format(name, len(shape)))
        if not (self.input.is_complex() if isinstance(self.input, torch.Tensor) else np.iscomplexobj(self.input)):
            raise ValueError("{} takes a complex input".format(name))
        n_channels, n_bins, n_frames = shape
        if not 2 <= n_channels <= 8:
            raise ValueError("{} supports 2 <= n_channels <= 8, got n_channels={}".format(name, n_channels))
        if n_bins < 1:
            raise ValueError("{}: empty input {}".format(name, shape))
        if n_frames < n_channels:
            raise ValueError("{} needs n_frames >= n_channels (X X^H of a bin is singular below), got n_frames={} for "
                             "n_channels={}".format(name, n_frames, n_channels))
        if n_channels * n_bins * n_frames >= 1 << 28:
            raise ValueError("{}: the input must stay below 4 GiB in complex128".format(name))
        self._check_normalize()
        self._check_parameters(n_channels)
        self._check_warm_start_array('demix_filter', (n_bins, n_channels, n_channels), real=False)
        param_dev = self._check_dnn()

        eng = self._ensure_engine()
        if param_dev != eng.dev:
            raise ValueError("the parameters of dnn are on {}, the model runs on {}".format(param_dev, eng.dev))
        self._batched = False
        self._X = self._upload(self.input, torch.complex128)
        self._status = eng.new_status(1)
        n_sources = n_channels  # n_channels == n_sources (idlma.py:29)

        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames

        if not hasattr(self, 'demix_filter'):
            W = torch.eye(n_sources, n_channels, dtype=torch.complex128, device=eng.dev)
            self._set_dev("W", W.repeat(1, n_bins, 1, 1).contiguous())
        self._estimation = None

        self._ws = eng.idlma_workspace(n_channels, n_bins, n_frames)
        self._R = eng.empty((n_sources, n_bins, n_frames), dtype=torch.float64)
        self._dnn_out = torch.ones((n_sources, n_bins, n_frames), dtype=torch.float32, device=eng.dev)  # idlma.py:39

    def _check_parameters(self, n_channels):
        pass

    @property
    def _Wd(self):
        return self._dev("W", True)

    @property
    def dnn_output(self):
        """(n_sources, n_bins, n_frames) float32, as the reference keeps it after the first source-model update."""
        if self._dnn_out is None:
            raise AttributeError("'{}' object has no attribute 'dnn_output'".format(type(self).__name__))
        return to_numpy(self._dnn_out, np.float32)

    @dnn_output.setter
    def dnn_output(self, value):
        eng = self._ensure_engine()
        t = to_device(value, torch.float32, eng.dev).contiguous()
        if self._dnn_out is not None and tuple(t.shape) != tuple(self._dnn_out.shape):
            raise ValueError("dnn_output has shape {}, the model needs {}".format(tuple(t.shape), tuple(self._dnn_out.shape)))
        self._dnn_out = t.clone() if t is value else t

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

        Y = self._engine.demix(self._X, self._Wd)
        self._check_status()
        output = self._unbatch(Y if isinstance(input, torch.Tensor) else to_numpy(Y, np.complex128))
        self.estimation = output

        return output

    def _fast_loop_ok(self):
        return False

    def _loop(self, iteration):
        """The loop of the reference's __call__ (idlma.py:52-62): a loss before the loop on every call, the callback
        after each iteration and not before the loop."""
        if self._fast_loop_ok():
            self._run_fast_loop(iteration)
            return

        self._record_loss()

        for idx in range(iteration):
            self.update_once()

            self._record_loss()

            if self.callback is not None:
                self.callback(self)

    def _record_loss(self):
        self.loss.append(self.compute_negative_loglikelihood())

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' function")

    def separate(self, input, demix_filter):
        """y = W x on the device (idlma.py:72-84): (n_channels, n_bins, n_frames), (n_bins, n_sources, n_channels)."""
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

    def compute_negative_loglikelihood(self):
        raise NotImplementedError("Implement 'compute_negative_loglikelihood' function.")


class GaussIDLMA(IDLMAbase):
    """reference: idlma.py:89-246"""

    _OWN_STEPS = ("update_once", "update_source_model", "update_space_model", "estimate_by_dnn", "floor_dnn_output",
                  "separate", "compute_negative_loglikelihood", "_record_loss")

    def __init__(self, domain=2, normalize='power', reference_id=0, callback=None, dnn_flooring=1e-5, eps=EPS,
                 threshold=THRESHOLD, *, dtype='float64', device=None):
        """
        Args:
            normalize <str>: 'projection-back': projection back based normalization.  The constructor's default 'power'
                is the reference's, which refuses it when the first update runs; here the call refuses it before.
            threshold <float>: threshold for condition number when computing (WU)^{-1}.
        """
        super().__init__(normalize=normalize, callback=callback, dnn_flooring=dnn_flooring, eps=eps, dtype=dtype,
                         device=device)

        if not 1 <= domain <= 2:
            raise ValueError("1 <= `domain` <= 2 is not satisfied.")

        self.domain = domain
        self.reference_id = reference_id
        self.threshold = threshold

    def _check_normalize(self):
        # idlma.py:149-159, raised there from inside the first update_once, after W has moved
        if not self.normalize:
            raise ValueError("Set normalize=True")
        if self.normalize != 'projection-back':
            raise ValueError("Not support normalization based on {}. Choose 'power' or 'projection-back'".format(
                self.normalize))

    def _check_parameters(self, n_channels):
        domain, ref = self.domain, self.reference_id
        if isinstance(domain, (bool, np.bool_)) or not isinstance(domain, (int, float, np.integer, np.floating)) \
                or not 1 <= domain <= 2:
            raise ValueError("1 <= `domain` <= 2 is not satisfied, got {!r}".format(domain))
        if isinstance(ref, (bool, np.bool_)) or not isinstance(ref, (int, np.integer)) or not 0 <= ref < n_channels:
            raise ValueError("reference_id must be an int in [0, {}), got {!r}".format(n_channels, ref))

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

        eng = self._engine
        scale = eng.projection_back_scale(self._X, self._Wd, int(self.reference_id), self._status)
        Y = eng.demix(self._X, self._Wd, scale=scale)  # idlma.py:130-135
        self._check_status()
        output = self._unbatch(Y if isinstance(input, torch.Tensor) else to_numpy(Y, np.complex128))
        self.estimation = output

        return output

    # ---- the loop rule: one assx_idlma_step per iteration, or the public steps -----------------
    def _fast_loop_ok(self):
        return self.callback is None and DeviceState._fast_loop_ok(self)

    def _step_args(self):
        return dict(domain=float(self.domain), dnn_flooring=float(self.dnn_flooring or 0.0), eps=float(self.eps),
                    threshold=float(self.threshold), ref=int(self.reference_id))

    def _run_fast_loop(self, iteration):
        eng = self._engine
        X, W = self._X[0], self._Wd[0]
        self.loss.append_device(self._device_loss(), False)
        if iteration < 1:
            return
        inp = eng.idlma_dnn_input(X, W, domain=float(self.domain))
        for idx in range(iteration):
            out = self._forward(inp)
            loss = eng.empty((1,), dtype=torch.float64)
            eng.idlma_step(X, W, out, self._dnn_out, self._ws, loss=loss, next_input=inp if idx + 1 < iteration else None,
                           status=self._status, **self._step_args())
            self.loss.append_device(loss, False)
        self._touch("W")
        self._estimation = None

    def _forward(self, inp):
        """The network on its float32 device input: no host copy, torch's current stream."""
        with torch.no_grad():
            out = self.dnn(inp)
        want = tuple(inp.shape)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != want or out.dtype != torch.float32 \
                or out.device != inp.device:
            raise ValueError("dnn must return a float32 tensor of shape {} on {}, got {}".format(
                want, inp.device, "{} {} on {}".format(out.dtype, tuple(out.shape), out.device)
                if isinstance(out, torch.Tensor) else type(out).__name__))
        return out.detach().contiguous()

    def update_once(self, is_source_model_update=True):
        """idlma.py:140-162 with the refit in its scaled form: W[f,n,:] *= scale[n,f]."""
        if is_source_model_update:
            self.update_source_model()
        self.update_space_model()

        eng = self._engine
        scale = eng.projection_back_scale(self._X, self._Wd, int(self.reference_id), self._status)
        eng.idlma_normalize_pb(self._Wd[0], scale[0])
        self._touch("W")
        self._estimation = None

    def update_source_model(self):
        """idlma.py:164-173"""
        eng = self._engine
        own = type(self).estimate_by_dnn is GaussIDLMA.estimate_by_dnn
        if own:
            inp = eng.idlma_dnn_input(self._X[0], self._Wd[0], domain=float(self.domain))
            out = self._forward(inp)
            eng.idlma_variance(out, self._dnn_out, self._R, domain=float(self.domain), dnn_flooring=0.0, eps=float(self.eps))
        else:
            P = eng.ilrma_power_map(self._X, self._Wd)[0]
            self.dnn_output = self.estimate_by_dnn(P)

        if self.dnn_flooring:
            self.floor_dnn_output()

    def update_space_model(self):
        """idlma.py:175-210: R = dnn_output**(2/domain) in float32 floored at float32(eps), then the IP sweep."""
        eng = self._engine
        eps = float(self.eps)
        eng.idlma_variance(None, self._dnn_out, self._R, domain=float(self.domain), eps=eps)
        eng.idlma_space_update(self._X, self._Wd, self._R.unsqueeze(0), domain=2, eps=float(np.float32(eps)),
                               threshold=float(self.threshold), status=self._status)
        self._touch("W")
        self._estimation = None

    def estimate_by_dnn(self, input):
        """idlma.py:212-225 for a power map (n_sources, n_bins, n_frames): the network on float32(input**(domain/2)), its
        output **(2/domain) in float32.  NumPy in, NumPy out; tensor in, tensor out.  The model's own loop does not come
        through here unless a subclass overrides it: it forms the network's input from X and W in one pass."""
        eng = self._ensure_engine()
        domain = self.domain
        x = to_device(input, torch.float64, eng.dev)
        x = (x if domain == 2 else torch.sqrt(x) if domain == 1 else x ** (domain / 2)).to(torch.float32)
        out = self._forward(x.contiguous())
        out = out if domain == 2 else out * out if domain == 1 else out ** np.float32(2 / domain)
        if isinstance(input, torch.Tensor):
            return out
        return to_numpy(out, np.float32)

    def floor_dnn_output(self):
        """idlma.py:227-231: dnn_output = maximum(dnn_output, float32(dnn_flooring))."""
        eng = self._engine
        # exponent 1 (domain 2) is the identity: the call floors dnn_output in place; R is rewritten before its next use
        eng.idlma_variance(self._dnn_out, self._dnn_out, self._R, domain=2, dnn_flooring=float(self.dnn_flooring),
                           eps=float(self.eps))

    def _record_loss(self):
        if type(self).compute_negative_loglikelihood is GaussIDLMA.compute_negative_loglikelihood:
            append_loss(self.loss, self._device_loss(), False)  # no host sync
        else:
            self.loss.append(self.compute_negative_loglikelihood())

    def _device_loss(self):
        eng = self._engine
        eng.idlma_variance(None, self._dnn_out, self._R, domain=float(self.domain), eps=float(self.eps))
        return eng.idlma_loss(self._X[0], self._Wd[0], self._R, self._ws)

    def compute_negative_loglikelihood(self):
        """idlma.py:233-246.  Syncs to return a float."""
        return np.float64(self._device_loss().item())
