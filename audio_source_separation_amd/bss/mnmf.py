"""FastMNMF and Sawada's MNMF on MI355X (DESIGN.md sections 9 and 10).

`FastMultichannelISNMF` is the drop-in for the reference class of the same name (`src/bss/mnmf.py`:
637-946): every step of its iteration -- the NMF update of basis and activation, the spatial-covariance update, the
diagonaliser update and the 'power' normalisation -- and its loss and `separate` run as HIP kernels
(csrc/assx_fastmnmf.hip); without callbacks the whole loop is one library call (assx_fastmnmf_iterate).  Its output
is `separate(input)`, (n_sources, n_bins, n_frames): the sources' images at channel `reference_id`.

`MultichannelISNMF` is the drop-in for the reference class of the same name (mnmf.py:115-617, Sawada's full-rank
MNMF): its four updates, loss and `separate` run as HIP kernels (csrc/assx_mnmf.hip), and without callbacks the loop is
one library call (assx_mnmf_iterate).

`update_diagonalizer` (mnmf.py:848-888) is also offered as a free function for callers that keep their NMF model
elsewhere: a weighted covariance per CHANNEL m -- weights R[f,t,m] = sum_n Lambda[n,f,t] g[n,f,m] -- followed by the
iterative-projection sweep with the normaliser floored at eps, on the very kernels of the ILRMA spatial update.
"""
import numpy as np

from .._device import to_device, to_numpy, torch
from .._loss import LazyLossList, append_loss
from .._state import DeviceArray, DeviceState
from .. import _lib
from ..algorithm.projection_back import _engine

EPS = 1e-12
THRESHOLD = 1e+12


def source_variance(basis, activation, latent=None):
    """Lambda (n_sources, n_bins, n_frames) as update_diagonalizer forms it (mnmf.py:858-866): W @ H, or with a
    partitioning function (latent Z (n_sources, n_basis), shared W (n_bins, n_basis), H (n_basis, n_frames))
    (Z[:, None, :] * W[None]) @ H.  Host-side convenience: a caller that keeps its NMF model elsewhere passes
    `variance=` to update_diagonalizer instead."""
    if latent is not None:
        return (latent[:, None, :] * basis[None, :, :]) @ activation[None, :, :]
    return basis @ activation


def update_diagonalizer(input, diagonalizer, spatial_covariance, variance=None, basis=None, activation=None, latent=None,
                        eps=EPS, threshold=THRESHOLD, *, dtype='float64', device=None):
    """
    Args:
        input (n_channels, n_bins, n_frames) complex
        diagonalizer Q (n_bins, n_channels, n_channels) complex (not modified)
        spatial_covariance g (n_sources, n_bins, n_channels) real
        variance Lambda (n_sources, n_bins, n_frames) real, or (basis, activation[, latent]) to form it
    Returns:
        Q after the sweep over the channels (mnmf.py:872-886).
    """
    if variance is None:
        if basis is None or activation is None:
            raise ValueError("Specify `variance` or (`basis`, `activation`).")
        variance = source_variance(np.asarray(basis), np.asarray(activation), None if latent is None else np.asarray(latent))
    eng = _engine(dtype, device)
    X = to_device(input, eng.prec.cplx, eng.dev)
    Q = to_device(diagonalizer, eng.prec.cplx, eng.dev)
    L = to_device(variance, eng.prec.real, eng.dev)
    g = to_device(spatial_covariance, eng.prec.real, eng.dev)
    batched = X.dim() == 4
    if not batched:
        X, Q, L, g = X.unsqueeze(0), Q.unsqueeze(0), L.unsqueeze(0), g.unsqueeze(0)
    B, M, F, T = (int(v) for v in X.shape)
    N = int(L.shape[1])
    if tuple(Q.shape) != (B, F, M, M) or tuple(L.shape) != (B, N, F, T) or tuple(g.shape) != (B, N, F, M):
        raise ValueError("shapes do not match: input {}, diagonalizer {}, variance {}, spatial_covariance {}".format(
            tuple(X.shape), tuple(Q.shape), tuple(L.shape), tuple(g.shape)))
    Q = Q.contiguous().clone()
    status = eng.new_status(B)
    eng.fastmnmf_update_diagonalizer(X.contiguous(), Q, L.contiguous(), g.contiguous(), eps=eps, threshold=threshold,
                                     status=status)
    if int(status.max().item()) & _lib.STATUS_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")
    if isinstance(input, torch.Tensor) and isinstance(diagonalizer, torch.Tensor):
        return Q if batched else Q[0]
    Q = to_numpy(Q, np.complex128)
    return Q if batched else Q[0]


class MultichannelNMFbase(DeviceState):
    """
    What the multichannel NMF models share (reference: mnmf.py:25-113): the constructor state, the parsing, limits and
    upload of the input, the warm-start check, the workspace cache, the loss record, `separate` and the loop.

    A model supplies its DeviceArray attributes and
        _reset(**kwargs)        the initial draws, built from the helpers below in the model's own order
        _update_once_dev()      one iteration in the step loop
        _run_fast_loop(n)       the whole loop as ONE library call
        _loss_dev()             the loss (B,) as a float64 device tensor
        _separate_dev(X)        the sources' images (B, n_sources, n_bins, n_frames) at channel `reference_id`
        _OWN_STEPS              the methods whose override sends the loop back to the step loop (DeviceState._fast_loop_ok)
    """
    MAX_CHANNELS, MAX_SOURCES, MAX_BASIS = 8, 8, 64

    _LABEL = None                  # the model's name in the messages of the limit checks
    _SAMPLES_NOTE = ""             # follows "n_frames < 268435456" in the message of the 2^28 limit
    _CALLBACKS_BEFORE_LOOP = True  # mnmf.py:80-82; FastMNMF's own __call__ (mnmf.py:691-735) has no such call

    def __init__(self, n_basis=10, n_sources=None, callbacks=None, reference_id=0, recordable_loss=True, eps=EPS, *,
                 dtype='float64', device=None):
        if callbacks is not None:
            if callable(callbacks):
                callbacks = [callbacks]
            self.callbacks = callbacks
        else:
            self.callbacks = None

        self.eps = eps
        self.n_basis = n_basis
        self.n_sources = n_sources

        self.input = None
        self.recordable_loss = recordable_loss
        if self.recordable_loss:
            self.loss = LazyLossList()  # a list; entries are materialised from HBM on first read
        else:
            self.loss = None

        self.reference_id = reference_id

        self.dtype = dtype
        self.device = device
        self._engine = None
        self._ws = None
        self._ws_key = None

    # ---- the pieces of _reset ----------------------------------------------------------------------------------------
    def _parse_input(self, **kwargs):
        """mnmf.py:49-63: keywords become attributes; (batched, B, n_channels, n_bins, n_frames, n_sources) of the input."""
        assert self.input is not None, "Specify data!"

        for key in kwargs.keys():
            setattr(self, key, kwargs[key])

        shape = self._shape_of(self.input)
        ndim = len(shape)
        if ndim not in (3, 4):
            raise ValueError("input must be (n_channels, n_bins, n_frames), got {} dims".format(ndim))
        B, n_channels, n_bins, n_frames = (1,) * (4 - ndim) + shape

        n_sources = self.n_sources
        if n_sources is None:
            n_sources = n_channels
        return ndim == 4, B, n_channels, n_bins, n_frames, n_sources

    def _check_limits(self, n_channels, n_sources, n_bins, n_frames):
        """Raises before anything is uploaded."""
        label, n_basis = self._LABEL, self.n_basis
        if not (2 <= n_channels <= self.MAX_CHANNELS and 1 <= n_sources <= self.MAX_SOURCES
                and 1 <= n_basis <= self.MAX_BASIS):
            raise ValueError("{} supports 2 <= n_channels <= {}, 1 <= n_sources <= {} and "
                             "1 <= n_basis <= {}; got n_channels={}, n_sources={}, n_basis={}".format(
                                 label, self.MAX_CHANNELS, self.MAX_SOURCES, self.MAX_BASIS, n_channels, n_sources,
                                 n_basis))
        if n_channels * n_bins * n_frames >= 1 << 28:
            raise ValueError("{}: one utterance must stay below 2^28 samples (n_channels * n_bins * "
                             "n_frames < 268435456{}); got {} x {} x {}".format(label, self._SAMPLES_NOTE, n_channels,
                                                                                 n_bins, n_frames))

    def _set_sizes(self, n_channels, n_sources, n_bins, n_frames):
        self.n_sources, self.n_channels = n_sources, n_channels
        self.n_bins, self.n_frames = n_bins, n_frames

    def _upload_input(self, batched):
        eng = self._ensure_engine()
        self._batched = batched
        self._X = self._upload(self.input, eng.prec.cplx)

    def _check_warm_start(self, table, copy=False):
        """table: (device name, attribute name, expected shape with the utterance axis, complex) per array.  The
        kernels take pointers and sizes: a warm-start array of another shape would be read past its end.  copy: the
        model owns its arrays afterwards, so it never writes into the caller's."""
        lead = 0 if self._batched else 1
        for name, attr, shape, cplx in table:
            got = tuple(self._dev(name, cplx).shape)
            if got != shape:
                raise ValueError("{}: expected shape {}, got {}".format(attr, shape[lead:], got[lead:]))
            if copy:
                self._set_dev(name, self._dev(name, cplx).contiguous().clone())

    def _ensure_workspace(self, key, alloc):
        """alloc(B, n_channels, n_sources, n_bins, n_frames, n_basis) runs only when `key` changes."""
        if self._ws_key != key:
            self._ws = alloc(*key[:6])
            self._ws_key = key

    # ---- loss, status, callbacks -----------------------------------------------------------------------------------
    def _record_loss(self):
        append_loss(self.loss, self._loss_dev(), self._batched)

    def compute_negative_loglikelihood(self):
        """mnmf.py:538-552 (in closed form) / 890-917.  Syncs to return a Python float (an array of B with a batch
        axis)."""
        loss = self._loss_dev()
        if self._batched:
            return to_numpy(loss, np.float64)
        return np.float64(loss.item())

    def _run_callbacks(self):
        if self.callbacks is not None:
            self._check_status()
            self._set_dev("Y", self._separate_dev(self._X))
            for callback in self.callbacks:
                callback(self)

    # ---- the loop ----------------------------------------------------------------------------------------------------
    def __call__(self, input, iteration=100, **kwargs):
        """
        Args:
            input (n_channels, n_bins, n_frames)
        Returns:
            output (n_sources, n_bins, n_frames)
        """
        self.input = input

        self._reset(**kwargs)

        if iteration > 0 and self._fast_loop_ok():
            # nothing observes the model between iterations: the loop is ONE call into the library (its *_iterate entry
            # enqueues the same entry points in the same order: bit-identical to the loop below)
            self._run_fast_loop(iteration)
        else:
            if self.recordable_loss:
                self._record_loss()
            if self._CALLBACKS_BEFORE_LOOP:
                self._run_callbacks()

            for idx in range(iteration):
                self._update_once_dev()

                if self.recordable_loss:
                    self._record_loss()
                self._run_callbacks()
        self._check_status()

        Y = self._separate_dev(self._X)
        self._set_dev("Y", Y)
        if isinstance(input, torch.Tensor):
            return self._unbatch(Y)
        return self.estimation

    def _reset(self, **kwargs):
        raise NotImplementedError("Implement '_reset' method")

    def _update_once_dev(self):
        raise NotImplementedError("Implement '_update_once_dev' method")

    def update_once(self):
        raise NotImplementedError("Implement 'update_once' method")

    def separate(self, input):
        """mnmf.py:554-583 / 919-946: (n_sources, n_bins, n_frames), the sources' images at channel `reference_id`."""
        eng = self._ensure_engine()
        X = to_device(input, eng.prec.cplx, eng.dev)
        batched = X.dim() == 4
        if not batched:
            X = X.unsqueeze(0)
        Y = self._separate_dev(X.contiguous())
        if isinstance(input, torch.Tensor):
            return Y if batched else Y[0]
        Y = to_numpy(Y, np.complex128)
        return Y if batched else Y[0]


class FastMultichannelISNMF(MultichannelNMFbase):
    """
    Reference: "Fast Multichannel Source Separation Based on Jointly Diagonalizable Spatial Covariance Matrices"
    (mnmf.py:637-946).  Supported: 2 <= n_channels <= 8, 1 <= n_sources <= 8, 1 <= n_basis <= 64.

    `basis` (n_sources, n_bins, n_basis), `activation` (n_sources, n_basis, n_frames), `spatial_covariance`
    (n_sources, n_bins, n_channels), `diagonalizer` (n_bins, n_channels, n_channels), `latent` and `estimation` live on
    the device and read as NumPy arrays (an in-place edit reaches the next kernel).  A leading utterance axis on the
    input, (B, n_channels, n_bins, n_frames), adds one to every attribute and to the output.  One utterance must stay
    below 2^28 samples (n_channels * n_bins * n_frames).  Arrays that do not fit the input -- a `separate` input of
    other sizes than the fitted model, a reassigned attribute of another shape -- raise ValueError.
    """
    basis = DeviceArray("W", complex_=False)
    activation = DeviceArray("H", complex_=False)
    spatial_covariance = DeviceArray("g", complex_=False)
    diagonalizer = DeviceArray("Q", complex_=True)
    latent = DeviceArray("Z", complex_=False)
    estimation = DeviceArray("Y", complex_=True)

    _LABEL = "FastMultichannelISNMF"
    _SAMPLES_NOTE = ": 4 GiB in complex128"
    _CALLBACKS_BEFORE_LOOP = False

    def __init__(self, n_basis=10, n_sources=None, partitioning=False, normalize='power', reference_id=0, callbacks=None,
                 recordable_loss=True, eps=EPS, threshold=THRESHOLD, *, dtype='float64', device=None):
        super().__init__(n_basis=n_basis, n_sources=n_sources, callbacks=callbacks, reference_id=reference_id,
                         recordable_loss=recordable_loss, eps=eps, dtype=dtype, device=device)

        self.partitioning = partitioning
        self.normalize = normalize

        self.threshold = threshold

        self._xt_src = None

    def _reset(self, **kwargs):
        """mnmf.py:47-61, 653-689: Q and g are reset on every call; basis / activation (and latent) only when absent."""
        batched, B, n_channels, n_bins, n_frames, n_sources = self._parse_input(**kwargs)
        eng = self._ensure_engine()
        self._set_sizes(n_channels, n_sources, n_bins, n_frames)
        n_basis = self.n_basis
        self._check_limits(n_channels, n_sources, n_bins, n_frames)
        self._upload_input(batched)

        Q = torch.eye(n_channels, dtype=eng.prec.cplx, device=eng.dev).repeat(B, n_bins, 1, 1)
        G = np.ones((n_sources, n_bins, n_channels)) * 1e-2
        for m in range(n_channels):
            G[m % n_sources, :, m] = 1
        G = to_device(G, eng.prec.real, eng.dev).unsqueeze(0).repeat(B, 1, 1, 1)

        lead = (B,) if self._batched else ()
        if self.partitioning:
            self._keep_or_draw('latent', lambda: np.ones(lead + (n_sources, n_basis), dtype=np.float64) / n_sources)
            self._keep_or_draw('basis', lambda: np.random.rand(*(lead + (n_bins, n_basis))))
            self._keep_or_draw('activation', lambda: np.random.rand(*(lead + (n_basis, n_frames))))
            table = [("Z", "latent", (B, n_sources, n_basis), False), ("W", "basis", (B, n_bins, n_basis), False),
                     ("H", "activation", (B, n_basis, n_frames), False)]
        else:
            self._keep_or_draw('basis', lambda: np.random.rand(*(lead + (n_sources, n_bins, n_basis))))
            self._keep_or_draw('activation', lambda: np.random.rand(*(lead + (n_sources, n_basis, n_frames))))
            table = [("W", "basis", (B, n_sources, n_bins, n_basis), False),
                     ("H", "activation", (B, n_sources, n_basis, n_frames), False)]
        self._check_warm_start(table)
        self._set_dev("Q", Q.contiguous())
        self._set_dev("g", G.contiguous())

        self._ensure_workspace((B, n_channels, n_sources, n_bins, n_frames, n_basis, eng.prec.name),
                               eng.fastmnmf_workspace)
        self._xt_src = None
        self._status = eng.new_status(B)

    # ---- device views of the model ---------------------------------------------------------------------------------
    def _model(self):
        """(W, H, g, Q) as the kernels read them: with a partitioning function, Lambda = (Z W) H expanded per source."""
        W, H = self._dev("W", False), self._dev("H", False)
        if self.partitioning:
            eng = self._engine
            Z = self._dev("Z", False)
            if Z.dim() != 3 or W.dim() != 3 or H.dim() != 3:
                raise ValueError("partitioning: expected latent (n_sources, n_basis), basis (n_bins, n_basis) and "
                                 "activation (n_basis, n_frames)")
            B, N, K = (int(s) for s in Z.shape)
            F, T = int(W.shape[1]), int(H.shape[2])
            if tuple(W.shape) != (B, F, K) or tuple(H.shape) != (B, K, T):
                raise ValueError("partitioning: latent {}, basis {} and activation {} do not fit together".format(
                    tuple(Z.shape), tuple(W.shape), tuple(H.shape)))
            Weff, Heff = eng.empty((B, N, F, K)), eng.empty((B, N, K, T))
            eng.ilrma_expand_partitioned(Z, W, H, Weff, Heff)
            W, H = Weff, Heff
        return W, H, self._dev("g", False), self._dev("Q", True)

    def _ensure_xt(self):
        """x~ = |Q x|^2 of the current diagonaliser in the model's workspace (P1 of DESIGN.md section 9)."""
        Q = self._dev("Q", True)
        if self._xt_src is not Q:
            W, H, g, _ = self._model()
            self._engine.fastmnmf_project(self._X, Q, W, H, g, self._ws, eps=self.eps)
            self._xt_src = Q

    def _loss_dev(self):
        W, H, g, Q = self._model()
        loss = self._engine.empty((int(self._X.shape[0]),), dtype=torch.float64)
        self._engine.fastmnmf_project(self._X, Q, W, H, g, self._ws, eps=self.eps, loss=loss)
        self._xt_src = Q
        return loss

    # ---- the loop ----------------------------------------------------------------------------------------------------
    _OWN_STEPS = ("update_once", "update_NMF", "update_SCM", "update_diagonalizer", "compute_negative_loglikelihood",
                  "_record_loss")

    def _fast_loop_ok(self):
        """DeviceState's rule, and what assx_fastmnmf_iterate knows: no partitioning function, 'power' or nothing."""
        return super()._fast_loop_ok() and not self.partitioning and self.normalize in (False, None, 0, '', 'power')

    def _run_fast_loop(self, iteration):
        W, H, g, Q = self._model()
        loss = self._iterate_block(iteration + 1, ("W", "H", "g", "Q"), lambda loss: self._engine.fastmnmf_iterate(
            iteration, self._X, Q, W, H, g, self._ws, normalize=bool(self.normalize), eps=self.eps,
            threshold=self.threshold, status=self._status, loss=loss))
        self._xt_src = Q if loss is not None else None  # the last projection ran only to record the last loss

    def __repr__(self):
        s = "FastMNMF("
        s += "n_basis={n_basis}"
        if hasattr(self, 'n_sources'):
            s += ", n_sources={n_sources}"
        if hasattr(self, 'n_channels'):
            s += ", n_channels={n_channels}"
        s += ", partitioning={partitioning}"
        s += ", normalize={normalize}"
        s += ")"

        return s.format(**self.__dict__)

    def _update_once_dev(self):
        self.update_once()  # the step loop runs the public method, whatever a subclass made of it

    def update_once(self):
        """mnmf.py:737-773"""
        self.update_NMF()
        self.update_SCM()
        self.update_diagonalizer()
        if self.normalize:
            if self.normalize == 'power':
                if self.partitioning:
                    raise ValueError("Not support partitioning function.")
                W, H, g, Q = self._model()
                self._engine.fastmnmf_normalize_power(self._X, Q, W, H, g, eps=self.eps)
                self._touch("W", "H", "g", "Q")
                self._xt_src = None
            else:
                raise ValueError("Not support normalization based on {}. Choose 'power'".format(self.normalize))

    def update_NMF(self):
        """mnmf.py:775-815: basis half, then the activation half with the new basis."""
        if self.partitioning:
            raise ValueError("Not support partitioning function.")
        self._ensure_xt()
        W, H, g, _ = self._model()
        self._engine.fastmnmf_update_nmf(self._X, W, H, g, self._ws, eps=self.eps)
        self._touch("W", "H")

    def update_SCM(self):
        """mnmf.py:817-846"""
        if self.partitioning:
            raise ValueError("Not support partitioning function.")
        self._ensure_xt()
        W, H, g, _ = self._model()
        self._engine.fastmnmf_update_scm(self._X, W, H, g, self._ws, eps=self.eps)
        self._touch("g")

    def update_diagonalizer(self):
        """mnmf.py:848-888, with R formed from the model on the fly."""
        W, H, g, Q = self._model()
        self._engine.fastmnmf_update_diagonalizer_model(self._X, Q, W, H, g, self._ws, eps=self.eps,
                                                        threshold=self.threshold, status=self._status)
        self._touch("Q")
        self._xt_src = None

    def _separate_dev(self, X):
        W, H, g, Q = self._model()
        status = self._engine.new_status(int(X.shape[0]))
        Y = self._engine.fastmnmf_separate(X, Q, W, H, g, ref=self.reference_id, eps=self.eps, status=status)
        if int(status.max().item()) & _lib.STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        return Y


class MultichannelISNMF(MultichannelNMFbase):
    """
    Reference: Sawada's MNMF, "Multichannel Extensions of Non-Negative Matrix Factorization With Complex-Valued Data"
    (mnmf.py:115-617).  Supported: author='Sawada', float64, 2 <= n_channels <= 8, 1 <= n_sources <= 8,
    1 <= n_basis <= 64 and n_channels * n_bins * n_frames < 2^28.

    `basis` (n_bins, n_basis), `activation` (n_basis, n_frames), `latent` (n_sources, n_basis), `spatial`
    (n_bins, n_sources, n_channels, n_channels) complex and `estimation` (n_sources, n_bins, n_frames) live on the
    device and read as NumPy arrays.  A leading utterance axis on the input, (B, n_channels, n_bins, n_frames), adds
    one to every attribute and to the output.  The loss is the exact value of the reference's log-det divergence
    (DESIGN.md section 10): the reference's own value carries about 1e-6 relative noise from an eigenvalue solver.
    """
    basis = DeviceArray("Tb", complex_=False)
    activation = DeviceArray("V", complex_=False)
    latent = DeviceArray("Z", complex_=False)
    spatial = DeviceArray("H", complex_=True)
    estimation = DeviceArray("Y", complex_=True)

    _LABEL = "MultichannelISNMF"

    def __init__(self, n_basis=10, n_sources=None, normalize=True, callbacks=None, reference_id=0, author='Sawada',
                 recordable_loss=True, eps=EPS, *, dtype='float64', device=None, **kwargs):
        super().__init__(n_basis=n_basis, n_sources=n_sources, callbacks=callbacks, reference_id=reference_id,
                         recordable_loss=recordable_loss, eps=eps, dtype='float64', device=device)

        self.normalize = normalize

        if not isinstance(author, str) or author.lower() not in ('sawada', 'ozerov'):
            raise ValueError("Choose from ['sawada', 'ozerov']")
        if author.lower() != 'sawada':
            raise ValueError("MultichannelISNMF: only Sawada's MNMF is supported (the reference marks Ozerov's as in "
                             "progress)")
        self.author = author

        if set(kwargs) != set():
            raise ValueError("Invalid keywords.")
        if not isinstance(reference_id, (int, np.integer)) or reference_id < 0:
            raise ValueError("reference_id must be a non-negative int, got {!r}".format(reference_id))

        self._require_float64(dtype, complex_ok=True)

    def _reset(self, **kwargs):
        """mnmf.py:47-61, 183-240: latent, spatial, basis and activation are drawn (in that order) only when absent."""
        batched, B, n_channels, n_bins, n_frames, n_sources = self._parse_input(**kwargs)
        n_basis = self.n_basis
        self._check_limits(n_channels, n_sources, n_bins, n_frames)
        if not 0 <= self.reference_id < n_channels:
            raise ValueError("reference_id must be in [0, {}), got {}".format(n_channels, self.reference_id))
        self._set_sizes(n_channels, n_sources, n_bins, n_frames)
        self._upload_input(batched)

        lead = (B,) if self._batched else ()
        eps = self.eps
        if not hasattr(self, 'latent'):
            Z = np.random.rand(*(lead + (n_sources, n_basis))) * 1e-2 + 1 / n_sources
            Zsum = Z.sum(axis=-2, keepdims=True)
            Zsum[Zsum < eps] = eps
            self.latent = Z / Zsum
        self._keep_or_draw('spatial', lambda: np.tile(np.eye(n_channels, dtype=np.complex128),
                                                      lead + (n_bins, n_sources, 1, 1)))
        self._keep_or_draw('basis', lambda: np.random.rand(*(lead + (n_bins, n_basis))))
        self._keep_or_draw('activation', lambda: np.random.rand(*(lead + (n_basis, n_frames))))
        # warm-start values are copied (mnmf.py:212-233)
        self._check_warm_start([("Z", "latent", (B, n_sources, n_basis), False),
                                ("H", "spatial", (B, n_bins, n_sources, n_channels, n_channels), True),
                                ("Tb", "basis", (B, n_bins, n_basis), False),
                                ("V", "activation", (B, n_basis, n_frames), False)], copy=True)

        eng = self._engine
        self._ensure_workspace((B, n_channels, n_sources, n_bins, n_frames, n_basis), eng.mnmf_workspace)
        self._status = eng.new_status(B)

    def _model(self):
        return self._dev("Tb", False), self._dev("V", False), self._dev("Z", False), self._dev("H", True)

    def _loss_dev(self):
        Tb, V, Z, H = self._model()
        return self._engine.mnmf_loss(self._X, Tb, V, Z, H, self._ws, eps=self.eps, status=self._status)

    # ---- the loop ----------------------------------------------------------------------------------------------------
    _OWN_STEPS = ("update_once", "_update_once_dev", "update_basis_sawada", "update_activation_sawada",
                  "update_latent_sawada", "update_spatial_sawada", "compute_negative_loglikelihood", "_record_loss")

    def _run_fast_loop(self, iteration):
        self._iterate_block(iteration + 1, ("Tb", "V", "Z", "H"), lambda loss: self._engine.mnmf_iterate(
            iteration, self._X, *self._model(), self._ws, normalize=bool(self.normalize), eps=self.eps,
            status=self._status, loss=loss))

    def __repr__(self):
        s = "IS-MNMF("
        s += "n_basis={n_basis}"
        if hasattr(self, 'n_sources'):
            s += ", n_sources={n_sources}"
        if hasattr(self, 'n_channels'):
            s += ", n_channels={n_channels}"
        s += ", normalize={normalize}"
        s += ", author={author}"
        s += ")"

        return s.format(**self.__dict__)

    def _update_once_dev(self):
        self.update_basis_sawada()
        self.update_activation_sawada()
        self.update_latent_sawada()
        self.update_spatial_sawada()

    def update_once(self):
        """mnmf.py:291-302: the four updates, then the estimation of the new model."""
        self._update_once_dev()
        self._check_status()
        self._set_dev("Y", self._separate_dev(self._X))

    def update_once_sawada(self):
        self._update_once_dev()

    def update_basis_sawada(self):
        """mnmf.py:431-451"""
        Tb, V, Z, H = self._model()
        self._engine.mnmf_update_basis(self._X, Tb, V, Z, H, self._ws, eps=self.eps, status=self._status)
        self._touch("Tb")

    def update_activation_sawada(self):
        """mnmf.py:453-473"""
        Tb, V, Z, H = self._model()
        self._engine.mnmf_update_activation(self._X, Tb, V, Z, H, self._ws, eps=self.eps, status=self._status)
        self._touch("V")

    def update_latent_sawada(self):
        """mnmf.py:475-497"""
        Tb, V, Z, H = self._model()
        self._engine.mnmf_update_latent(self._X, Tb, V, Z, H, self._ws, eps=self.eps, status=self._status)
        self._touch("Z")

    def update_spatial_sawada(self):
        """mnmf.py:499-525"""
        Tb, V, Z, H = self._model()
        self._engine.mnmf_update_spatial(self._X, Tb, V, Z, H, self._ws, normalize=bool(self.normalize),
                                         eps=self.eps, status=self._status)
        self._touch("H")

    def _separate_dev(self, X):
        Tb, V, Z, H = self._model()
        status = self._engine.new_status(int(X.shape[0]))
        Y = self._engine.mnmf_separate(X, Tb, V, Z, H, ref=self.reference_id, eps=self.eps, status=status)
        if int(status.max().item()) & _lib.STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        return Y
