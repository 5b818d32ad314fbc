"""Thin, typed wrappers over the C-ABI working on batched device tensors.

Shapes follow include/assx.h (leading utterance axis B):  X (B,M,F,T) complex, W (B,F,N,M) complex,
Tb (B,N,F,K), V (B,N,K,T), U (B,N,F,M,M), Y (B,N,F,T).  Every method launches asynchronously on
torch's current stream for the engine's device; none of them synchronises.
"""
import ctypes

import torch

from . import _lib
from ._device import Precision, Workspace, context, ptr, require_gpu, stream_ptr

_RAW = _lib.lib


# ---------------------------------------------------------------------- argument checks of the factorisation models
# The C-ABI takes pointers and sizes, and its kernels write float64, int32 or the model's own type through them.  An
# array of another shape, dtype or device, or a strided view -- a separate() input longer than the fitted activation, a
# batched input on an unbatched model, a reassigned attribute, a float32 `loss`, a `status` left on the CPU -- would be
# read or written past its end.  Every array and workspace of FastMNMF, MNMF, ComplexEUCNMF, EUCNTF, LDPSDTF, the
# two IPSDTA models, the covariance-domain MNMF, the gradient IVA / FDICA, the ProxLaplaceIVA, the beamformer / PCA / MDP and the IDLMA entry points passes one of the two checks below, where all of that is still known, and is refused with ValueError
# before anything is launched.
def check_array(model, name, a, dtype, device, shape=None, numel=None):
    """`a` must be a contiguous `dtype` tensor on `device`: of exactly `shape`, or (shape None) of at least `numel`
    elements, any shape."""
    if a.dtype != dtype or a.device != device:
        raise ValueError("%s: %s must be %s on %s, got %s on %s" % (model, name, dtype, device, a.dtype, a.device))
    fits = tuple(a.shape) == tuple(shape) if shape is not None else a.numel() >= numel
    if not (fits and a.is_contiguous()):
        need = "shape %s" % (tuple(shape),) if shape is not None else "at least %d elements" % numel
        raise ValueError("%s: %s has shape %s%s, needs %s (contiguous)"
                         % (model, name, tuple(a.shape), "" if a.is_contiguous() else " (not contiguous)", need))


def check_workspace(model, ws, device, need):
    """`ws` must hold at least `need` contiguous bytes as torch.uint8 on `device`; `need` is what the library's
    *_workspace_bytes reports, 0 for sizes outside the model's envelope."""
    if need == 0:
        raise ValueError("%s: workspace for sizes that the model does not support" % model)
    if ws.dtype != torch.uint8 or ws.device != device or ws.numel() < need or not ws.is_contiguous():
        raise ValueError("%s: workspace of %d x %s%s on %s, needs at least %d contiguous bytes of torch.uint8 on %s"
                         % (model, ws.numel(), ws.dtype, "" if ws.is_contiguous() else " (not contiguous)", ws.device,
                            need, device))


class _DeviceGuardedLib:
    """libassx entry points called with the engine's device made current for the duration of the call.

    The C library never switches devices (it refuses a call whose context device is not current); torch owns the
    calling thread's current device, so a model built with device='cuda:1' while cuda:0 is current -- or two models
    on different GPUs in one process -- are handled here, not by the caller."""

    def __init__(self, dev):
        self._dev = dev

    def __getattr__(self, name):
        fn = getattr(_RAW, name)
        dev, index = self._dev, self._dev.index

        def call(*args):
            if torch.cuda.current_device() == index:
                return fn(*args)
            with torch.cuda.device(dev):
                return fn(*args)

        call.__name__ = name
        setattr(self, name, call)
        return call


class Engine:
    def __init__(self, dtype="float64", device=None):
        self.dev = require_gpu(device)
        self.prec = Precision(dtype)
        context(self.dev)  # fail here, not at the first kernel, if the device cannot be opened
        self._ws = Workspace(self.dev)
        self._L = _DeviceGuardedLib(self.dev)

    @property
    def ctx(self):
        """The CALLING thread's context for this engine's device (contexts are per thread, include/assx.h)."""
        return context(self.dev)

    # ------------------------------------------------------------------ helpers
    def _check(self, rc, what):
        _lib.check(self.ctx, rc, what)

    def _scratch(self, B, M, F, T, K):
        n = self._L.assx_workspace_bytes(B, M, F, T, max(int(K), 1), self.prec.code)
        return self._ws.get(n)

    def _st(self):
        return stream_ptr(self.dev)

    def empty(self, shape, complex_=False, dtype=None):
        dt = dtype if dtype is not None else (self.prec.cplx if complex_ else self.prec.real)
        return torch.empty(shape, dtype=dt, device=self.dev)

    def new_status(self, B):
        return torch.zeros(B, dtype=torch.int32, device=self.dev)

    @staticmethod
    def _dims(X):
        B, M, F, T = X.shape
        return int(B), int(M), int(F), int(T)

    # ------------------------------------------------------------------ (a3)
    @staticmethod
    def _model_shapes(X, W=None, Tb=None, V=None):
        """The C-ABI takes pointers and sizes: a model array of another shape would be read past its end (a partitioned
        basis (F, K) handed to an entry point that reads (N, F, K) was found as an intermittent memory fault).  Refuse it
        here, where the shapes are still known."""
        B, M, F, T = (int(d) for d in X.shape)
        if W is not None and tuple(W.shape) != (B, F, M, M):
            raise ValueError("demix_filter: expected shape %s, got %s" % ((B, F, M, M), tuple(W.shape)))
        if Tb is not None:
            K = int(Tb.shape[-1])
            if tuple(Tb.shape) != (B, M, F, K):
                raise ValueError("basis: expected shape %s, got %s" % ((B, M, F, K), tuple(Tb.shape)))
            if V is not None and tuple(V.shape) != (B, M, K, T):
                raise ValueError("activation: expected shape %s, got %s" % ((B, M, K, T), tuple(V.shape)))

    def demix(self, X, W, scale=None, out=None):
        B, M, F, T = self._dims(X)
        Y = out if out is not None else self.empty((B, M, F, T), complex_=True)
        self._check(self._L.assx_demix(self.ctx, ptr(X), ptr(W), ptr(scale), ptr(Y), B, M, F, T, self.prec.code, self._st()),
                    "assx_demix")
        return Y

    # ------------------------------------------------------------------ (a4)
    def cov_accumulate(self, X, r=None, eps=1e-12):
        """r: None (plain covariance, returns (B,1,F,M,M)), (B,N,T) or (B,N,F,T)."""
        B, M, F, T = self._dims(X)
        if r is None:
            kind, N = _lib.W_NONE, 1
        elif r.dim() == 3:
            kind, N = _lib.W_NT, int(r.shape[1])
        else:
            kind, N = _lib.W_NFT, int(r.shape[1])
        U = self.empty((B, N, F, M, M), complex_=True)
        ws = self._scratch(B, M, F, T, 1)
        self._check(self._L.assx_cov_accumulate(self.ctx, ptr(X), ptr(r), kind, float(eps), ptr(U), ptr(ws), B, M, N, F, T,
                                          self.prec.code, self._st()), "assx_cov_accumulate")
        return U

    # ------------------------------------------------------------------ (a5)
    def ip_update(self, U, W, threshold=1e12, status=None):
        B, F, N, M = (int(s) for s in W.shape)
        self._check(self._L.assx_ip_update(self.ctx, ptr(U), ptr(W), float(threshold), ptr(status), B, M, F, self.prec.code,
                                     self._st()), "assx_ip_update")
        return W

    # ------------------------------------------------------------------ ILRMA
    def ilrma_source_update(self, X, W, Tb, V, domain=2, eps=1e-12, sources=None, loss_prev=None):
        """sources: None = all, or an iterable of source indices (pairwise update).
        loss_prev: optional (B,) float64 tensor receiving the loss of the model at entry (fused into the basis pass)."""
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        mask = (1 << M) - 1 if sources is None else sum(1 << int(n) for n in set(sources))
        self._check(self._L.assx_ilrma_source_update(self.ctx, ptr(X), ptr(W), ptr(Tb), ptr(V), float(domain), float(eps),
                                               mask, ptr(loss_prev), ptr(ws), B, M, F, T, K, self.prec.code,
                                               self._st()),
                    "assx_ilrma_source_update")

    # ---- partitioning function (shared bases + latent variables), domain 2
    def ilrma_expand_partitioned(self, Z, Tb, V, Teff, Veff):
        """Teff (B,N,F,K) = Z[n,k] Tb[f,k], Veff (B,N,K,T) = V[k,t]; either output may be None."""
        B, N, K = (int(s) for s in Z.shape)
        F, T = int(Tb.shape[1]), int(V.shape[2])
        self._check(self._L.assx_ilrma_expand_partitioned(self.ctx, ptr(Z), ptr(Tb), ptr(V), ptr(Teff), ptr(Veff), B, N, F,
                                                    T, K, self.prec.code, self._st()),
                    "assx_ilrma_expand_partitioned")

    def ilrma_source_update_partitioned(self, X, W, Z, Tb, V, Teff, Veff, eps=1e-12):
        B, M, F, T = self._dims(X)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_ilrma_source_update_partitioned(self.ctx, ptr(X), ptr(W), ptr(Z), ptr(Tb), ptr(V),
                                                           ptr(Teff), ptr(Veff), float(eps), ptr(ws), B, M, F, T, K,
                                                           self.prec.code, self._st()),
                    "assx_ilrma_source_update_partitioned")

    def ilrma_normalize_power_bins_partitioned(self, W, Z, Tb, power_bins, n_frames, eps=1e-12):
        B, F, N, M = (int(s) for s in W.shape)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, int(n_frames), K)
        self._check(self._L.assx_ilrma_normalize_power_bins_partitioned(self.ctx, ptr(W), ptr(Z), ptr(Tb), ptr(power_bins),
                                                                  float(eps), ptr(ws), B, M, F, K, self.prec.code,
                                                                  self._st()),
                    "assx_ilrma_normalize_power_bins_partitioned")

    def ip2_update(self, U, W, pair, threshold=1e12, status=None):
        B, F, N, M = (int(s) for s in W.shape)
        self._check(self._L.assx_ip2_update(self.ctx, ptr(U), ptr(W), float(threshold), ptr(status), int(pair[0]),
                                      int(pair[1]), B, M, F, self.prec.code, self._st()), "assx_ip2_update")
        return W

    def iss_update(self, U, W, n_frames):
        B, F, N, M = (int(s) for s in W.shape)
        self._check(self._L.assx_iss_update(self.ctx, ptr(U), ptr(W), int(n_frames), B, M, F, self.prec.code, self._st()),
                    "assx_iss_update")
        return W

    def ilrma_spatial_update(self, X, W, Tb, V, domain=2, eps=1e-12, threshold=1e12, status=None, U_out=None,
                             C=None, power_bins=None, spatial=_lib.SPATIAL_IP, pair=(0, 1)):
        """C (B,F,M,M) + power_bins (B,N,F) float64: also emit the per-bin power statistic of the updated filters."""
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_ilrma_spatial_update(self.ctx, int(spatial), int(pair[0]), int(pair[1]), ptr(X), ptr(W), ptr(Tb), ptr(V), float(domain), float(eps),
                                                float(threshold), ptr(U_out), ptr(C), ptr(power_bins), ptr(status),
                                                ptr(ws), B, M, F, T, K, self.prec.code, self._st()),
                    "assx_ilrma_spatial_update")

    def ilrma_cov_partials(self, X, Tb, V, domain=2, eps=1e-12):
        """ONE launch of the covariance-accumulate kernel (stage 1 of ilrma_spatial_update); for kernel timing."""
        B, M, F, T = self._dims(X)
        self._model_shapes(X, None, Tb, V)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_ilrma_cov_partials(self.ctx, ptr(X), ptr(Tb), ptr(V), float(domain), float(eps), ptr(ws),
                                              B, M, F, T, K, self.prec.code, self._st()), "assx_ilrma_cov_partials")

    def demix_power(self, X, W, out=None):
        B, M, F, T = self._dims(X)
        p = out if out is not None else self.empty((B, M))
        ws = self._scratch(B, M, F, T, 1)
        self._check(self._L.assx_demix_power(self.ctx, ptr(X), ptr(W), ptr(p), ptr(ws), B, M, F, T, self.prec.code,
                                       self._st()), "assx_demix_power")
        return p

    def power_from_cov(self, C, W, T_frames, out=None):
        B, F, N, M = (int(s) for s in W.shape)
        p = out if out is not None else self.empty((B, M))
        ws = self._scratch(B, M, F, int(T_frames), 1)
        self._check(self._L.assx_power_from_cov(self.ctx, ptr(C), ptr(W), ptr(p), ptr(ws), B, M, F, self.prec.code,
                                          self._st()), "assx_power_from_cov")
        return p

    def ilrma_normalize_power(self, W, Tb, power, domain=2, eps=1e-12):
        B, F, N, M = (int(s) for s in W.shape)
        K = int(Tb.shape[-1])
        self._check(self._L.assx_ilrma_normalize_power(self.ctx, ptr(W), ptr(Tb), ptr(power), float(domain), float(eps), B, M,
                                                 F, K, self.prec.code, self._st()), "assx_ilrma_normalize_power")

    def ilrma_normalize_power_bins(self, W, Tb, power_bins, domain=2, eps=1e-12):
        B, F, N, M = (int(s) for s in W.shape)
        K = int(Tb.shape[-1])
        self._check(self._L.assx_ilrma_normalize_power_bins(self.ctx, ptr(W), ptr(Tb), ptr(power_bins), float(domain),
                                                      float(eps), B, M, F, K, self.prec.code, self._st()),
                    "assx_ilrma_normalize_power_bins")

    def ilrma_normalize_pb(self, W, Tb, scale, domain=2):
        B, F, N, M = (int(s) for s in W.shape)
        K = int(Tb.shape[-1])
        self._check(self._L.assx_ilrma_normalize_pb(self.ctx, ptr(W), ptr(Tb), ptr(scale), float(domain), B, M, F, K,
                                              self.prec.code, self._st()), "assx_ilrma_normalize_pb")

    def ilrma_loss(self, X, W, Tb, V, domain=2, eps=1e-12, out=None):
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        loss = out if out is not None else self.empty((B,), dtype=torch.float64)
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_ilrma_loss(self.ctx, ptr(X), ptr(W), ptr(Tb), ptr(V), float(domain), float(eps), ptr(loss),
                                      ptr(ws), B, M, F, T, K, self.prec.code, self._st()), "assx_ilrma_loss")
        return loss

    # ------------------------------------------------------------------ whole loops in one call
    def nmf_iterate(self, n_iter, kind, X, Tb, V, domain=2, eps=1e-12, param=0.0, loss=None):
        """n_iter x (update, loss[i]); loss: (n_iter, B) float64 device tensor or None (criterion not evaluated)."""
        B, F, T = (int(s) for s in X.shape)
        K = int(Tb.shape[-1])
        ws = self._nmf_scratch(B, F, T, K)
        self._check(self._L.assx_nmf_iterate(self.ctx, int(n_iter), int(kind), float(domain), float(param), float(eps),
                                             ptr(X), ptr(Tb), ptr(V), ptr(loss), ptr(ws), B, F, T, K, self.prec.code,
                                             self._st()), "assx_nmf_iterate")

    def auxiva_iterate(self, n_iter, kind, X, W, r, eps=1e-12, threshold=1e12, status=None, loss=None,
                       spatial=_lib.SPATIAL_IP, pair=(0, 1)):
        """n_iter x (weights [+ loss[i]], covariance + sweep), then loss[n_iter]; loss: (n_iter + 1, B) float64 or None."""
        B, M, F, T = self._dims(X)
        ws = self._scratch(B, M, F, T, 1)
        self._check(self._L.assx_auxiva_iterate(self.ctx, int(n_iter), int(kind), int(spatial), int(pair[0]), int(pair[1]),
                                                ptr(X), ptr(W), float(eps), float(threshold), ptr(r), ptr(loss),
                                                ptr(status), ptr(ws), B, M, F, T, self.prec.code, self._st()),
                    "assx_auxiva_iterate")

    def ilrma_iterate(self, n_iter, X, W, Tb, V, domain=2, eps=1e-12, threshold=1e12, status=None, loss=None,
                      spatial=_lib.SPATIAL_IP, pair=(0, 1), normalize=0, C=None, power_bins=None, scale=None, ref=0,
                      pb_exponent=2.0):
        """n_iter x (source model, spatial model, normalisation); loss: (n_iter + 1, B) float64 or None.
        normalize: 0 none, 1 'power' (C + power_bins), 2 'projection-back' (scale scratch, ref, pb_exponent)."""
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_ilrma_iterate(self.ctx, int(n_iter), int(spatial), int(pair[0]), int(pair[1]),
                                               int(normalize), int(ref), float(pb_exponent), ptr(X), ptr(W), ptr(Tb),
                                               ptr(V), float(domain), float(eps), float(threshold), ptr(C),
                                               ptr(power_bins), ptr(scale), ptr(loss), ptr(status), ptr(ws), B, M, F,
                                               T, K, self.prec.code, self._st()), "assx_ilrma_iterate")

    # ------------------------------------------------------------------ STFT / iSTFT (row f3)
    def stft(self, x, window, fft_size, hop):
        """x (C, L) real -> X (C, fft_size//2+1, n_frames) complex; scipy.signal.stft semantics (include/assx.h)."""
        C, n = int(x.shape[0]), int(x.shape[1])
        T = int(self._L.assx_stft_num_frames(n, fft_size, hop))
        X = self.empty((C, fft_size // 2 + 1, max(T, 0)), complex_=True)
        ws = self._ws.get(self._L.assx_stft_workspace_bytes(C, fft_size, max(T, 1), self.prec.code))
        self._check(self._L.assx_stft(self.ctx, ptr(x), ptr(window), float(window.sum().item()), ptr(X), ptr(ws), C, n,
                                fft_size, hop, T, self.prec.code, self._st()), "assx_stft")
        return X

    def istft(self, X, window, fft_size, hop):
        """X (C, fft_size//2+1, n_frames) complex -> y (C, n_samples) real; scipy.signal.istft semantics."""
        C, F, T = (int(v) for v in X.shape)
        if F != fft_size // 2 + 1:
            raise ValueError("istft: {} bins do not match fft_size={}".format(F, fft_size))
        n = int(self._L.assx_istft_num_samples(fft_size, hop, T))
        y = self.empty((C, max(n, 0)))
        ws = self._ws.get(self._L.assx_stft_workspace_bytes(C, fft_size, T, self.prec.code))
        self._check(self._L.assx_istft(self.ctx, ptr(X), ptr(window), float(window.sum().item()), ptr(y), ptr(ws), C,
                                 fft_size, hop, T, self.prec.code, self._st()), "assx_istft")
        return y

    # ------------------------------------------------------------------ t-ILRMA
    def tilrma_source_update(self, X, W, Tb, V, nu, eps=1e-12):
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_tilrma_source_update(self.ctx, ptr(X), ptr(W), ptr(Tb), ptr(V), float(nu), float(eps),
                                                ptr(ws), B, M, F, T, K, self.prec.code, self._st()),
                    "assx_tilrma_source_update")

    def tilrma_spatial_update(self, X, W, Tb, V, nu, Xi, eps=1e-12, status=None, C=None, power_bins=None):
        """Xi: scratch (B,N,F,T) reals receiving the auxiliary weights."""
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_tilrma_spatial_update(self.ctx, ptr(X), ptr(W), ptr(Tb), ptr(V), float(nu), float(eps),
                                                 ptr(Xi), ptr(C), ptr(power_bins), ptr(status), ptr(ws), B, M, F, T,
                                                 K, self.prec.code, self._st()), "assx_tilrma_spatial_update")
        return W

    def tilrma_loss(self, X, W, Tb, V, nu, eps=1e-12, out=None):
        B, M, F, T = self._dims(X)
        self._model_shapes(X, W, Tb, V)
        K = int(Tb.shape[-1])
        loss = out if out is not None else self.empty((B,), dtype=torch.float64)
        ws = self._scratch(B, M, F, T, K)
        self._check(self._L.assx_tilrma_loss(self.ctx, ptr(X), ptr(W), ptr(Tb), ptr(V), float(nu), float(eps), ptr(loss),
                                       ptr(ws), B, M, F, T, K, self.prec.code, self._st()), "assx_tilrma_loss")
        return loss

    # ------------------------------------------------------------------ AuxIVA
    def auxiva_weights(self, X, W, kind, eps=1e-12, with_loss=False, out=None):
        B, M, F, T = self._dims(X)
        r = out if out is not None else self.empty((B, M, T))
        loss = self.empty((B,), dtype=torch.float64) if with_loss else None
        ws = self._scratch(B, M, F, T, 1)
        self._check(self._L.assx_auxiva_weights(self.ctx, ptr(X), ptr(W), int(kind), float(eps), ptr(r), ptr(loss), ptr(ws),
                                          B, M, F, T, self.prec.code, self._st()), "assx_auxiva_weights")
        return r, loss

    def auxiva_spatial_update(self, X, W, r, eps=1e-12, threshold=1e12, status=None, U_out=None,
                              spatial=_lib.SPATIAL_IP, pair=(0, 1)):
        B, M, F, T = self._dims(X)
        ws = self._scratch(B, M, F, T, 1)
        self._check(self._L.assx_auxiva_spatial_update(self.ctx, int(spatial), int(pair[0]), int(pair[1]), ptr(X), ptr(W), ptr(r), float(eps), float(threshold),
                                                 ptr(U_out), ptr(status), ptr(ws), B, M, F, T, self.prec.code,
                                                 self._st()), "assx_auxiva_spatial_update")

    # ------------------------------------------------------------------ other callers of cov + IP (row f4)
    def idlma_space_update(self, X, W, dnn_output, domain=2, eps=1e-12, threshold=1e12, status=None):
        """GaussIDLMA.update_space_model: W (B,F,N,M) in place from the source variances dnn_output (B,N,F,T)."""
        B, M, F, T = self._dims(X)
        ws = self._scratch(B, M, F, T, 1)
        scratch = None if float(domain) == 2.0 else self.empty((B, M, F, T))
        self._check(self._L.assx_idlma_space_update(self.ctx, ptr(X), ptr(W), ptr(dnn_output), float(domain), float(eps),
                                                    float(threshold), ptr(scratch), ptr(status), ptr(ws), B, M, F, T,
                                                    self.prec.code, self._st()), "assx_idlma_space_update")
        return W

    def fastmnmf_update_diagonalizer(self, X, Q, Lambda, g, eps=1e-12, threshold=1e12, status=None):
        """FastMultichannelISNMF.update_diagonalizer: Q (B,F,M,M) in place; Lambda (B,N,F,T), g (B,N,F,M)."""
        B, M, F, T = self._dims(X)
        N = int(Lambda.shape[1])
        ws = self._scratch(B, M, F, T, 1)
        scratch = self.empty((B, M, F, T))
        self._check(self._L.assx_fastmnmf_update_diagonalizer(self.ctx, ptr(X), ptr(Q), ptr(Lambda), ptr(g), float(eps),
                                                              float(threshold), ptr(scratch), ptr(status), ptr(ws), B, M,
                                                              N, F, T, self.prec.code, self._st()),
                    "assx_fastmnmf_update_diagonalizer")
        return Q

    # ------------------------------------------------------------------ the seven factorisation model families
    # Every array and workspace goes through check_array / check_workspace (top of this module) before its address does
    # through ptr().  A `_X_dims` holds only what is its family's own: how the sizes are read off the arrays, the range
    # limits, the arrays wanted as (name, array, shape, dtype), the workspace query.
    def _arg(self, model, name, a, dtype, shape=None, numel=None):
        """check_array on this engine's device; an optional array left None passes."""
        if a is not None:
            check_array(model, name, a, dtype, self.dev, shape, numel)

    def _args(self, model, want):
        dev = self.dev
        for name, a, shape, dtype in want:
            if a is not None:
                check_array(model, name, a, dtype, dev, shape)

    def _new_workspace(self, nbytes, supports, *got):
        """A model's own scratch of `nbytes`; 0 is the library's word for sizes outside the model's envelope."""
        if nbytes == 0:
            raise ValueError(supports % got)
        return torch.empty(int(nbytes), dtype=torch.uint8, device=self.dev)

    # ------------------------------------------------------------------ FastMNMF (bss/mnmf.py)
    def _fastmnmf_dims(self, X, W, H, g, Q=None, ws=None):
        if X.dim() != 4 or W.dim() != 4:
            raise ValueError("FastMNMF: expected X (B,M,F,T) and basis (B,N,F,K), got %s and %s"
                             % (tuple(X.shape), tuple(W.shape)))
        B, M, F, T = (int(d) for d in X.shape)
        N, K = int(W.shape[1]), int(W.shape[3])
        real, cplx = self.prec.real, self.prec.cplx
        self._args("FastMNMF", (("basis", W, (B, N, F, K), real), ("activation", H, (B, N, K, T), real),
                                ("spatial_covariance", g, (B, N, F, M), real), ("diagonalizer", Q, (B, F, M, M), cplx),
                                ("input", X, (B, M, F, T), cplx)))
        if ws is not None:
            check_workspace("FastMNMF", ws, self.dev,
                            self._L.assx_fastmnmf_workspace_bytes(B, M, N, F, T, K, self.prec.code))
        return B, M, N, F, T, K

    def fastmnmf_workspace(self, B, M, N, F, T, K):
        """A model's own scratch: it carries x~ from assx_fastmnmf_project to the NMF and SCM updates."""
        return self._new_workspace(self._L.assx_fastmnmf_workspace_bytes(B, M, N, F, T, K, self.prec.code),
                                   "FastMNMF supports 2 <= n_channels <= 8, 1 <= n_sources <= 8, 1 <= n_basis <= 64; got "
                                   "n_channels=%d, n_sources=%d, n_basis=%d", M, N, K)

    def fastmnmf_project(self, X, Q, W, H, g, ws, eps=1e-12, loss=None):
        """x~ = |Q x|^2 into ws; loss (B,) float64 (or None) = the negative log-likelihood of the model as it stands."""
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, Q, ws)
        self._arg("FastMNMF", "loss", loss, torch.float64, numel=B)
        self._check(self._L.assx_fastmnmf_project(self.ctx, ptr(X), ptr(Q), ptr(W), ptr(H), ptr(g), float(eps), ptr(loss),
                                                  ptr(ws), B, M, N, F, T, K, self.prec.code, self._st()),
                    "assx_fastmnmf_project")
        return loss

    def fastmnmf_update_nmf(self, X, W, H, g, ws, eps=1e-12):
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, None, ws)
        self._check(self._L.assx_fastmnmf_update_nmf(self.ctx, ptr(W), ptr(H), ptr(g), float(eps), ptr(ws), B, M, N, F, T,
                                                     K, self.prec.code, self._st()), "assx_fastmnmf_update_nmf")

    def fastmnmf_update_scm(self, X, W, H, g, ws, eps=1e-12):
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, None, ws)
        self._check(self._L.assx_fastmnmf_update_scm(self.ctx, ptr(W), ptr(H), ptr(g), float(eps), ptr(ws), B, M, N, F, T,
                                                     K, self.prec.code, self._st()), "assx_fastmnmf_update_scm")

    def fastmnmf_update_diagonalizer_model(self, X, Q, W, H, g, ws, eps=1e-12, threshold=1e12, status=None):
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, Q, ws)
        self._arg("FastMNMF", "status", status, torch.int32, numel=B)
        self._check(self._L.assx_fastmnmf_update_diagonalizer_model(self.ctx, ptr(X), ptr(Q), ptr(W), ptr(H), ptr(g),
                                                                    float(eps), float(threshold), ptr(status), ptr(ws), B,
                                                                    M, N, F, T, K, self.prec.code, self._st()),
                    "assx_fastmnmf_update_diagonalizer_model")

    def fastmnmf_normalize_power(self, X, Q, W, H, g, eps=1e-12):
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, Q)
        self._check(self._L.assx_fastmnmf_normalize_power(self.ctx, ptr(Q), ptr(W), ptr(H), ptr(g), float(eps), B, M, N, F,
                                                          T, K, self.prec.code, self._st()),
                    "assx_fastmnmf_normalize_power")

    def fastmnmf_separate(self, X, Q, W, H, g, ref=0, eps=1e-12, status=None, out=None):
        """(B,N,F,T) complex: x_hat[:, ref] of the reference's separate."""
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, Q)
        self._arg("FastMNMF", "status", status, torch.int32, numel=B)
        Y = out if out is not None else self.empty((B, N, F, T), complex_=True)
        self._arg("FastMNMF", "out", Y, self.prec.cplx, numel=B * N * F * T)
        self._check(self._L.assx_fastmnmf_separate(self.ctx, ptr(X), ptr(Q), ptr(W), ptr(H), ptr(g), int(ref), float(eps),
                                                   ptr(Y), ptr(status), B, M, N, F, T, K, self.prec.code, self._st()),
                    "assx_fastmnmf_separate")
        return Y

    def fastmnmf_iterate(self, n_iter, X, Q, W, H, g, ws, normalize=True, eps=1e-12, threshold=1e12, status=None,
                         loss=None):
        """loss: (n_iter + 1, B) float64 or None."""
        B, M, N, F, T, K = self._fastmnmf_dims(X, W, H, g, Q, ws)
        self._arg("FastMNMF", "loss", loss, torch.float64, numel=(int(n_iter) + 1) * B)
        self._arg("FastMNMF", "status", status, torch.int32, numel=B)
        self._check(self._L.assx_fastmnmf_iterate(self.ctx, int(n_iter), 1 if normalize else 0, ptr(X), ptr(Q), ptr(W),
                                                  ptr(H), ptr(g), float(eps), float(threshold), ptr(loss), ptr(status),
                                                  ptr(ws), B, M, N, F, T, K, self.prec.code, self._st()),
                    "assx_fastmnmf_iterate")

    # ------------------------------------------------------------------ MultichannelISNMF (bss/mnmf.py)
    def _mnmf_dims(self, X, Tb, V, Z, H, ws=None):
        if X.dim() != 4 or Z.dim() != 3:
            raise ValueError("MNMF: expected X (B,M,F,T) and latent (B,N,K), got %s and %s"
                             % (tuple(X.shape), tuple(Z.shape)))
        B, M, F, T = (int(d) for d in X.shape)
        N, K = int(Z.shape[1]), int(Z.shape[2])
        self._args("MNMF", (("input", X, (B, M, F, T), torch.complex128), ("basis", Tb, (B, F, K), torch.float64),
                            ("activation", V, (B, K, T), torch.float64), ("latent", Z, (B, N, K), torch.float64),
                            ("spatial", H, (B, F, N, M, M), torch.complex128)))
        if ws is not None:
            check_workspace("MNMF", ws, self.dev, self._L.assx_mnmf_workspace_bytes(B, M, N, F, T, K, _lib.F64))
        return B, M, N, F, T, K

    def mnmf_workspace(self, B, M, N, F, T, K):
        return self._new_workspace(self._L.assx_mnmf_workspace_bytes(B, M, N, F, T, K, _lib.F64),
                                   "MNMF supports float64, 2 <= n_channels <= 8, 1 <= n_sources <= 8, 1 <= n_basis <= 64; "
                                   "got n_channels=%d, n_sources=%d, n_basis=%d", M, N, K)

    def _mnmf_step(self, what, X, Tb, V, Z, H, ws, eps, status):
        B, M, N, F, T, K = self._mnmf_dims(X, Tb, V, Z, H, ws)
        self._arg("MNMF", "status", status, torch.int32, numel=B)
        self._check(getattr(self._L, what)(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(Z), ptr(H), float(eps), ptr(status),
                                           ptr(ws), B, M, N, F, T, K, _lib.F64, self._st()), what)

    def mnmf_update_basis(self, X, Tb, V, Z, H, ws, eps=1e-12, status=None):
        self._mnmf_step("assx_mnmf_update_basis", X, Tb, V, Z, H, ws, eps, status)

    def mnmf_update_activation(self, X, Tb, V, Z, H, ws, eps=1e-12, status=None):
        self._mnmf_step("assx_mnmf_update_activation", X, Tb, V, Z, H, ws, eps, status)

    def mnmf_update_latent(self, X, Tb, V, Z, H, ws, eps=1e-12, status=None):
        self._mnmf_step("assx_mnmf_update_latent", X, Tb, V, Z, H, ws, eps, status)

    def mnmf_update_spatial(self, X, Tb, V, Z, H, ws, normalize=True, eps=1e-12, status=None):
        B, M, N, F, T, K = self._mnmf_dims(X, Tb, V, Z, H, ws)
        self._arg("MNMF", "status", status, torch.int32, numel=B)
        self._check(self._L.assx_mnmf_update_spatial(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(Z), ptr(H),
                                                     1 if normalize else 0, float(eps), ptr(status), ptr(ws), B, M, N,
                                                     F, T, K, _lib.F64, self._st()), "assx_mnmf_update_spatial")

    def mnmf_loss(self, X, Tb, V, Z, H, ws, eps=1e-12, status=None, loss=None):
        """loss (B,) float64: the negative log-likelihood of the model as it stands."""
        B, M, N, F, T, K = self._mnmf_dims(X, Tb, V, Z, H, ws)
        self._arg("MNMF", "status", status, torch.int32, numel=B)
        loss = loss if loss is not None else self.empty((B,), dtype=torch.float64)
        self._arg("MNMF", "loss", loss, torch.float64, numel=B)
        self._check(self._L.assx_mnmf_loss(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(Z), ptr(H), float(eps), ptr(loss),
                                           ptr(status), ptr(ws), B, M, N, F, T, K, _lib.F64, self._st()),
                    "assx_mnmf_loss")
        return loss

    def mnmf_separate(self, X, Tb, V, Z, H, ref=0, eps=1e-12, status=None, out=None):
        """(B,N,F,T) complex: lam_n (H_n P x)[ref]."""
        B, M, N, F, T, K = self._mnmf_dims(X, Tb, V, Z, H)
        self._arg("MNMF", "status", status, torch.int32, numel=B)
        Y = out if out is not None else self.empty((B, N, F, T), dtype=torch.complex128)
        self._arg("MNMF", "out", Y, torch.complex128, numel=B * N * F * T)
        self._check(self._L.assx_mnmf_separate(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(Z), ptr(H), int(ref), float(eps),
                                               ptr(Y), ptr(status), B, M, N, F, T, K, _lib.F64, self._st()),
                    "assx_mnmf_separate")
        return Y

    def mnmf_iterate(self, n_iter, X, Tb, V, Z, H, ws, normalize=True, eps=1e-12, status=None, loss=None):
        """loss: (n_iter + 1, B) float64 or None."""
        B, M, N, F, T, K = self._mnmf_dims(X, Tb, V, Z, H, ws)
        self._arg("MNMF", "loss", loss, torch.float64, numel=(int(n_iter) + 1) * B)
        self._arg("MNMF", "status", status, torch.int32, numel=B)
        self._check(self._L.assx_mnmf_iterate(self.ctx, int(n_iter), 1 if normalize else 0, ptr(X), ptr(Tb), ptr(V),
                                              ptr(Z), ptr(H), float(eps), ptr(loss), ptr(status), ptr(ws), B, M, N, F,
                                              T, K, _lib.F64, self._st()), "assx_mnmf_iterate")

    # ------------------------------------------------------------------ ComplexEUCNMF (algorithm/nmf.py)
    def _cnmf_dims(self, Tb, V, Phi=None, X=None, ws=None):
        if self.prec.code != _lib.F64:
            raise ValueError("ComplexEUCNMF supports float64 only")
        if Tb.dim() != 3 or V.dim() != 3:
            raise ValueError("ComplexEUCNMF: expected basis (B,F,K) and activation (B,K,T), got %s and %s"
                             % (tuple(Tb.shape), tuple(V.shape)))
        B, F, K = (int(d) for d in Tb.shape)
        T = int(V.shape[2])
        if not 1 <= K <= 64:
            raise ValueError("ComplexEUCNMF: n_basis must be in [1, 64], got %d" % K)
        self._args("ComplexEUCNMF", (("basis", Tb, (B, F, K), torch.float64), ("activation", V, (B, K, T), torch.float64),
                                     ("phase", Phi, (B, F, K, T), torch.float64),
                                     ("target", X, (B, F, T), torch.complex128)))
        if ws is not None:
            check_workspace("ComplexEUCNMF", ws, self.dev, self._L.assx_cnmf_workspace_bytes(B, F, T, K, _lib.F64))
        return B, F, T, K

    def cnmf_workspace(self, B, F, T, K):
        return self._new_workspace(self._L.assx_cnmf_workspace_bytes(B, F, T, K, self.prec.code),
                                   "ComplexEUCNMF supports float64 and 1 <= n_basis <= 64; got dtype=%s, n_basis=%d",
                                   self.prec.name, K)

    def cnmf_update(self, X, Tb, V, Phi, ws, regularizer=0.1, p=1, eps=1e-12):
        B, F, T, K = self._cnmf_dims(Tb, V, Phi, X, ws)
        self._check(self._L.assx_cnmf_update(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(Phi), float(regularizer), float(p),
                                             float(eps), ptr(ws), B, F, T, K, _lib.F64, self._st()), "assx_cnmf_update")

    def cnmf_loss(self, X, Tb, V, Phi, ws, eps=1e-12, loss=None):
        """loss (B,) float64: sum |sum_k T V e^{i Phi} - X|^2 of the model as it stands."""
        B, F, T, K = self._cnmf_dims(Tb, V, Phi, X, ws)
        loss = loss if loss is not None else self.empty((B,), dtype=torch.float64)
        self._arg("ComplexEUCNMF", "loss", loss, torch.float64, numel=B)
        self._check(self._L.assx_cnmf_loss(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(Phi), float(eps), ptr(loss), ptr(ws), B,
                                           F, T, K, _lib.F64, self._st()), "assx_cnmf_loss")
        return loss

    def cnmf_beta(self, Tb, V, eps=1e-12, out=None):
        """(B,F,K,T): T V / max(sum_k T V, eps)."""
        B, F, T, K = self._cnmf_dims(Tb, V)
        Beta = out if out is not None else self.empty((B, F, K, T), dtype=torch.float64)
        self._arg("ComplexEUCNMF", "out", Beta, torch.float64, numel=B * F * K * T)
        self._check(self._L.assx_cnmf_beta(self.ctx, ptr(Tb), ptr(V), float(eps), ptr(Beta), B, F, T, K, _lib.F64,
                                           self._st()), "assx_cnmf_beta")
        return Beta

    def cnmf_reconstruct(self, Tb, V, Phi, out=None):
        """(B,F,T) complex: sum_k T V e^{i Phi}."""
        B, F, T, K = self._cnmf_dims(Tb, V, Phi)
        Y = out if out is not None else self.empty((B, F, T), dtype=torch.complex128)
        self._arg("ComplexEUCNMF", "out", Y, torch.complex128, numel=B * F * T)
        self._check(self._L.assx_cnmf_reconstruct(self.ctx, ptr(Tb), ptr(V), ptr(Phi), ptr(Y), B, F, T, K, _lib.F64,
                                                  self._st()), "assx_cnmf_reconstruct")
        return Y

    def cnmf_iterate(self, n_iter, X, Tb, V, Phi, ws, regularizer=0.1, p=1, eps=1e-12, loss=None):
        """n_iter x update; loss: (n_iter, B) float64 or None."""
        B, F, T, K = self._cnmf_dims(Tb, V, Phi, X, ws)
        self._arg("ComplexEUCNMF", "loss", loss, torch.float64, numel=int(n_iter) * B)
        self._check(self._L.assx_cnmf_iterate(self.ctx, int(n_iter), ptr(X), ptr(Tb), ptr(V), ptr(Phi),
                                              float(regularizer), float(p), float(eps), ptr(loss), ptr(ws), B, F, T, K,
                                              _lib.F64, self._st()), "assx_cnmf_iterate")

    # ------------------------------------------------------------------ EUCNTF (algorithm/ntf.py)
    def _ntf_dims(self, Z, Tb, V, X=None, ws=None):
        if self.prec.code != _lib.F64:
            raise ValueError("EUCNTF supports float64 only")
        if Z.dim() != 3 or Tb.dim() != 3 or V.dim() != 3:
            raise ValueError("EUCNTF: expected partitioning (B,N,K), basis (B,I,K) and activation (B,K,J), got %s, %s "
                             "and %s" % (tuple(Z.shape), tuple(Tb.shape), tuple(V.shape)))
        B, N, K = (int(d) for d in Z.shape)
        I, J = int(Tb.shape[1]), int(V.shape[2])
        if not 1 <= K <= 64:
            raise ValueError("EUCNTF: n_basis must be in [1, 64], got %d" % K)
        if not 1 <= N <= 32:
            raise ValueError("EUCNTF: n_channels must be in [1, 32], got %d" % N)
        self._args("EUCNTF", (("partitioning", Z, (B, N, K), torch.float64), ("basis", Tb, (B, I, K), torch.float64),
                              ("activation", V, (B, K, J), torch.float64), ("target", X, (B, N, I, J), torch.float64)))
        if ws is not None:
            check_workspace("EUCNTF", ws, self.dev, self._L.assx_ntf_workspace_bytes(B, N, I, J, K, _lib.F64))
        return B, N, I, J, K

    def ntf_workspace(self, B, N, I, J, K):
        return self._new_workspace(self._L.assx_ntf_workspace_bytes(B, N, I, J, K, self.prec.code),
                                   "EUCNTF supports float64, 1 <= n_basis <= 64 and 1 <= n_channels <= 32; got dtype=%s, "
                                   "n_basis=%d, n_channels=%d", self.prec.name, K, N)

    def ntf_update(self, X, Z, Tb, V, ws, eps=1e-12):
        """One update_once of (Z, Tb, V), in place."""
        B, N, I, J, K = self._ntf_dims(Z, Tb, V, X, ws)
        self._check(self._L.assx_ntf_update(self.ctx, ptr(X), ptr(Z), ptr(Tb), ptr(V), float(eps), ptr(ws), B, N, I, J, K,
                                            _lib.F64, self._st()), "assx_ntf_update")

    def ntf_loss(self, X, Z, Tb, V, ws, loss=None):
        """loss (B,) float64: sum (X - sum_k Z T V)^2 of the model as it stands."""
        B, N, I, J, K = self._ntf_dims(Z, Tb, V, X, ws)
        loss = loss if loss is not None else self.empty((B,), dtype=torch.float64)
        self._arg("EUCNTF", "loss", loss, torch.float64, (B,))
        self._check(self._L.assx_ntf_loss(self.ctx, ptr(X), ptr(Z), ptr(Tb), ptr(V), ptr(loss), ptr(ws), B, N, I, J, K,
                                          _lib.F64, self._st()), "assx_ntf_loss")
        return loss

    def ntf_reconstruct(self, Z, Tb, V, out=None):
        """(B,N,I,J): sum_k Z T V."""
        B, N, I, J, K = self._ntf_dims(Z, Tb, V)
        Xh = out if out is not None else self.empty((B, N, I, J), dtype=torch.float64)
        self._arg("EUCNTF", "out", Xh, torch.float64, (B, N, I, J))
        self._check(self._L.assx_ntf_reconstruct(self.ctx, ptr(Z), ptr(Tb), ptr(V), ptr(Xh), B, N, I, J, K, _lib.F64,
                                                 self._st()), "assx_ntf_reconstruct")
        return Xh

    def ntf_iterate(self, n_iter, X, Z, Tb, V, ws, eps=1e-12, loss=None):
        """n_iter x update; loss: (n_iter, B) float64 or None."""
        B, N, I, J, K = self._ntf_dims(Z, Tb, V, X, ws)
        if int(n_iter) < 0:
            raise ValueError("EUCNTF: n_iter must be >= 0, got %d" % int(n_iter))
        self._arg("EUCNTF", "loss", loss, torch.float64, (int(n_iter), B))
        self._check(self._L.assx_ntf_iterate(self.ctx, int(n_iter), ptr(X), ptr(Z), ptr(Tb), ptr(V), float(eps),
                                             ptr(loss), ptr(ws), B, N, I, J, K, _lib.F64, self._st()), "assx_ntf_iterate")

    # ------------------------------------------------------------------ LDPSDTF (algorithm/psdtf.py)
    def _psdtf_dims(self, V, H, X=None, ws=None, status=None):
        if self.prec.code != _lib.F64:
            raise ValueError("LDPSDTF supports float64 only")
        if V.dim() != 4 or H.dim() != 3 or V.shape[2] != V.shape[3]:
            raise ValueError("LDPSDTF: expected basis (B,K,M,M) and activation (B,K,T), got %s and %s"
                             % (tuple(V.shape), tuple(H.shape)))
        B, K, M = (int(d) for d in V.shape[:3])
        T = int(H.shape[2])
        if not 1 <= K <= 64:
            raise ValueError("LDPSDTF: n_basis must be in [1, 64], got %d" % K)
        if not 1 <= M <= 64:
            raise ValueError("LDPSDTF: n_bins must be in [1, 64], got %d" % M)
        if B < 1 or T < 1:
            raise ValueError("LDPSDTF: empty problem B=%d T=%d" % (B, T))
        self._args("LDPSDTF", (("basis", V, (B, K, M, M), torch.float64), ("activation", H, (B, K, T), torch.float64),
                               ("target", X, (B, T, M, M), torch.float64)))
        if ws is not None:
            check_workspace("LDPSDTF", ws, self.dev, self._L.assx_psdtf_workspace_bytes(B, M, T, K, _lib.F64))
        self._arg("LDPSDTF", "status", status, torch.int32, (B,))
        return B, M, T, K

    def psdtf_workspace(self, B, M, T, K):
        return self._new_workspace(self._L.assx_psdtf_workspace_bytes(B, M, T, K, self.prec.code),
                                   "LDPSDTF supports float64, 1 <= n_bins <= 64 and 1 <= n_basis <= 64; got dtype=%s, "
                                   "n_bins=%d, n_basis=%d", self.prec.name, M, K)

    def psdtf_to_psd(self, A, eps=1e-12):
        """to_PSD of (n, M, M) symmetric matrices, in place."""
        if A.dim() != 3 or A.shape[1] != A.shape[2] or not 1 <= int(A.shape[1]) <= 64 or int(A.shape[0]) < 1:
            raise ValueError("psdtf_to_psd: expected (n, M, M) with 1 <= M <= 64, got %s" % (tuple(A.shape),))
        self._arg("LDPSDTF", "A", A, torch.float64, A.shape)
        self._check(self._L.assx_psdtf_to_psd(self.ctx, ptr(A), int(A.shape[0]), int(A.shape[1]), float(eps), self._st()),
                    "assx_psdtf_to_psd")
        return A

    def psdtf_update_basis(self, X, V, H, ws, eps=1e-12, status=None):
        B, M, T, K = self._psdtf_dims(V, H, X, ws, status)
        self._check(self._L.assx_psdtf_update_basis(self.ctx, ptr(X), ptr(V), ptr(H), float(eps), ptr(status), ptr(ws), B, M,
                                                    T, K, _lib.F64, self._st()), "assx_psdtf_update_basis")

    def psdtf_update_activation(self, X, V, H, eps=1e-12, status=None):
        B, M, T, K = self._psdtf_dims(V, H, X, None, status)
        self._check(self._L.assx_psdtf_update_activation(self.ctx, ptr(X), ptr(V), ptr(H), float(eps), ptr(status), B, M, T,
                                                         K, _lib.F64, self._st()), "assx_psdtf_update_activation")

    def psdtf_normalize(self, V, H):
        B, M, T, K = self._psdtf_dims(V, H)
        self._check(self._L.assx_psdtf_normalize(self.ctx, ptr(V), ptr(H), B, M, T, K, _lib.F64, self._st()),
                    "assx_psdtf_normalize")

    def psdtf_update(self, X, V, H, ws, eps=1e-12, normalize=True, status=None):
        """One update_once of (V, H), in place."""
        B, M, T, K = self._psdtf_dims(V, H, X, ws, status)
        self._check(self._L.assx_psdtf_update(self.ctx, ptr(X), ptr(V), ptr(H), float(eps), int(bool(normalize)),
                                              ptr(status), ptr(ws), B, M, T, K, _lib.F64, self._st()), "assx_psdtf_update")

    def psdtf_loss(self, X, V, H, ws, eps=1e-12, loss=None, status=None):
        """loss (B,) float64: the log-det divergence of the model as it stands, summed over the frames."""
        B, M, T, K = self._psdtf_dims(V, H, X, ws, status)
        loss = loss if loss is not None else self.empty((B,), dtype=torch.float64)
        self._arg("LDPSDTF", "loss", loss, torch.float64, (B,))
        self._check(self._L.assx_psdtf_loss(self.ctx, ptr(X), ptr(V), ptr(H), float(eps), ptr(loss), ptr(status), ptr(ws), B,
                                            M, T, K, _lib.F64, self._st()), "assx_psdtf_loss")
        return loss

    def psdtf_reconstruct(self, V, H, out=None):
        """(B,T,M,M): sum_k H V_k."""
        B, M, T, K = self._psdtf_dims(V, H)
        Xh = out if out is not None else self.empty((B, T, M, M), dtype=torch.float64)
        self._arg("LDPSDTF", "out", Xh, torch.float64, (B, T, M, M))
        self._check(self._L.assx_psdtf_reconstruct(self.ctx, ptr(V), ptr(H), ptr(Xh), B, M, T, K, _lib.F64, self._st()),
                    "assx_psdtf_reconstruct")
        return Xh

    def psdtf_iterate(self, n_iter, X, V, H, ws, eps=1e-12, normalize=True, loss=None, status=None):
        """n_iter x (update, loss); loss: (n_iter, B) float64 or None."""
        B, M, T, K = self._psdtf_dims(V, H, X, ws, status)
        if int(n_iter) < 0:
            raise ValueError("LDPSDTF: n_iter must be >= 0, got %d" % int(n_iter))
        self._arg("LDPSDTF", "loss", loss, torch.float64, (int(n_iter), B))
        self._check(self._L.assx_psdtf_iterate(self.ctx, int(n_iter), ptr(X), ptr(V), ptr(H), float(eps),
                                               int(bool(normalize)), ptr(loss), ptr(status), ptr(ws), B, M, T, K, _lib.F64,
                                               self._st()), "assx_psdtf_iterate")

    # ------------------------------------------------------------------ GaussIPSDTA (include/assx.h (f10))
    _IPSDTA_SUPPORTS = ("%s supports float64, 2 <= n_channels <= 8, 1 <= n_basis <= 64, 1 <= n_blocks <= n_bins "
                        "and blocks of at most 8 bins; got dtype=%s, n_channels=%d, n_bins=%d, n_frames=%d, n_basis=%d, "
                        "n_blocks=%d")

    @staticmethod
    def ipsdta_packed_size(F, n_blocks):
        """P: the entries of one packed basis (the nb x nb blocks end to end)."""
        nn, rem = F // n_blocks, F % n_blocks
        return (n_blocks - rem) * nn * nn + rem * (nn + 1) * (nn + 1)

    def _ipsdta_dims(self, n_blocks, U, H, X=None, W=None, ws=None, status=None, nu=None):
        """nu: None for (f10), the degree of freedom for (f11), whose workspace is then the one checked."""
        model = "GaussIPSDTA" if nu is None else "tIPSDTA"
        if U.dim() != 3 or H.dim() != 3:
            raise ValueError("%s: packed basis (N, K, P) and activation (N, K, T) expected, got %s and %s"
                             % (model, tuple(U.shape), tuple(H.shape)))
        M, K, T = (int(d) for d in H.shape)
        if X is not None:
            F = int(X.shape[1])
        elif W is not None:
            F = int(W.shape[0])
        else:
            raise ValueError("%s: the number of bins is unknown without X or W" % model)
        n_blocks = int(n_blocks)
        need = self._L.assx_ipsdta_workspace_bytes(M, F, T, K, n_blocks, self.prec.code)
        if need == 0:
            raise ValueError(self._IPSDTA_SUPPORTS % (model, self.prec.name, M, F, T, K, n_blocks))
        self._args(model, (("basis", U, (M, K, self.ipsdta_packed_size(F, n_blocks)), torch.complex128),
                           ("activation", H, (M, K, T), torch.float64), ("input", X, (M, F, T), torch.complex128),
                           ("demix_filter", W, (F, M, M), torch.complex128), ("status", status, (1,), torch.int32)))
        if nu is not None:
            nu = float(nu)
            if not 0.0 < nu < float("inf"):
                raise ValueError("tIPSDTA: nu must be finite and > 0, got %r" % (nu,))
            need = self._L.assx_tipsdta_workspace_bytes(M, F, T, K, n_blocks, self.prec.code, nu)
        if ws is not None:
            check_workspace(model, ws, self.dev, need)
        return M, F, T, K, n_blocks

    def _ipsdta_call(self, entry, nu, X, W, U, H, ws, n_blocks, eps, status, lead=(), mid=(), counts=None, loss=None):
        """The dims check and the call of assx_ipsdta_<entry> (nu None) or assx_tipsdta_<entry>: `lead` goes before X, nu
        after eps, `mid` after nu.  counts: (message, values) of the arguments that must be >= 0; loss: (array or None,
        shape) where the entry takes a loss, whose pointer then follows `mid`."""
        model, name = ("GaussIPSDTA", "assx_ipsdta_" + entry) if nu is None else ("tIPSDTA", "assx_tipsdta_" + entry)
        M, F, T, K, nb = self._ipsdta_dims(n_blocks, U, H, X, W, ws, status, nu)
        if counts is not None and min(counts[1]) < 0:
            raise ValueError("%s: %s must be >= 0, got %s" % (model, counts[0], " and ".join("%d" % v for v in counts[1])))
        if loss is not None:
            self._arg(model, "loss", loss[0], torch.float64, loss[1])
            mid = tuple(mid) + (ptr(loss[0]),)
        args = tuple(lead) + (ptr(X), ptr(W), ptr(U), ptr(H), float(eps)) + (() if nu is None else (float(nu),)) + tuple(mid)
        self._check(getattr(self._L, name)(self.ctx, *args, ptr(status), ptr(ws), M, F, T, K, nb, _lib.F64, self._st()), name)

    def _ipsdta_loss(self, nu, X, W, U, H, ws, n_blocks, eps, loss, status):
        loss = loss if loss is not None else self.empty((1,), dtype=torch.float64)
        self._ipsdta_call("loss", nu, X, W, U, H, ws, n_blocks, eps, status, loss=(loss, (1,)))
        return loss

    def _ipsdta_iterate(self, nu, n_iter, spatial_iteration, X, W, U, H, ws, n_blocks, eps, normalize, loss, status):
        n_iter, sp = int(n_iter), int(spatial_iteration)
        self._ipsdta_call("iterate", nu, X, W, U, H, ws, n_blocks, eps, status, lead=(n_iter, sp),
                          mid=(int(bool(normalize)),), counts=("n_iter and spatial_iteration", (n_iter, sp)),
                          loss=(loss, (n_iter,)))

    def ipsdta_workspace(self, M, F, T, K, n_blocks):
        return self._new_workspace(self._L.assx_ipsdta_workspace_bytes(int(M), int(F), int(T), int(K), int(n_blocks),
                                                                       self.prec.code),
                                   self._IPSDTA_SUPPORTS, "GaussIPSDTA", self.prec.name, M, F, T, K, n_blocks)

    def ipsdta_to_psd(self, A, eps=1e-12):
        """to_PSD of (n, nb, nb) Hermitian matrices, in place."""
        if A.dim() != 3 or A.shape[1] != A.shape[2] or not 1 <= int(A.shape[1]) <= 8 or int(A.shape[0]) < 1:
            raise ValueError("ipsdta_to_psd: expected (n, nb, nb) with 1 <= nb <= 8, got %s" % (tuple(A.shape),))
        self._arg("GaussIPSDTA", "A", A, torch.complex128, A.shape)
        self._check(self._L.assx_ipsdta_to_psd(self.ctx, ptr(A), int(A.shape[0]), int(A.shape[1]), float(eps), self._st()),
                    "assx_ipsdta_to_psd")
        return A

    def ipsdta_update_basis(self, X, W, U, H, ws, n_blocks, eps=1e-12, status=None):
        self._ipsdta_call("update_basis", None, X, W, U, H, ws, n_blocks, eps, status)

    def ipsdta_update_activation(self, X, W, U, H, ws, n_blocks, eps=1e-12, status=None):
        self._ipsdta_call("update_activation", None, X, W, U, H, ws, n_blocks, eps, status)

    def ipsdta_normalize(self, U, H, n_bins, n_blocks):
        if U.dim() != 3 or H.dim() != 3:
            raise ValueError("GaussIPSDTA: packed basis (N, K, P) and activation (N, K, T) expected, got %s and %s"
                             % (tuple(U.shape), tuple(H.shape)))
        M, K, T = (int(d) for d in H.shape)
        F, nb = int(n_bins), int(n_blocks)
        if self._L.assx_ipsdta_workspace_bytes(M, F, T, K, nb, self.prec.code) == 0:
            raise ValueError("GaussIPSDTA: n_channels=%d n_bins=%d n_basis=%d n_blocks=%d outside the envelope" % (M, F, K, nb))
        self._args("GaussIPSDTA", (("basis", U, (M, K, self.ipsdta_packed_size(F, nb)), torch.complex128),
                                   ("activation", H, (M, K, T), torch.float64)))
        self._check(self._L.assx_ipsdta_normalize(self.ctx, ptr(U), ptr(H), M, F, T, K, nb, _lib.F64, self._st()),
                    "assx_ipsdta_normalize")

    def ipsdta_update_source(self, X, W, U, H, ws, n_blocks, eps=1e-12, normalize=True, status=None):
        self._ipsdta_call("update_source", None, X, W, U, H, ws, n_blocks, eps, status, mid=(int(bool(normalize)),))

    def ipsdta_update_spatial(self, X, W, U, H, ws, n_blocks, n_sweeps=1, eps=1e-12, status=None):
        self._ipsdta_call("update_spatial", None, X, W, U, H, ws, n_blocks, eps, status, lead=(int(n_sweeps),),
                          counts=("n_sweeps", (int(n_sweeps),)))

    def ipsdta_loss(self, X, W, U, H, ws, n_blocks, eps=1e-12, loss=None, status=None):
        """loss (1,) float64: the negative log-likelihood of the model as it stands."""
        return self._ipsdta_loss(None, X, W, U, H, ws, n_blocks, eps, loss, status)

    def ipsdta_iterate(self, n_iter, spatial_iteration, X, W, U, H, ws, n_blocks, eps=1e-12, normalize=True, loss=None,
                       status=None):
        """n_iter x (source update, `spatial_iteration` sweeps, loss); loss: (n_iter,) float64 or None."""
        self._ipsdta_iterate(None, n_iter, spatial_iteration, X, W, U, H, ws, n_blocks, eps, normalize, loss, status)

    # ------------------------------------------------------------------ tIPSDTA (include/assx.h (f11))
    def tipsdta_workspace(self, M, F, T, K, n_blocks, nu=1.0):
        return self._new_workspace(self._L.assx_tipsdta_workspace_bytes(int(M), int(F), int(T), int(K), int(n_blocks),
                                                                        self.prec.code, float(nu)),
                                   "tIPSDTA supports float64, 2 <= n_channels <= 8, 1 <= n_basis <= 64, 1 <= n_blocks <= "
                                   "n_bins, blocks of at most 8 bins and a finite nu > 0; got dtype=%s, n_channels=%d, "
                                   "n_bins=%d, n_frames=%d, n_basis=%d, n_blocks=%d, nu=%r",
                                   self.prec.name, M, F, T, K, n_blocks, nu)

    def tipsdta_update_basis(self, X, W, U, H, ws, n_blocks, nu=1.0, eps=1e-12, status=None):
        self._ipsdta_call("update_basis", nu, X, W, U, H, ws, n_blocks, eps, status)

    def tipsdta_update_activation(self, X, W, U, H, ws, n_blocks, nu=1.0, eps=1e-12, status=None):
        self._ipsdta_call("update_activation", nu, X, W, U, H, ws, n_blocks, eps, status)

    def tipsdta_update_source(self, X, W, U, H, ws, n_blocks, nu=1.0, eps=1e-12, normalize=True, status=None):
        self._ipsdta_call("update_source", nu, X, W, U, H, ws, n_blocks, eps, status, mid=(int(bool(normalize)),))

    def tipsdta_update_spatial(self, X, W, U, H, ws, n_blocks, nu=1.0, n_sweeps=1, eps=1e-12, status=None):
        self._ipsdta_call("update_spatial", nu, X, W, U, H, ws, n_blocks, eps, status, lead=(int(n_sweeps),),
                          counts=("n_sweeps", (int(n_sweeps),)))

    def tipsdta_loss(self, X, W, U, H, ws, n_blocks, nu=1.0, eps=1e-12, loss=None, status=None):
        """loss (1,) float64: the negative log-likelihood of the model as it stands."""
        return self._ipsdta_loss(nu, X, W, U, H, ws, n_blocks, eps, loss, status)

    def tipsdta_iterate(self, n_iter, spatial_iteration, X, W, U, H, ws, n_blocks, nu=1.0, eps=1e-12, normalize=True,
                        loss=None, status=None):
        """n_iter x (source update, `spatial_iteration` sweeps, loss); loss: (n_iter,) float64 or None."""
        self._ipsdta_iterate(nu, n_iter, spatial_iteration, X, W, U, H, ws, n_blocks, eps, normalize, loss, status)

    def hermitian_riccati(self, A, Bm, status=None):
        """H (n,M,M) complex128: the positive-definite solution of H A H = B for each of n pairs."""
        if A.dim() != 3 or tuple(Bm.shape) != tuple(A.shape) or A.shape[1] != A.shape[2]:
            raise ValueError("hermitian_riccati: A and B must be (n, M, M), got %s and %s"
                             % (tuple(A.shape), tuple(Bm.shape)))
        for a in (A, Bm):
            if a.dtype != torch.complex128 or a.device != self.dev or not a.is_contiguous():
                raise ValueError("hermitian_riccati: A and B must be contiguous complex128 on %s" % self.dev)
        n, M = int(A.shape[0]), int(A.shape[1])
        self._arg("hermitian_riccati", "status", status, torch.int32, numel=n)
        H = self.empty((n, M, M), dtype=torch.complex128)
        self._check(self._L.assx_hermitian_riccati(self.ctx, ptr(A), ptr(Bm), ptr(H), ptr(status), n, M, _lib.F64,
                                                   self._st()), "assx_hermitian_riccati")
        return H

    # ------------------------------------------------------------------ covariance-domain MultichannelISNMF (algorithm/nmf.py)
    def _covnmf_dims(self, Tb, V, H, X=None, ws=None, status=None):
        if Tb.dim() != 2 or V.dim() != 2 or H.dim() != 4:
            raise ValueError("CovNMF: expected basis (F,K), activation (K,T) and spatial (F,K,M,M), got %s, %s and %s"
                             % (tuple(Tb.shape), tuple(V.shape), tuple(H.shape)))
        F, K = (int(d) for d in Tb.shape)
        M, T = int(H.shape[-1]), int(V.shape[-1])
        self._args("CovNMF", (("target", X, (F, T, M, M), torch.complex128), ("basis", Tb, (F, K), torch.float64),
                              ("activation", V, (K, T), torch.float64), ("spatial", H, (F, K, M, M), torch.complex128)))
        self._arg("CovNMF", "status", status, torch.int32, numel=1)
        if ws is not None:
            check_workspace("CovNMF", ws, self.dev, self._L.assx_covnmf_workspace_bytes(M, F, T, K, _lib.F64))
        return M, F, T, K

    def covnmf_workspace(self, M, F, T, K):
        return self._new_workspace(self._L.assx_covnmf_workspace_bytes(M, F, T, K, _lib.F64),
                                   "CovNMF supports float64, 2 <= n_channels <= 8, 1 <= n_basis <= 64 and a target below "
                                   "4 GiB; got n_channels=%d, n_basis=%d, n_bins=%d, n_frames=%d", M, K, F, T)

    def _covnmf_step(self, what, X, Tb, V, H, ws, eps, status):
        M, F, T, K = self._covnmf_dims(Tb, V, H, X, ws, status)
        self._check(getattr(self._L, what)(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(H), float(eps), ptr(status), ptr(ws), M,
                                           F, T, K, _lib.F64, self._st()), what)

    def covnmf_update_basis(self, X, Tb, V, H, ws, eps=1e-12, status=None):
        self._covnmf_step("assx_covnmf_update_basis", X, Tb, V, H, ws, eps, status)

    def covnmf_update_activation(self, X, Tb, V, H, ws, eps=1e-12, status=None):
        self._covnmf_step("assx_covnmf_update_activation", X, Tb, V, H, ws, eps, status)

    def covnmf_update_spatial(self, X, Tb, V, H, ws, normalize=True, eps=1e-12, status=None):
        M, F, T, K = self._covnmf_dims(Tb, V, H, X, ws, status)
        self._check(self._L.assx_covnmf_update_spatial(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(H), 1 if normalize else 0,
                                                       float(eps), ptr(status), ptr(ws), M, F, T, K, _lib.F64,
                                                       self._st()), "assx_covnmf_update_spatial")

    def covnmf_reconstruct(self, Tb, V, H, out=None):
        """(F,T,M,M) complex128 = sum_k Tb V H_k."""
        M, F, T, K = self._covnmf_dims(Tb, V, H)
        Xh = out if out is not None else self.empty((F, T, M, M), dtype=torch.complex128)
        self._arg("CovNMF", "out", Xh, torch.complex128, shape=(F, T, M, M))
        self._check(self._L.assx_covnmf_reconstruct(self.ctx, ptr(Tb), ptr(V), ptr(H), ptr(Xh), M, F, T, K, _lib.F64,
                                                    self._st()), "assx_covnmf_reconstruct")
        return Xh

    def covnmf_loss(self, X, Tb, V, H, ws, eps=1e-12, loss=None, status=None):
        """loss (1,) float64: the multichannel Itakura-Saito divergence of the model as it stands."""
        M, F, T, K = self._covnmf_dims(Tb, V, H, X, ws, status)
        loss = loss if loss is not None else self.empty((1,), dtype=torch.float64)
        self._arg("CovNMF", "loss", loss, torch.float64, numel=1)
        self._check(self._L.assx_covnmf_loss(self.ctx, ptr(X), ptr(Tb), ptr(V), ptr(H), float(eps), ptr(loss), ptr(status),
                                             ptr(ws), M, F, T, K, _lib.F64, self._st()), "assx_covnmf_loss")
        return loss

    def covnmf_iterate(self, n_iter, X, Tb, V, H, ws, normalize=True, eps=1e-12, loss=None, status=None):
        """n_iter x (basis, activation, spatial, loss); loss: (n_iter,) float64 or None."""
        M, F, T, K = self._covnmf_dims(Tb, V, H, X, ws, status)
        self._arg("CovNMF", "loss", loss, torch.float64, numel=max(int(n_iter), 1))
        self._check(self._L.assx_covnmf_iterate(self.ctx, int(n_iter), 1 if normalize else 0, ptr(X), ptr(Tb), ptr(V),
                                                ptr(H), float(eps), ptr(loss), ptr(status), ptr(ws), M, F, T, K, _lib.F64,
                                                self._st()), "assx_covnmf_iterate")

    # ------------------------------------------------------------------ gradient IVA / FDICA (bss/iva.py, bss/fdica.py)
    def _gradbss_dims(self, X, W, ws=None, status=None):
        if X.dim() != 3 or W.dim() != 3:
            raise ValueError("GradBSS: expected input (M,F,T) and demix_filter (F,M,M), got %s and %s"
                             % (tuple(X.shape), tuple(W.shape)))
        M, F, T = (int(d) for d in X.shape)
        self._args("GradBSS", (("input", X, (M, F, T), torch.complex128), ("demix_filter", W, (F, M, M), torch.complex128)))
        self._arg("GradBSS", "status", status, torch.int32, numel=1)
        if ws is not None:
            check_workspace("GradBSS", ws, self.dev, self._L.assx_gradbss_workspace_bytes(M, F, T))
        return M, F, T

    def gradbss_workspace(self, M, F, T):
        return self._new_workspace(self._L.assx_gradbss_workspace_bytes(M, F, T),
                                   "GradBSS supports 2 <= n_channels <= 8 and an input below 4 GiB; got n_channels=%d, "
                                   "n_bins=%d, n_frames=%d", M, F, T)

    def gradbss_update(self, model, natural, X, W, ws, lr=0.1, eps=1e-12, status=None):
        """One update of W (F,M,M) in place; model: _lib.GRADBSS_IVA / GRADBSS_FDICA."""
        M, F, T = self._gradbss_dims(X, W, ws, status)
        self._check(self._L.assx_gradbss_update(self.ctx, int(model), 1 if natural else 0, ptr(X), ptr(W), ptr(ws),
                                                float(lr), float(eps), M, F, T, ptr(status), self._st()),
                    "assx_gradbss_update")

    def gradbss_loss(self, model, X, W, ws, loss=None):
        """loss (1,) float64 of the W as it stands."""
        M, F, T = self._gradbss_dims(X, W, ws)
        loss = loss if loss is not None else self.empty((1,), dtype=torch.float64)
        self._arg("GradBSS", "loss", loss, torch.float64, numel=1)
        self._check(self._L.assx_gradbss_loss(self.ctx, int(model), ptr(X), ptr(W), ptr(ws), ptr(loss), M, F, T,
                                              self._st()), "assx_gradbss_loss")
        return loss

    def gradbss_iterate(self, n_iter, model, natural, X, W, ws, lr=0.1, eps=1e-12, loss=None, status=None):
        """n_iter updates; loss: (n_iter + 1,) float64 (the loss before the loop and after every update) or None."""
        M, F, T = self._gradbss_dims(X, W, ws, status)
        self._arg("GradBSS", "loss", loss, torch.float64, numel=int(n_iter) + 1)
        self._check(self._L.assx_gradbss_iterate(self.ctx, int(n_iter), int(model), 1 if natural else 0, ptr(X), ptr(W),
                                                 ptr(ws), float(lr), float(eps), ptr(loss), M, F, T, ptr(status),
                                                 self._st()), "assx_gradbss_iterate")

    def fdica_solve_permutation(self, X, W, ws, eps=1e-12):
        """FDICA's permutation solver on W (F,M,M) in place; returns (order (F,), perm (F,M)) int32."""
        M, F, T = self._gradbss_dims(X, W, ws)
        order = self.empty((F,), dtype=torch.int32)
        perm = self.empty((F, M), dtype=torch.int32)
        self._check(self._L.assx_fdica_solve_permutation(self.ctx, ptr(X), ptr(W), ptr(ws), ptr(order), ptr(perm),
                                                         float(eps), M, F, T, self._st()), "assx_fdica_solve_permutation")
        return order, perm

    # ------------------------------------------------------------------ ProxLaplaceIVA (bss/prox.py, bss/iva.py)
    def _pdsbss_dims(self, X, W=None, y=None, norm=None, ws=None, status=None):
        if X.dim() != 3:
            raise ValueError("PDSBSS: expected input (M,F,T), got %s" % (tuple(X.shape),))
        M, F, T = (int(d) for d in X.shape)
        self._args("PDSBSS", (("input", X, (M, F, T), torch.complex128),))
        if W is not None:
            self._args("PDSBSS", (("demix_filter", W, (F, M, M), torch.complex128),))
        if y is not None:
            self._args("PDSBSS", (("y", y, (F, M, T), torch.complex128),))
        if norm is not None:
            self._arg("PDSBSS", "norm", norm, torch.float64, numel=1)
        self._arg("PDSBSS", "status", status, torch.int32, numel=1)
        if ws is not None:
            check_workspace("PDSBSS", ws, self.dev, self._L.assx_pdsbss_workspace_bytes(M, F, T))
        return M, F, T

    def pdsbss_workspace(self, M, F, T):
        return self._new_workspace(self._L.assx_pdsbss_workspace_bytes(M, F, T),
                                   "PDSBSS supports 2 <= n_channels <= 8 and an input below 4 GiB; got n_channels=%d, "
                                   "n_bins=%d, n_frames=%d", M, F, T)

    def pdsbss_operator_norm(self, X, ws, norm=None, status=None):
        """norm (1,) float64 = max_f sigma_max(X_f); stays on the device."""
        M, F, T = self._pdsbss_dims(X, ws=ws, status=status)
        norm = norm if norm is not None else self.empty((1,), dtype=torch.float64)
        self._arg("PDSBSS", "norm", norm, torch.float64, numel=1)
        self._check(self._L.assx_pdsbss_operator_norm(self.ctx, ptr(X), ptr(ws), ptr(norm), M, F, T, ptr(status),
                                                      self._st()), "assx_pdsbss_operator_norm")
        return norm

    def pdsbss_adjoint(self, X, norm, y, ws):
        """G (F,M,M) = sum_t conj(X / norm) y."""
        M, F, T = self._pdsbss_dims(X, y=y, norm=norm, ws=ws)
        G = self.empty((F, M, M), dtype=torch.complex128)
        self._check(self._L.assx_pdsbss_adjoint(self.ctx, ptr(X), ptr(norm), ptr(y), ptr(G), ptr(ws), M, F, T, self._st()),
                    "assx_pdsbss_adjoint")
        return G

    def pdsbss_prox_logdet(self, W, mu=1.0, status=None):
        """(F,M,M) -> (F,M,M): per bin U h(S) V^H of the SVD of W, h(s) = (s + sqrt(s^2 + 4 mu)) / 2."""
        if W.dim() != 3 or W.shape[1] != W.shape[2]:
            raise ValueError("PDSBSS: expected demix_filter (F,M,M), got %s" % (tuple(W.shape),))
        F, M = int(W.shape[0]), int(W.shape[1])
        self._arg("PDSBSS", "demix_filter", W, torch.complex128, shape=(F, M, M))
        self._arg("PDSBSS", "status", status, torch.int32, numel=1)
        out = self.empty((F, M, M), dtype=torch.complex128)
        self._check(self._L.assx_pdsbss_prox_logdet(self.ctx, ptr(W), ptr(out), float(mu), M, F, ptr(status), self._st()),
                    "assx_pdsbss_prox_logdet")
        return out

    def pdsbss_forward(self, X, norm, y, D):
        """z (F,M,T) = y + (X / norm) D."""
        M, F, T = self._pdsbss_dims(X, W=D, y=y, norm=norm)
        z = self.empty((F, M, T), dtype=torch.complex128)
        self._check(self._L.assx_pdsbss_forward(self.ctx, ptr(X), ptr(norm), ptr(y), ptr(D), ptr(z), M, F, T, self._st()),
                    "assx_pdsbss_forward")
        return z

    def pdsbss_prox_group(self, z, ws, C=1.0, mu=1.0, penalty=_lib.PDSBSS_LAPLACE):
        """(F,N,T) -> (F,N,T): C max(0, 1 - mu / den) z, den[n,t] = sqrt(sum_f |z|^2) (mu where it is <= 0)."""
        if z.dim() != 3:
            raise ValueError("PDSBSS: expected z (F,N,T), got %s" % (tuple(z.shape),))
        F, N, T = (int(d) for d in z.shape)
        self._arg("PDSBSS", "z", z, torch.complex128, shape=(F, N, T))
        check_workspace("PDSBSS", ws, self.dev, self._L.assx_pdsbss_workspace_bytes(N, F, T))
        out = self.empty((F, N, T), dtype=torch.complex128)
        self._check(self._L.assx_pdsbss_prox_group(self.ctx, int(penalty), ptr(z), ptr(out), ptr(ws), float(C), float(mu), N,
                                                   F, T, self._st()), "assx_pdsbss_prox_group")
        return out

    def pdsbss_update(self, X, norm, W, y, ws, C=1.0, mu1=1.0, mu2=1.0, alpha=1.0, status=None,
                      penalty=_lib.PDSBSS_LAPLACE):
        """One iteration on W (F,M,M) and y (F,M,T), both in place."""
        M, F, T = self._pdsbss_dims(X, W, y, norm, ws, status)
        self._check(self._L.assx_pdsbss_update(self.ctx, int(penalty), ptr(X), ptr(norm), ptr(W), ptr(y), ptr(ws), float(C),
                                               float(mu1), float(mu2), float(alpha), M, F, T, ptr(status), self._st()),
                    "assx_pdsbss_update")

    def pdsbss_loss(self, X, W, ws, C=1.0, loss=None, terms=None, penalty=_lib.PDSBSS_LAPLACE):
        """loss (1,) float64 of the W as it stands; terms (2,): the penalty and the negative log-determinant."""
        M, F, T = self._pdsbss_dims(X, W, ws=ws)
        loss = loss if loss is not None else self.empty((1,), dtype=torch.float64)
        self._arg("PDSBSS", "loss", loss, torch.float64, numel=1)
        self._arg("PDSBSS", "terms", terms, torch.float64, numel=2)
        self._check(self._L.assx_pdsbss_loss(self.ctx, int(penalty), ptr(X), ptr(W), ptr(ws), float(C), ptr(loss), ptr(terms),
                                             M, F, T, self._st()), "assx_pdsbss_loss")
        return loss

    def pdsbss_iterate(self, n_iter, X, norm, W, y, ws, C=1.0, mu1=1.0, mu2=1.0, alpha=1.0, loss=None, status=None,
                       penalty=_lib.PDSBSS_LAPLACE):
        """n_iter iterations; loss: (n_iter + 1,) float64 (before the loop and after every iteration) or None."""
        M, F, T = self._pdsbss_dims(X, W, y, norm, ws, status)
        self._arg("PDSBSS", "loss", loss, torch.float64, numel=int(n_iter) + 1)
        self._check(self._L.assx_pdsbss_iterate(self.ctx, int(n_iter), 0 if loss is None else 1, int(penalty), ptr(X),
                                                ptr(norm), ptr(W), ptr(y), ptr(ws), float(C), float(mu1), float(mu2),
                                                float(alpha), ptr(loss), M, F, T, ptr(status), self._st()),
                    "assx_pdsbss_iterate")

    # ------------------------------------------------------------------ beamformers, PCA, MDP (bss/beamform.py, ...)
    def _bf_weights(self, A):
        if A.dim() != 3:
            raise ValueError("beamform: expected steering_vector (F,M,N), got %s" % (tuple(A.shape),))
        F, M, N = (int(d) for d in A.shape)
        self._arg("beamform", "steering_vector", A, torch.complex128, shape=(F, M, N))
        return F, M, N, self.empty((F, N, M), dtype=torch.complex128), self.empty((F, N), dtype=torch.complex128)

    def bf_workspace(self, C, N, F, T):
        return self._new_workspace(self._L.assx_bf_workspace_bytes(C, N, F, T),
                                   "MDP supports 1 to 8 reference channels and sources and arrays below 4 GiB; got "
                                   "n_channels=%d, n_sources=%d, n_bins=%d, n_frames=%d", C, N, F, T)

    def bf_apply(self, X, Wf, s=None):
        """Y (N,F,T) = s[f,n] sum_m Wf[f,n,m] X[m,f,t] for X (M,F,T), Wf (F,N,M) and an optional s (F,N)."""
        if X.dim() != 3 or Wf.dim() != 3:
            raise ValueError("beamform: expected input (M,F,T) and a filter (F,N,M), got %s and %s"
                             % (tuple(X.shape), tuple(Wf.shape)))
        M, F, T = (int(d) for d in X.shape)
        N = int(Wf.shape[1])
        self._args("beamform", (("input", X, (M, F, T), torch.complex128), ("filter", Wf, (F, N, M), torch.complex128),
                                ("scale", s, (F, N), torch.complex128)))
        Y = self.empty((N, F, T), dtype=torch.complex128)
        self._check(self._L.assx_bf_apply(self.ctx, ptr(X), ptr(Wf), ptr(s), ptr(Y), M, N, F, T, self._st()), "assx_bf_apply")
        return Y

    def bf_ds_weights(self, A, ref=0):
        """(Wf (F,N,M), s (F,N)) of the delay-and-sum beamformer for steering vectors A (F,M,N)."""
        F, M, N, Wf, s = self._bf_weights(A)
        self._check(self._L.assx_bf_ds_weights(self.ctx, ptr(A), ptr(Wf), ptr(s), int(ref), M, N, F, self._st()),
                    "assx_bf_ds_weights")
        return Wf, s

    def bf_ml_weights(self, A, R, ref=0, eps=1e-12, status=None):
        """(Wf, s) of the ML beamformer for A (F,M,N) and a covariance R (F,M,M)."""
        F, M, N, Wf, s = self._bf_weights(A)
        self._arg("beamform", "covariance", R, torch.complex128, shape=(F, M, M))
        self._arg("beamform", "status", status, torch.int32, numel=1)
        self._check(self._L.assx_bf_ml_weights(self.ctx, ptr(A), ptr(R), ptr(Wf), ptr(s), int(ref), float(eps), M, N, F,
                                               ptr(status), self._st()), "assx_bf_ml_weights")
        return Wf, s

    def pca_basis(self, C, status=None):
        """(V (F,M,M), w (F,M) ascending, Wf (F,M,M) = V^H) of a Hermitian C (F,M,M)."""
        if C.dim() != 3 or C.shape[1] != C.shape[2]:
            raise ValueError("pca: expected covariance (F,M,M), got %s" % (tuple(C.shape),))
        F, M = int(C.shape[0]), int(C.shape[1])
        self._arg("pca", "covariance", C, torch.complex128, shape=(F, M, M))
        self._arg("pca", "status", status, torch.int32, numel=1)
        V, Wf = self.empty((F, M, M), dtype=torch.complex128), self.empty((F, M, M), dtype=torch.complex128)
        w = self.empty((F, M), dtype=torch.float64)
        self._check(self._L.assx_pca_basis(self.ctx, ptr(C), ptr(V), ptr(w), ptr(Wf), M, F, ptr(status), self._st()),
                    "assx_pca_basis")
        return V, w, Wf

    def mdp_scale(self, Y, Xref, ws=None):
        """scale (C,N,F) = sum_t conj(Y) Xref / sum_t |Y|^2 for Y (N,F,T) and Xref (C,F,T)."""
        if Y.dim() != 3 or Xref.dim() != 3:
            raise ValueError("MDP: expected Y (N,F,T) and a reference (C,F,T), got %s and %s"
                             % (tuple(Y.shape), tuple(Xref.shape)))
        N, F, T = (int(d) for d in Y.shape)
        C = int(Xref.shape[0])
        self._args("MDP", (("Y", Y, (N, F, T), torch.complex128), ("reference", Xref, (C, F, T), torch.complex128)))
        ws = ws if ws is not None else self.bf_workspace(C, N, F, T)
        check_workspace("MDP", ws, self.dev, self._L.assx_bf_workspace_bytes(C, N, F, T))
        scale = self.empty((C, N, F), dtype=torch.complex128)
        self._check(self._L.assx_mdp_scale(self.ctx, ptr(Y), ptr(Xref), ptr(scale), ptr(ws), C, N, F, T, self._st()),
                    "assx_mdp_scale")
        return scale

    # ------------------------------------------------------------------ GaussIDLMA around its network (sss/idlma.py)
    def _idlma_dims(self, X, W, ws=None, status=None, **maps):
        """(M, F, T) of X (M,F,T) and W (F,M,M); maps: name -> ((N,F,T) tensor or None, its dtype)."""
        if X.dim() != 3:
            raise ValueError("IDLMA: expected input (M,F,T), got %s" % (tuple(X.shape),))
        M, F, T = (int(d) for d in X.shape)
        self._args("IDLMA", (("input", X, (M, F, T), torch.complex128), ("demix_filter", W, (F, M, M), torch.complex128)))
        for name, (a, dtype) in maps.items():
            self._arg("IDLMA", name, a, dtype, shape=(M, F, T))
        self._arg("IDLMA", "status", status, torch.int32, numel=1)
        if ws is not None:
            check_workspace("IDLMA", ws, self.dev, self._L.assx_idlma_workspace_bytes(M, F, T))
        return M, F, T

    def idlma_workspace(self, M, F, T):
        return self._new_workspace(self._L.assx_idlma_workspace_bytes(M, F, T),
                                   "IDLMA supports 2 <= n_channels <= 8, n_frames >= n_channels and an input below 4 GiB; "
                                   "got n_channels=%d, n_bins=%d, n_frames=%d", M, F, T)

    def idlma_dnn_input(self, X, W, domain=2, out=None):
        """The network's input (N,F,T) float32 = (|W_f x|^2)^(domain/2) for X (M,F,T) and W (F,N,M)."""
        M, F, T = self._idlma_dims(X, W, dnn_input=(out, torch.float32))
        out = out if out is not None else self.empty((M, F, T), dtype=torch.float32)
        self._check(self._L.assx_idlma_dnn_input(self.ctx, ptr(X), ptr(W), float(domain), ptr(out), M, F, T, self._st()),
                    "assx_idlma_dnn_input")
        return out

    def idlma_variance(self, network_output, dnn_output, R, domain=2, dnn_flooring=1e-5, eps=1e-12):
        """dnn_output (N,F,T) float32 from the network's float32 output (None: dnn_output is read as it stands) and the
        variance R (N,F,T) float64, both written in place."""
        if dnn_output.dim() != 3:
            raise ValueError("IDLMA: expected dnn_output (N,F,T), got %s" % (tuple(dnn_output.shape),))
        N, F, T = (int(d) for d in dnn_output.shape)
        self._args("IDLMA", (("network_output", network_output, (N, F, T), torch.float32),
                             ("dnn_output", dnn_output, (N, F, T), torch.float32), ("R", R, (N, F, T), torch.float64)))
        self._check(self._L.assx_idlma_variance(self.ctx, ptr(network_output), float(domain), float(dnn_flooring), float(eps),
                                                ptr(dnn_output), ptr(R), N, F, T, self._st()), "assx_idlma_variance")

    def idlma_normalize_pb(self, W, scale):
        """W (F,N,M) in place: W[f,n,:] *= scale[n,f] for scale (N,F)."""
        if W.dim() != 3 or W.shape[1] != W.shape[2]:
            raise ValueError("IDLMA: expected demix_filter (F,M,M), got %s" % (tuple(W.shape),))
        F, M = int(W.shape[0]), int(W.shape[1])
        self._args("IDLMA", (("demix_filter", W, (F, M, M), torch.complex128), ("scale", scale, (M, F), torch.complex128)))
        self._check(self._L.assx_idlma_normalize_pb(self.ctx, ptr(W), ptr(scale), M, F, self._st()), "assx_idlma_normalize_pb")

    def idlma_loss(self, X, W, R, ws, loss=None):
        """loss (1,) float64 of W (F,N,M) and the variance R (N,F,T) float64."""
        M, F, T = self._idlma_dims(X, W, ws=ws, R=(R, torch.float64))
        loss = loss if loss is not None else self.empty((1,), dtype=torch.float64)
        self._arg("IDLMA", "loss", loss, torch.float64, numel=1)
        self._check(self._L.assx_idlma_loss(self.ctx, ptr(X), ptr(W), ptr(R), ptr(loss), ptr(ws), M, F, T, self._st()),
                    "assx_idlma_loss")
        return loss

    def idlma_step(self, X, W, network_output, dnn_output, ws, domain=2, dnn_flooring=1e-5, eps=1e-12, threshold=1e12, ref=0,
                   loss=None, next_input=None, status=None):
        """Everything between two evaluations of the network in one call: W (F,N,M) and dnn_output (N,F,T) float32 in place,
        loss (1,) float64 of the updated model and the network's next input (N,F,T) float32 where given."""
        M, F, T = self._idlma_dims(X, W, ws=ws, status=status, network_output=(network_output, torch.float32),
                                   dnn_output=(dnn_output, torch.float32), next_input=(next_input, torch.float32))
        self._arg("IDLMA", "loss", loss, torch.float64, numel=1)
        self._check(self._L.assx_idlma_step(self.ctx, ptr(X), ptr(W), ptr(network_output), float(domain), float(dnn_flooring),
                                            float(eps), float(threshold), int(ref), ptr(dnn_output), ptr(loss),
                                            ptr(next_input), ptr(status), ptr(ws), M, F, T, self._st()), "assx_idlma_step")

    # ------------------------------------------------------------------ projection back
    def projection_back_scale(self, X, W, ref=0, status=None):
        B, M, F, T = self._dims(X)
        scale = self.empty((B, M, F), complex_=True)
        ws = self._scratch(B, M, F, T, 1)
        self._check(self._L.assx_projection_back_scale(self.ctx, ptr(X), ptr(W), int(ref), ptr(scale), ptr(status), ptr(ws),
                                                 B, M, F, T, self.prec.code, self._st()), "assx_projection_back_scale")
        return scale

    def projection_back(self, Y, reference, status=None):
        B, N, F, T = self._dims(Y)
        scale = self.empty((B, N, F), complex_=True)
        ws = self._scratch(B, N, F, T, 1)
        self._check(self._L.assx_projection_back(self.ctx, ptr(Y), ptr(reference), ptr(scale), ptr(status), ptr(ws), B, N, F,
                                           T, self.prec.code, self._st()), "assx_projection_back")
        return scale

    # ------------------------------------------------------------------ least-squares demixing filter
    def compute_demix_filter(self, Y, X, status=None):
        """W (B,F,M,M) = (Y X^H)(X X^H)^-1 per bin for Y, X (B,M,F,T)."""
        B, M, F, T = self._dims(X)
        W = self.empty((B, F, M, M), complex_=True)
        self._check(self._L.assx_compute_demix_filter(self.ctx, ptr(Y), ptr(X), ptr(W), ptr(status), B, M, F, T,
                                                      self.prec.code, self._st()), "assx_compute_demix_filter")
        return W

    # ------------------------------------------------------------------ pieces for the F-sharded mode (row f2)
    def ilrma_power_map(self, X, W, out=None):
        """P (B,N,F,T) real = |W x|^2."""
        B, M, F, T = self._dims(X)
        P = out if out is not None else self.empty((B, M, F, T))
        self._check(self._L.assx_ilrma_power_map(self.ctx, ptr(X), ptr(W), ptr(P), B, M, F, T, self.prec.code, self._st()),
                    "assx_ilrma_power_map")
        return P

    def nmf_half_sums(self, kind, half, X, Tb, V, domain=2, eps=1e-12, param=0.0, out=None):
        """(2, B, F*K) [half 0: basis] or (2, B, K*T) [half 1: activation] numerators / denominators of one half of a
        multiplicative update on X (B,F,T), not applied."""
        B, F, T = (int(s) for s in X.shape)
        K = int(Tb.shape[-1])
        count = F * K if int(half) == 0 else K * T
        sums = out if out is not None else self.empty((2, B, count))
        ws = self._nmf_scratch(B, F, T, K)
        self._check(self._L.assx_nmf_half_sums(self.ctx, int(kind), float(domain), float(param), float(eps), int(half),
                                               ptr(X), ptr(Tb), ptr(V), ptr(sums), ptr(ws), B, F, T, K, self.prec.code,
                                               self._st()), "assx_nmf_half_sums")
        return sums

    def nmf_apply_sums(self, kind, A, sums, domain=2, eps=1e-12):
        """A (B, ...) *= (num / max(den, eps)) ** exponent(kind, domain), sums (2, B, count)."""
        B = int(sums.shape[1])
        count = int(sums.shape[2])
        self._check(self._L.assx_nmf_apply_sums(self.ctx, int(kind), float(domain), float(eps), ptr(A), ptr(sums), B,
                                                count, self.prec.code, self._st()), "assx_nmf_apply_sums")
        return A

    def ordered_sum(self, parts, weights=None):
        """sum over the leading axis of `parts` (S, ...) in ascending order, optionally weighted (float64 (S,))."""
        S = int(parts.shape[0])
        count = int(parts[0].numel())
        if parts.dtype not in (torch.float64, torch.float32):
            raise ValueError("ordered_sum: float64 / float32 only")
        code = _lib.F64 if parts.dtype == torch.float64 else _lib.F32
        out = torch.empty(parts.shape[1:], dtype=parts.dtype, device=self.dev)
        self._check(self._L.assx_ordered_sum(self.ctx, ptr(parts.contiguous()), ptr(weights), ptr(out), S, count, code,
                                             self._st()), "assx_ordered_sum")
        return out

    # ------------------------------------------------------------------ NMF
    def _nmf_scratch(self, B, F, T, K):
        return self._ws.get(self._L.assx_nmf_workspace_bytes(B, F, T, K, self.prec.code))

    def nmf_update(self, kind, X, Tb, V, domain=2, eps=1e-12, param=0.0):
        B, F, T = (int(s) for s in X.shape)
        K = int(Tb.shape[-1])
        ws = self._nmf_scratch(B, F, T, K)
        self._check(self._L.assx_nmf_update_ex(self.ctx, int(kind), float(domain), float(param), float(eps), ptr(X), ptr(Tb),
                                         ptr(V), ptr(ws), B, F, T, K, self.prec.code, self._st()), "assx_nmf_update_ex")

    def nmf_loss(self, kind, X, Tb, V, domain=2, eps=1e-12, out=None, param=0.0):
        B, F, T = (int(s) for s in X.shape)
        K = int(Tb.shape[-1])
        loss = out if out is not None else self.empty((B,), dtype=torch.float64)
        ws = self._nmf_scratch(B, F, T, K)
        self._check(self._L.assx_nmf_loss_ex(self.ctx, int(kind), float(domain), float(param), float(eps), ptr(X), ptr(Tb),
                                       ptr(V), ptr(loss), ptr(ws), B, F, T, K, self.prec.code, self._st()),
                    "assx_nmf_loss_ex")
        return loss
