"""NumPy restatement of ComplexEUCNMF (Kameoka's complex NMF) in the closed forms the HIP kernels use.

The model is basis T (F, K), activation V (K, T), phase Phi (F, K, T) angles, for a complex target X (F, T).  With
E = exp(i Phi), a = T V (V as it stands) and tv = max(sum_k a, eps), one update is

    ZX   = X - sum_k a E            Beta = max(a / tv, eps)          Zbar = a E + Beta ZX
    Re   = real(conj(Zbar) E)       Vf   = max(V, eps)
    T'   = sum_t (Vf / Beta) Re / max(sum_t Vf^2 / Beta, eps)
    V'   = sum_f (T' / Beta) Re / max(sum_f T'^2 / Beta + regularizer p Vf^(p-2), eps)
    Phi' = angle(Zbar)              T''  = T' / sum_f T'

and the model becomes (T'', V', Phi').  Beta is never state: it is T V / max(sum_k T V, eps) of the current T and V.
The loss of a model is sum |sum_k T V E - X|^2.  Everything is evaluated in chunks of bins, so no more than one chunk
of (K, T) temporaries exists at a time.  Written from the equations above; nothing is taken from another code base.
"""
import glob
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cnmf")
SNAP_ITERS = (1, 2, 5, 19, 20)
CHUNK = 8


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "cnmf_*.npz")))


def tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as fh:
        return json.load(fh)


def initial_phase(X, K):
    return np.tile(np.angle(X)[:, None, :], (1, K, 1))


def state(fx, it):
    """(T, V, Phi) of a fixture after `it` iterations (0: what the reference's _reset leaves)."""
    if it == 0:
        return fx["T0"].copy(), fx["V0"].copy(), initial_phase(fx["X"], fx["T0"].shape[1])
    return fx["basis_%d" % it].copy(), fx["activation_%d" % it].copy(), fx["phase_%d" % it].copy()


def start_iters(fx):
    """The recorded states whose successor is recorded too: 0, 1, 19, and 4 in the files that hold iteration 4."""
    return tuple(it for it in (0, 1, 4, 19) if it == 0 or "basis_%d" % it in fx.files)


def params(fx):
    return float(fx["regularizer"]), float(fx["p"]), float(fx["eps"])


def _chunks(F):
    return [(f0, min(f0 + CHUNK, F)) for f0 in range(0, F, CHUNK)]


def components(T, V, Phi):
    """(F, K, T) complex: T V exp(i Phi)."""
    out = np.empty(Phi.shape, dtype=np.complex128)
    for f0, f1 in _chunks(T.shape[0]):
        out[f0:f1] = (T[f0:f1, :, None] * V[None]) * np.exp(1j * Phi[f0:f1])
    return out


def reconstruct(T, V, Phi):
    out = np.empty((T.shape[0], V.shape[1]), dtype=np.complex128)
    for f0, f1 in _chunks(T.shape[0]):
        out[f0:f1] = ((T[f0:f1, :, None] * V[None]) * np.exp(1j * Phi[f0:f1])).sum(axis=1)
    return out


def loss(X, T, V, Phi):
    Z = reconstruct(T, V, Phi) - X
    return float(np.sum(Z.real ** 2 + Z.imag ** 2))


def beta(T, V, eps):
    out = np.empty((T.shape[0],) + V.shape)
    for f0, f1 in _chunks(T.shape[0]):
        a = T[f0:f1, :, None] * V[None]
        out[f0:f1] = a / np.maximum(a.sum(axis=1, keepdims=True), eps)
    return out


def reg_power(Vf, p):
    if p == 1:
        return 1.0 / Vf
    if p == 2:
        return np.ones_like(Vf)
    return Vf ** (p - 2)


def update(X, T, V, Phi, regularizer, p, eps):
    """One update; returns new arrays (T'', V', Phi') and leaves its inputs alone."""
    F, K = T.shape
    Vf = np.maximum(V, eps)
    Tn = np.empty_like(T)
    Pn = np.empty_like(Phi)
    num_v = np.zeros_like(V)
    den_v = np.zeros_like(V)
    for f0, f1 in _chunks(F):
        E = np.exp(1j * Phi[f0:f1])
        a = T[f0:f1, :, None] * V[None]
        Xk = a * E
        ZX = X[f0:f1] - Xk.sum(axis=1)
        B = np.maximum(a / np.maximum(a.sum(axis=1, keepdims=True), eps), eps)
        Zbar = Xk + B * ZX[:, None, :]
        Re = Zbar.real * E.real + Zbar.imag * E.imag
        Tc = ((Vf[None] / B) * Re).sum(axis=2) / np.maximum(((Vf * Vf)[None] / B).sum(axis=2), eps)
        Tn[f0:f1] = Tc
        num_v += ((Tc[:, :, None] / B) * Re).sum(axis=0)
        den_v += ((Tc * Tc)[:, :, None] / B).sum(axis=0)
        Pn[f0:f1] = np.arctan2(Zbar.imag, Zbar.real)
    Vn = num_v / np.maximum(den_v + (regularizer * p) * reg_power(Vf, p), eps)
    return Tn / Tn.sum(axis=0), Vn, Pn


def rel(a, b):
    """max-abs of the difference over max-abs of the reference b."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), np.finfo(np.float64).tiny))


def compare(got, want, X):
    """The four metrics of a model `got` against `want` (each a (T, V, Phi) triple): T, V, components, loss."""
    return {"T": rel(got[0], want[0]), "V": rel(got[1], want[1]),
            "components": rel(components(*got), components(*want)),
            "loss": rel(loss(X, *got), loss(X, *want))}


def one_ulp(a, rng):
    """Every entry moved to a neighbouring double, direction drawn per entry."""
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def synthetic(F, T, K, seed):
    """A target and a model for the shapes the fixtures do not cover (same recipe as the fixtures' targets)."""
    rng = np.random.default_rng(seed)
    X = (rng.random((F, 3)) @ rng.random((3, T))) * np.exp(2j * np.pi * rng.random((F, T)))
    Tb, V = rng.random((F, K)), rng.random((K, T))
    Phi = np.angle(X)[:, None, :] + 0.3 * rng.standard_normal((F, K, T))
    return X, Tb, V, Phi
