"""NumPy restatement of EUCNTF (non-negative tensor factorisation) in the Gram form the HIP kernels use.

The model is partitioning Z (N, K), basis T (I, K), activation V (K, J) for a non-negative target X (N, I, J):
X_hat[n,i,j] = sum_k Z[n,k] T[i,k] V[k,j].  With fl(a) = max(a, eps) one update is

    T' = T o fl(sum_{n,j} X Z V)   / fl(T ((Z^T Z)   o (V V^T)))
    V' = V o fl(sum_{n,i} X Z T')  / fl(((Z^T Z)  o (T'^T T')) V)
    Z' = Z o fl(sum_{i,j} X T' V') / fl(Z ((T'^T T') o (V' V'^T)))

and the model becomes (Z', T', V').  The denominators are sum X_hat Z V and its two analogues with X_hat written out and
the sums over the data axes done first: K x K Gram matrices, no array with both a K and a J axis besides V.  The loss is
sum (X - X_hat)^2, the difference formed per entry.  Written from the equations above; nothing is taken from another
code base.
"""
import glob
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ntf")
SNAP_ITERS = (1, 2, 4, 5, 19, 20)
START_ITERS = (0, 1, 4, 19)  # the recorded states whose successor is recorded too
METRICS = ("Z", "T", "V", "loss")
N_ITER = 20


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "ntf_*.npz")))


def tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as fh:
        return json.load(fh)


def state(fx, it):
    """(Z, T, V) of a fixture after `it` iterations (0: the reference's draws)."""
    if it == 0:
        return fx["Z0"].copy(), fx["T0"].copy(), fx["V0"].copy()
    return tuple(fx["%s_%d" % (a, it)].copy() for a in ("partitioning", "basis", "activation"))


def reconstruct(Z, T, V):
    """(N, I, J): sum_k Z T V."""
    return np.einsum("nk,ik,kj->nij", Z, T, V, optimize=True)


def loss(X, Z, T, V):
    D = X - reconstruct(Z, T, V)
    return float(np.sum(D * D))


def update(X, Z, T, V, eps, sums=None):
    """One update; returns new arrays (Z', T', V') and leaves its inputs alone.  `sums`: a list that receives the three
    (numerator, denominator) pairs before the floor, in the order basis, activation, partitioning."""
    ZZ = Z.T @ Z
    num = np.einsum("nij,nk,kj->ik", X, Z, V, optimize=True)
    den = T @ (ZZ * (V @ V.T))
    Tn = T * (np.maximum(num, eps) / np.maximum(den, eps))
    pairs = [(num, den)]

    TT = Tn.T @ Tn
    num = np.einsum("nij,nk,ik->kj", X, Z, Tn, optimize=True)
    den = (ZZ * TT) @ V
    Vn = V * (np.maximum(num, eps) / np.maximum(den, eps))
    pairs.append((num, den))

    num = np.einsum("nij,ik,kj->nk", X, Tn, Vn, optimize=True)
    den = Z @ (TT * (Vn @ Vn.T))
    Zn = Z * (np.maximum(num, eps) / np.maximum(den, eps))
    pairs.append((num, den))
    if sums is not None:
        sums.extend(pairs)
    return Zn, Tn, Vn


def run(X, model, eps, n):
    """The models after 1..n updates from `model` = (Z, T, V)."""
    out = []
    for _ in range(n):
        model = update(X, *model, eps)
        out.append(model)
    return out


def rel_entry(a, b):
    """Largest |a - b| / |b| over the entries; every entry of the reference b is positive."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def compare(got, want, X):
    """The four metrics of a model `got` against `want` (each a (Z, T, V) triple), entry by entry."""
    return {"Z": rel_entry(got[0], want[0]), "T": rel_entry(got[1], want[1]), "V": rel_entry(got[2], want[2]),
            "loss": rel_entry(loss(X, *got), loss(X, *want))}


def one_ulp(a, rng):
    """Every entry moved to a neighbouring double, direction drawn per entry."""
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def synthetic(N, I, J, K, seed):
    """A target and a model for the shapes the fixtures do not cover (same recipe as the fixtures' plain targets)."""
    rng = np.random.default_rng(seed)
    X = reconstruct(rng.random((N, 3)), rng.random((I, 3)), rng.random((3, J))) * (1 + 0.01 * rng.random((N, I, J)))
    return X, rng.random((N, K)), rng.random((I, K)), rng.random((K, J))
