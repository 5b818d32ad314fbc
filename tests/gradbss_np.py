"""Independent NumPy restatement of the gradient family: GradLaplaceIVA, NaturalGradLaplaceIVA (reference
src/bss/iva.py:130-287), GradLaplaceFDICA, NaturalGradLaplaceFDICA and FDICAbase.solve_permutation (src/bss/fdica.py:8-301),
written from the formulas of DESIGN.md section 18 in the shape the GPU kernels use: bins are streamed one at a time, the
N x M cross-moment of a bin is one matrix product, and the solver scores the N! candidates of a bin from an N x N matrix.
Nothing here is copied from the reference; tests/golden/gradbss pins it to the reference's recorded output.

Shapes: X (M,F,T) complex, W (F,N,M) complex with N = M, order (F,) and perm (F,N) integers.
"""
import functools
import itertools

import numpy as np

EPS = 1e-12
LR = 0.1
N_ITER = 10
SNAP_ITERS = (1, 2, 5, 10)
MODELS = ("iva", "fdica")
CLASSES = {"GradLaplaceIVA": ("iva", False), "NaturalGradLaplaceIVA": ("iva", True),
           "GradLaplaceFDICA": ("fdica", False), "NaturalGradLaplaceFDICA": ("fdica", True)}


def mixture(M, F, T, seed):
    """A seeded convolutive mixture of Laplacian sources, scaled to unit mean power."""
    rng = np.random.default_rng(seed)
    S = rng.laplace(size=(M, F, T)) + 1j * rng.laplace(size=(M, F, T))
    S = S * (0.2 + rng.random((M, 1, T)))  # frame envelopes, shared by the bins of a source
    A = rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))
    X = np.einsum("fmn,nft->mft", A, S)
    return X / np.sqrt(np.mean(np.abs(X) ** 2))


def identity(M, F):
    return np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1))


def demix_bin(X, W, f):
    return W[f] @ X[:, f, :]  # (N, T)


def frame_weights(X, W):
    """r[n,t] = sqrt(sum_f |y[n,f,t]|^2), bins streamed."""
    r2 = np.zeros((W.shape[1], X.shape[2]))
    for f in range(X.shape[1]):
        r2 += np.abs(demix_bin(X, W, f)) ** 2
    return np.sqrt(r2)


def floor(a, eps):
    return np.where(a < eps, eps, a)


def update(model, natural, X, W, lr=LR, eps=EPS, floor_square=False, natural_with_x=False):
    """One update of every bin.  floor_square / natural_with_x: the planted faults of tests/test_gradbss_cpu.py."""
    M, F, T = X.shape
    if model == "iva":
        r = frame_weights(X, W)
        den_all = np.sqrt(floor(r ** 2, eps)) if floor_square else floor(r, eps)
    out = np.empty_like(W)
    for f in range(F):
        x = X[:, f, :]
        y = W[f] @ x
        den = den_all if model == "iva" else floor(np.abs(y), eps)
        phi = y / den
        if natural:
            z = x if natural_with_x else y
            G = (phi @ z.conj().T) / T
            out[f] = W[f] - lr * ((G - np.eye(M)) @ W[f])
        else:
            G = (phi @ x.conj().T) / T
            out[f] = W[f] - lr * (G - np.linalg.inv(W[f]).conj().T)
    return out


def loss(model, X, W):
    M, F, T = X.shape
    logdet = sum(np.log(np.abs(np.linalg.det(W[f]))) for f in range(F))
    if model == "iva":
        data = frame_weights(X, W).sum()
    else:
        data = sum(np.abs(demix_bin(X, W, f)).sum() for f in range(F))
    return 2.0 * data / T - 2.0 * logdet


def smallest_denominator(model, X, W):
    """The smallest value that the score function floors at eps."""
    if model == "iva":
        return float(frame_weights(X, W).min())
    return float(min(np.abs(demix_bin(X, W, f)).min() for f in range(X.shape[1])))


def run(model, natural, X, W0, n_iter=N_ITER, lr=LR, eps=EPS, **fault):
    """({iteration: W}, [loss before the loop, loss after every iteration])."""
    W = W0.copy()
    states, losses = {0: W}, [loss(model, X, W)]
    for it in range(1, n_iter + 1):
        W = update(model, natural, X, W, lr, eps, **fault)
        states[it] = W
        losses.append(loss(model, X, W))
    return states, losses


# ---------------------------------------------------------------------------------------------------------- the solver
def presence(X, W, f, eps=EPS):
    """P[n,t] = |y| / max(sqrt(sum_n |y|^2), eps) of bin f."""
    a = np.abs(demix_bin(X, W, f))
    return a / floor(np.sqrt((a ** 2).sum(axis=0, keepdims=True)), eps)


def correlations(X, W, eps=EPS):
    return np.array([(presence(X, W, f, eps).sum(axis=0) ** 2).sum() for f in range(X.shape[1])])


def rank_order(c):
    """The device's rule for ANY values: ascending, equal values by index, NaN last by index.  order[rank of f] = f with
    the rank of a bin = the number of bins before it, so the result is a permutation of 0..F-1 whatever c holds."""
    c = np.asarray(c, dtype=np.float64)
    F = c.size
    order = np.full(F, -1, dtype=np.int64)
    for f in range(F):
        rank = 0
        for g in range(F):
            ng, nf = np.isnan(c[g]), np.isnan(c[f])
            if ng != nf:
                before = nf
            elif ng:
                before = g < f
            else:
                before = c[g] < c[f] or (c[g] == c[f] and g < f)
            rank += bool(before)
        order[rank] = f
    return order


def best_permutation(C):
    """(perm, scores): the first permutation in lexicographic order whose sum_n C[n, pi(n)] is the largest, compared
    with strict > from the identity on (a NaN never wins, and a NaN identity is never beaten)."""
    N = C.shape[0]
    perms = _permutations(N)
    scores = np.zeros(len(perms))
    for n in range(N):  # n ascending, as the kernel adds
        scores = scores + C[n, perms[:, n]]
    if np.isnan(scores[0]):
        return perms[0].copy(), scores
    best = int(np.argmax(np.where(np.isnan(scores), -np.inf, scores)))  # the first of equals
    return perms[best].copy(), scores


@functools.lru_cache(maxsize=None)
def _permutations(N):
    """(N!, N): the permutations of 0..N-1 in lexicographic order."""
    return np.array(list(itertools.permutations(range(N))), dtype=np.int64)


def solve_permutation(X, W, eps=EPS, descending=False, columns=False):
    """(W after, order, perm, gaps) with gaps = (smallest relative gap of neighbouring sorted correlations, smallest
    relative gap between the best and the second-best score of a bin).  descending / columns: planted faults."""
    M, F, T = X.shape
    c = correlations(X, W, eps)
    order = rank_order(c)
    if descending:
        order = order[::-1].copy()
    cs = c[order]
    gap_c = float(np.min(np.abs(np.diff(cs)) / np.abs(cs[1:]))) if F > 1 else np.inf
    Wn = W.copy()
    perm = np.tile(np.arange(M), (F, 1))
    crit = presence(X, W, order[0], eps)
    gap_s = np.inf
    for f in order[1:]:
        P = presence(X, W, f, eps)
        p, scores = best_permutation(crit @ P.T)
        top = np.sort(scores)[::-1]
        gap_s = min(gap_s, float((top[0] - top[1]) / abs(top[0])))
        crit = crit + P[p]
        perm[f] = p
        Wn[f] = W[f][:, p] if columns else W[f][p]
    return Wn, order, perm, (gap_c, gap_s)


# ---------------------------------------------------------------------------------------------------------- outputs
def projection_back_scale(Y, ref):
    """scale[n,f] of projection back onto the reference channel `ref` (F,T): per bin the least-squares fit of ref by the
    rows of Y."""
    N, F, T = Y.shape
    scale = np.empty((N, F), dtype=np.complex128)
    for f in range(F):
        y = Y[:, f, :]
        scale[:, f] = (ref[f] @ y.conj().T) @ np.linalg.inv(y @ y.conj().T)
    return scale


def separate(X, W, reference_id=0, projection_back=True):
    Y = np.stack([demix_bin(X, W, f) for f in range(X.shape[1])], axis=1)
    if projection_back:
        Y = Y * projection_back_scale(Y, X[reference_id])[..., None]
    return Y


def fixtures(golden_dir):
    import glob
    import os
    return sorted(glob.glob(os.path.join(golden_dir, "*.npz")))
