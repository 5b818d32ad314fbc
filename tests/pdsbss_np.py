"""Independent NumPy restatement of ProxLaplaceIVA (reference src/bss/iva.py:831-904) on PDSBSSbase (src/bss/prox.py:13-201),
written from the formulas of DESIGN.md section 19.  The reference states the algorithm with scipy.sparse, as one block-diagonal
operator with a block per (bin, source); here it is dense algebra per bin, the shape the GPU kernels use.  Nothing here is
copied from the reference; tests/golden/pdsbss pins it to the reference's recorded output.

Shapes: X (M,F,T) complex, W (F,N,M) complex with N = M, the dual y (F,N,T) complex, norm a float.
"""
import functools

import numpy as np

from gradbss_np import identity, mixture, separate  # noqa: F401  the same inputs and the same output stage

N_ITER = 10
SNAP_ITERS = (1, 2, 5, 10)
STAGE_ITERS = (1, 2)
STAGES = ("G", "Wt", "z", "yt")


def operator_norm(X):
    """The largest singular value of the block operator: max over the bins of sigma_max of the (T,M) slice."""
    return float(max(np.linalg.svd(X[:, f, :], compute_uv=False)[0] for f in range(X.shape[1])))


def adjoint(Xn, y, no_conj=False):
    """G[f,n,m] = sum_t conj(Xn[m,f,t]) y[f,n,t].  no_conj: a planted fault."""
    A = Xn if no_conj else Xn.conj()
    return np.stack([y[f] @ A[:, f, :].T for f in range(Xn.shape[1])])


def h(sigma, mu):
    return (sigma + np.sqrt(sigma ** 2 + 4 * mu)) / 2


def prox_logdet(W, mu):
    """Per bin U h(S) V^H of the SVD of W."""
    out = np.empty_like(W)
    for f in range(W.shape[0]):
        U, S, Vh = np.linalg.svd(W[f])
        out[f] = (U * h(S, mu)) @ Vh
    return out


def forward(Xn, y, D):
    """z[f,n,t] = y[f,n,t] + sum_m Xn[m,f,t] D[f,n,m]."""
    return np.stack([y[f] + D[f] @ Xn[:, f, :] for f in range(Xn.shape[1])])


def group_norm(z):
    """den[n,t] = sqrt(sum_f |z[f,n,t]|^2), bins streamed."""
    r2 = np.zeros(z.shape[1:])
    for f in range(z.shape[0]):
        r2 += np.abs(z[f]) ** 2
    return np.sqrt(r2)


def prox_group(z, mu, C, per_bin=False, drop_c=False):
    """C max(0, 1 - mu / den) z with den the norm across the bins (mu where it is <= 0).  per_bin / drop_c: planted faults."""
    den = np.abs(z) if per_bin else group_norm(z)[None]
    den = np.where(den <= 0, mu, den)
    return (1.0 if drop_c else C) * np.maximum(0, 1 - mu / den) * z


def shrinking(z, mu):
    """The (n,t) cells of z that the prox shrinks (den > mu), as a boolean array, and the smallest relative distance of a
    den from mu."""
    den = group_norm(z)
    den = np.where(den <= 0, mu, den)
    return den > mu, float(np.min(np.abs(den - mu)) / mu)


def update(Xn, W, y, C=1.0, mu1=1.0, mu2=1.0, alpha=1.0, no_conj=False, z_from_wt=False, per_bin=False, drop_c=False):
    """One iteration: (W, y, stages) with stages = {G, arg, Wt, z, yt}."""
    G = adjoint(Xn, y, no_conj)
    arg = W - mu1 * mu2 * G
    Wt = prox_logdet(arg, mu1)
    z = forward(Xn, y, Wt if z_from_wt else 2 * Wt - W)
    yt = z - prox_group(z, 1 / mu2, C, per_bin, drop_c)
    return alpha * Wt + (1 - alpha) * W, alpha * yt + (1 - alpha) * y, dict(G=G, arg=arg, Wt=Wt, z=z, yt=yt)


def penalty(X, W, C=1.0):
    r2 = np.zeros((W.shape[1], X.shape[2]))
    for f in range(X.shape[1]):
        r2 += np.abs(W[f] @ X[:, f, :]) ** 2
    return C * np.sqrt(r2).sum()


def negative_logdet(W):
    return -sum(np.log(np.abs(np.linalg.det(W[f]))) for f in range(W.shape[0]))


def loss(X, W, C=1.0):
    """With the unnormalised X."""
    return penalty(X, W, C) + negative_logdet(W)


def run(X, W0, n_iter=N_ITER, norm=None, C=1.0, mu1=1.0, mu2=1.0, alpha=1.0, **fault):
    """({iteration: (W, y)}, [loss before the loop, loss after every iteration], {iteration: stages})."""
    norm = operator_norm(X) if norm is None else norm
    Xn = X / norm
    W, y = W0.copy(), np.zeros((X.shape[1], W0.shape[1], X.shape[2]), dtype=np.complex128)
    states, losses, stages = {0: (W, y)}, [loss(X, W, C)], {}
    for it in range(1, n_iter + 1):
        W, y, st = update(Xn, W, y, C, mu1, mu2, alpha, **fault)
        states[it], stages[it] = (W, y), st
        losses.append(loss(X, W, C))
    return states, losses, stages


def params(g):
    """The four real parameters of a fixture."""
    return dict(C=float(g["C"]), mu1=float(g["mu1"]), mu2=float(g["mu2"]), alpha=float(g["alpha"]))


def cases(golden_dir):
    """The names of the recorded cases (a case is `<name>.npz` and its numbered parts `<name>.part<i>.npz`)."""
    import glob
    import os
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "*.npz")) if ".part" not in p)


@functools.lru_cache(maxsize=None)
def load_case(golden_dir, name):
    """Every array of a case, its parts put together, as a dict of read-only arrays."""
    import os
    head = np.load(os.path.join(golden_dir, name + ".npz"))
    out = {k: head[k] for k in head.files}
    for i in range(1, int(out["n_parts"])):
        part = np.load(os.path.join(golden_dir, "%s.part%d.npz" % (name, i)))
        out.update({k: part[k] for k in part.files})
    for v in out.values():
        v.setflags(write=False)
    return out
