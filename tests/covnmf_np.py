"""Independent NumPy restatement of the covariance-domain MultichannelISNMF (reference src/algorithm/nmf.py:116-148,
678-815) in the closed forms the GPU kernels use.  Nothing here is copied from the reference;
tests/golden/covnmf pins it to the reference's recorded output.

With X^ = sum_k T[f,k] V[k,t] H[f,k], P = (X^ + eps I)^-1 and Q = P X P, the basis and activation updates weight the
traces a_k = Re tr(Q H_k) and b_k = Re tr(P H_k); the spatial update solves H A H = B with A = sum_t V P and
B = H (sum_t V Q) H by the matrix geometric mean (`mnmf_np.riccati`: Cholesky of A, one Hermitian eigendecomposition)
in place of the reference's 2M x 2M eigen-solve.  The loss takes both log-determinants from Cholesky factors.

Shapes: X (F,T,M,M) complex Hermitian, T (F,K) basis, V (K,T) activation, H (F,K,M,M) complex spatial.
"""
import numpy as np

from mnmf_np import riccati

EPS = 1e-12
N_ITER = 20
SNAP_ITERS = (1, 2, 5, 20)


def reconstruct(Tb, V, H):
    return np.einsum("fk,kt,fkij->ftij", Tb, V, H)


def _eval(X, Tb, V, H, eps):
    """P and Q (F,T,M,M), a and b (F,K,T)."""
    M = X.shape[-1]
    P = np.linalg.inv(reconstruct(Tb, V, H) + eps * np.eye(M))
    Q = P @ X @ P
    a = np.einsum("ftij,fkji->fkt", Q, H).real
    b = np.einsum("ftij,fkji->fkt", P, H).real
    return P, Q, a, b


def denominators(X, Tb, V, H, eps=EPS):
    """The smallest of the denominators that the basis and activation updates clamp at eps."""
    _, _, _, b = _eval(X, Tb, V, H, eps)
    return float(min(np.einsum("kt,fkt->fk", V, b).min(), np.einsum("fk,fkt->kt", Tb, b).min()))


def update_basis(X, Tb, V, H, eps=EPS):
    _, _, a, b = _eval(X, Tb, V, H, eps)
    num = np.einsum("kt,fkt->fk", V, a)
    den = np.einsum("kt,fkt->fk", V, b)
    den[den < eps] = eps
    return Tb * np.sqrt(num / den)


def update_activation(X, Tb, V, H, eps=EPS):
    _, _, a, b = _eval(X, Tb, V, H, eps)
    num = np.einsum("fk,fkt->kt", Tb, a)
    den = np.einsum("fk,fkt->kt", Tb, b)
    den[den < eps] = eps
    return V * np.sqrt(num / den)


def update_spatial(X, Tb, V, H, normalize=True, eps=EPS):
    M = X.shape[-1]
    P, Q, _, _ = _eval(X, Tb, V, H, eps)
    A = np.einsum("kt,ftij->fkij", V, P)
    C = np.einsum("kt,ftij->fkij", V, Q)
    Hn = riccati(A, H @ C @ H) + eps * np.eye(M)
    if normalize:
        Hn = Hn / np.trace(Hn, axis1=2, axis2=3)[..., None, None]
    return Hn


def loss(X, Tb, V, H, eps=EPS):
    """sum_{f,t} Re tr((X + eps I)(X^ + eps I)^-1) - ln det(X + eps I) + ln det(X^ + eps I) - M."""
    M = X.shape[-1]
    Xe, Xh = X + eps * np.eye(M), reconstruct(Tb, V, H) + eps * np.eye(M)
    Lx, Lh = np.linalg.cholesky(Xe), np.linalg.cholesky(Xh)
    ldx = 2 * np.log(np.diagonal(Lx, axis1=-2, axis2=-1).real).sum(axis=-1)
    ldh = 2 * np.log(np.diagonal(Lh, axis1=-2, axis2=-1).real).sum(axis=-1)
    tr = np.einsum("ftij,ftji->ft", Xe, np.linalg.inv(Xh)).real
    return float((tr - ldx + ldh - M).sum())


def update_once(X, Tb, V, H, normalize=True, eps=EPS):
    Tb = update_basis(X, Tb, V, H, eps)
    V = update_activation(X, Tb, V, H, eps)
    H = update_spatial(X, Tb, V, H, normalize, eps)
    return Tb, V, H


def init_spatial(M, F, K):
    return np.tile(np.eye(M, dtype=np.complex128), (F, K, 1, 1))


def run(X, T0, V0, n_iter, normalize=True, eps=EPS, H0=None, step=update_once):
    """({iteration: (H, Tb, V)} for every iteration, [loss after every iteration])."""
    F, T, M, _ = X.shape
    Tb, V = np.array(T0), np.array(V0)
    H = init_spatial(M, F, Tb.shape[1]) if H0 is None else np.array(H0)
    states, losses = {}, []
    for it in range(1, n_iter + 1):
        Tb, V, H = step(X, Tb, V, H, normalize, eps)
        states[it] = (H, Tb, V)
        losses.append(loss(X, Tb, V, H, eps))
    return states, losses


def target(M, F, T, smooth, seed):
    """A positive-definite target (F,T,M,M): the mean of `smooth` >= M consecutive outer products of a seeded
    convolutive mixture of M sources (T + smooth - 1 frames of it)."""
    rng = np.random.default_rng(seed)
    n = T + smooth - 1
    src = (rng.standard_normal((M, F, n)) + 1j * rng.standard_normal((M, F, n))) * (0.2 + rng.random((M, 1, n)))
    mix = rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))
    x = np.einsum("fmn,nft->ftm", mix, src)  # (F, n, M)
    outer = x[..., :, None] * x[..., None, :].conj()
    X = sum(outer[:, s:s + T] for s in range(smooth)) / smooth
    return (X + X.conj().swapaxes(-1, -2)) / 2


def fixtures(directory):
    import glob
    import os
    return sorted(glob.glob(os.path.join(directory, "covnmf_*.npz")))


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
