"""Independent NumPy restatement of Sawada's MNMF (MultichannelISNMF, reference src/bss/mnmf.py:115-617) in the closed
forms the GPU kernels use.  Nothing here is copied from the reference; tests/golden/mnmf pins
it to the reference's recorded output.

With X^ = sum_k T[f,k] V[k,t] sum_n Z[n,k] H[f,n] and P = (X^ + eps I)^-1, the reference's P (x x^H) P has rank one,
so its traces reduce to  a_n = y^H H_n y  (y = P x)  and  b_n = tr(P H_n).  The spatial update solves H A H = B by the
matrix geometric mean (Cholesky of A, one Hermitian eigendecomposition), with H = 0 where A is exactly 0.  The loss is
the exact value of the reference's log-det divergence (see `loss`).  Every function works chunk by chunk over f, so
full-size problems run in bounded memory.

Shapes: X (M,F,T) complex, T (F,K) basis, V (K,T) activation, Z (N,K) latent, H (F,N,M,M) complex spatial.
"""
import numpy as np

EPS = 1e-12
CHUNK = 16  # bins per chunk


def _herm(A):
    return (A + A.conj().swapaxes(-1, -2)) / 2


def _chunks(F):
    for f0 in range(0, F, CHUNK):
        yield slice(f0, min(F, f0 + CHUNK))


def _eval(X, Tb, V, Z, H, eps):
    """One chunk of bins: lam (N,f,T), P (f,T,M,M), y (f,T,M), a and b (N,f,T)."""
    M = X.shape[0]
    lam = np.einsum("nk,fk,kt->nft", Z, Tb, V)
    Xh = np.einsum("nft,fnij->ftij", lam, H)
    P = np.linalg.inv(Xh + eps * np.eye(M))
    x = X.transpose(1, 2, 0)
    y = np.einsum("ftij,ftj->fti", P, x)
    a = np.einsum("fti,fnij,ftj->nft", y.conj(), H, y).real
    b = np.einsum("ftij,fnji->nft", P, H).real
    return lam, P, y, a, b


def update_basis(X, Tb, V, Z, H, eps=EPS):
    num = np.empty_like(Tb)
    den = np.empty_like(Tb)
    for s in _chunks(Tb.shape[0]):
        _, _, _, a, b = _eval(X[:, s], Tb[s], V, Z, H[s], eps)
        num[s] = np.einsum("nk,kt,nft->fk", Z, V, a)
        den[s] = np.einsum("nk,kt,nft->fk", Z, V, b)
    den[den < eps] = eps
    return Tb * np.sqrt(num / den)


def update_activation(X, Tb, V, Z, H, eps=EPS):
    num = np.zeros_like(V)
    den = np.zeros_like(V)
    for s in _chunks(Tb.shape[0]):
        _, _, _, a, b = _eval(X[:, s], Tb[s], V, Z, H[s], eps)
        num += np.einsum("nk,fk,nft->kt", Z, Tb[s], a)
        den += np.einsum("nk,fk,nft->kt", Z, Tb[s], b)
    den[den < eps] = eps
    return V * np.sqrt(num / den)


def update_latent(X, Tb, V, Z, H, eps=EPS):
    num = np.zeros_like(Z)
    den = np.zeros_like(Z)
    for s in _chunks(Tb.shape[0]):
        _, _, _, a, b = _eval(X[:, s], Tb[s], V, Z, H[s], eps)
        num += np.einsum("fk,kt,nft->nk", Tb[s], V, a)
        den += np.einsum("fk,kt,nft->nk", Tb[s], V, b)
    den[den < eps] = eps
    Z = Z * np.sqrt(num / den)
    Zsum = Z.sum(axis=0)
    Zsum[Zsum < eps] = eps
    return Z / Zsum


def riccati(A, B):
    """The positive-definite solution of H A H = B (A positive definite, B positive semi-definite): the geometric mean
    L^-H (L^H B L)^(1/2) L^-1 with A = L L^H.  Where A is exactly zero, H = 0."""
    A, B = np.asarray(A), np.asarray(B)
    zero = np.all(A == 0, axis=(-2, -1))
    M = A.shape[-1]
    A = np.where(zero[..., None, None], np.eye(M), A)
    L = np.linalg.cholesky(A)
    C = _herm(L.conj().swapaxes(-1, -2) @ B @ L)
    w, U = np.linalg.eigh(C)
    S = (U * np.sqrt(np.maximum(w, 0))[..., None, :]) @ U.conj().swapaxes(-1, -2)
    Li = np.linalg.inv(L)
    H = _herm(Li.conj().swapaxes(-1, -2) @ S @ Li)
    return np.where(zero[..., None, None], 0, H)


def update_spatial(X, Tb, V, Z, H, normalize=True, eps=EPS):
    M = X.shape[0]
    Hn = np.empty_like(H)
    for s in _chunks(Tb.shape[0]):
        lam, P, y, _, _ = _eval(X[:, s], Tb[s], V, Z, H[s], eps)
        A = np.einsum("nft,ftij->fnij", lam, P)
        C = np.einsum("nft,fti,ftj->fnij", lam, y, y.conj())
        Bm = H[s] @ C @ H[s]
        Hs = riccati(A, Bm) + eps * np.eye(M)
        if normalize:
            Hs = Hs / np.trace(Hs, axis1=2, axis2=3)[..., None, None]
        Hn[s] = Hs
    return Hn


def loss(X, Tb, V, Z, H, eps=EPS):
    """The exact value of the reference's logdet_divergence(to_PSD(X^) + eps I, to_PSD(x x^H) + eps I), summed: with
    c = eps |x|^2 + eps and X' = X^ + (eps tr X^ + eps) I, per (f, t)
        x^H X'^-1 x + c tr X'^-1 - (M - 1) ln c - ln(|x|^2 + c) + ln det X' - M."""
    M = X.shape[0]
    total = 0.0
    for s in _chunks(Tb.shape[0]):
        lam = np.einsum("nk,fk,kt->nft", Z, Tb[s], V)
        Xh = np.einsum("nft,fnij->ftij", lam, H[s])
        tr = np.trace(Xh, axis1=2, axis2=3).real
        Xp = Xh + (eps * tr + eps)[..., None, None] * np.eye(M)
        Pi = np.linalg.inv(Xp)
        x = X[:, s].transpose(1, 2, 0)
        n2 = np.sum(np.abs(x) ** 2, axis=-1)
        c = eps * n2 + eps
        quad = np.einsum("fti,ftij,ftj->ft", x.conj(), Pi, x).real
        _, ld = np.linalg.slogdet(Xp)
        term = quad + c * np.trace(Pi, axis1=2, axis2=3).real - (M - 1) * np.log(c) - np.log(n2 + c) + ld - M
        total += term.sum()
    return total


def separate(X, Tb, V, Z, H, reference_id=0, eps=EPS):
    """(N, F, T): lam_n (H_n P x)[reference_id]."""
    N, F, T = Z.shape[0], X.shape[1], X.shape[2]
    Y = np.empty((N, F, T), dtype=np.complex128)
    for s in _chunks(F):
        lam, _, y, _, _ = _eval(X[:, s], Tb[s], V, Z, H[s], eps)
        Y[:, s] = lam * np.einsum("fnj,ftj->nft", H[s][:, :, reference_id, :], y)
    return Y


def update_once(X, Tb, V, Z, H, normalize=True, eps=EPS):
    Tb = update_basis(X, Tb, V, Z, H, eps)
    V = update_activation(X, Tb, V, Z, H, eps)
    Z = update_latent(X, Tb, V, Z, H, eps)
    H = update_spatial(X, Tb, V, Z, H, normalize, eps)
    return Tb, V, Z, H


def init_spatial(M, N, F):
    return np.tile(np.eye(M, dtype=np.complex128), (F, N, 1, 1))


def run(X, T0, V0, Z0, n_iter, normalize=True, eps=EPS, record=None, with_loss=True):
    """The reference's loop from (T0, V0, Z0) and H = I.  record(i, state) after every iteration (and i = 0)."""
    M, F, _ = X.shape
    Tb, V, Z, H = T0.copy(), V0.copy(), Z0.copy(), init_spatial(M, Z0.shape[0], F)
    losses = [loss(X, Tb, V, Z, H, eps)] if with_loss else []
    if record:
        record(0, dict(basis=Tb, activation=V, latent=Z, spatial=H))
    for i in range(n_iter):
        Tb, V, Z, H = update_once(X, Tb, V, Z, H, normalize, eps)
        if with_loss:
            losses.append(loss(X, Tb, V, Z, H, eps))
        if record:
            record(i + 1, dict(basis=Tb, activation=V, latent=Z, spatial=H))
    return separate(X, Tb, V, Z, H, 0, eps), losses, dict(basis=Tb, activation=V, latent=Z, spatial=H)
