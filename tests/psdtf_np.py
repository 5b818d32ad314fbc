"""NumPy restatement of LDPSDTF (log-det positive semidefinite tensor factorisation), stage by stage as the HIP kernels
run it.

The model is Y_t = sum_k H[k,t] V_k for a target of T real symmetric M x M matrices X_t, with K symmetric bases V_k and
an activation H (K, T).  psd(A) = (A + A^T) / 2 - min(lambda_min, 0) I + eps tr(A) I follows every constructed matrix.
One update:

    per frame   Y = psd(sum_k H V_k),  Yi = psd(Y^-1),  Z = psd(Yi X Yi)
    per basis   P = psd(sum_t H Yi),  Q = psd(sum_t H Z),  L = chol(Q),  C = psd(L^T V P V L),
                S = psd(C^1/2)^-1 (eigenvalues clamped at 0 before the root),  V <- psd(V L S L^T V)
    per frame   Y, Yi again from the new V;  num = tr(Yi V_k Yi X), den = tr(Yi V_k);
                H <- H sqrt(max(num, 0) / max(den, eps))
    normalise   V_k /= tr V_k,  H[k,:] *= tr V_k

and the loss is sum_t tr(X Y^-1) - (logdet X - logdet Y) - M with Y = psd(sum_k H V_k) and both sets of eigenvalues
floored at eps.  Arrays here are matrix-contiguous: X (T, M, M), V (K, M, M), H (K, T); `kmm` / `mmk` convert a basis
from and to the public (M, M, K) shape.  Every function takes `la`, the linear algebra it runs on: LAPACK (numpy.linalg) or
KERNEL, NumPy models of the kernels' own algorithms (Cholesky inverse, Jacobi in the kernels' rotation order and sweep
rule, the Cholesky shortcut of psd), so that the method difference can be measured without a GPU.  Written from the
equations above; nothing is taken from another code base.
"""
import glob
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "psdtf")
SNAP_ITERS = (1, 2, 4, 5, 19, 20)
START_ITERS = (0, 1, 4, 19)  # the recorded states whose successor is recorded too
METRICS = ("V", "H", "loss")
N_ITER = 20
JACOBI_SWEEPS = 30


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "psdtf_*.npz")))


def tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as fh:
        return json.load(fh)


def state(fx, it):
    """(basis (M, M, K), activation (K, T)) of a fixture after `it` iterations (0: the state the first update starts
    from, that is the draws after the reference's reset)."""
    if it == 0:
        return fx["V0"].copy(), fx["H0"].copy()
    return fx["basis_%d" % it].copy(), fx["activation_%d" % it].copy()


def kmm(V):
    return np.ascontiguousarray(np.transpose(V, (2, 0, 1)))


def mmk(V):
    return np.ascontiguousarray(np.transpose(V, (1, 2, 0)))


def frames_first(X):
    """target (M, M, T) -> (T, M, M)"""
    return np.ascontiguousarray(np.transpose(X, (2, 0, 1)))


# ---------------------------------------------------------------------------------------------- the kernels' algorithms
def chol_lower(A, floor=0.0):
    """Left-looking Cholesky of (N, n, n); a pivot at or below `floor` (relative: an (N,) array is allowed) is replaced by 1
    and reported.  Returns (L, ok (N,))."""
    A = np.array(A, dtype=np.float64)
    N, n, _ = A.shape
    ok = np.ones(N, dtype=bool)
    floor = np.broadcast_to(np.asarray(floor, dtype=np.float64), (N,))
    for j in range(n):
        A[:, j:, j] -= np.einsum("nik,nk->ni", A[:, j:, :j], A[:, j, :j])
        d = A[:, j, j].copy()
        bad = ~(d > floor)
        ok &= ~bad
        d[bad] = 1.0
        r = np.sqrt(d)
        A[:, j + 1:, j] /= r[:, None]
        A[:, j, j] = r
    return np.tril(A), ok


def tri_inv(L):
    """Inverse of lower triangles (N, n, n) by forward substitution, column by column."""
    N, n, _ = L.shape
    Li = np.zeros_like(L)
    idx = np.arange(n)
    Li[:, idx, idx] = 1.0 / L[:, idx, idx]
    for i in range(1, n):
        acc = np.einsum("nk,nkj->nj", L[:, i, :i], Li[:, :i, :i])
        Li[:, i, :i] = -acc / L[:, i, i][:, None]
    return Li


def chol_inverse(A):
    """A^-1 = Li^T Li of positive definite (N, n, n); numpy.linalg.LinAlgError otherwise."""
    L, ok = chol_lower(A)
    if not ok.all():
        raise np.linalg.LinAlgError("Matrix is not positive definite")
    Li = tri_inv(L)
    return np.transpose(Li, (0, 2, 1)) @ Li


def jacobi_pairs(m, r):
    """The m / 2 disjoint pairs of step r of a sweep (round-robin: the last index stays, the others turn)."""
    t = np.arange(1, m // 2)
    a = np.concatenate([[r], (r + t) % (m - 1)])
    b = np.concatenate([[m - 1], (r - t + (m - 1)) % (m - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_eigh(A):
    """(w (N, n), vectors (N, n, n) as columns, converged (N,)) of symmetric (N, n, n): parallel-order Jacobi, all pairs of a
    step at once, a sweep test on the off-diagonal mass before every sweep (stop at 1e-32 of the total), at most
    JACOBI_SWEEPS sweeps.  An odd n is padded with a zero row and column."""
    A = np.array(A, dtype=np.float64)
    N, n, _ = A.shape
    m = (n + 1) & ~1
    W = np.zeros((N, m, m))
    W[:, :n, :n] = A
    Vv = np.tile(np.eye(m), (N, 1, 1))
    conv = np.zeros(N, dtype=bool)
    idx = np.arange(n)
    for sweep in range(JACOBI_SWEEPS + 1):
        low = np.tril(W[:, :n, :n], -1)
        off = np.sum(low * low, axis=(1, 2))
        dg = np.sum(W[:, idx, idx] ** 2, axis=1)
        conv = off <= 1e-32 * (dg + 2.0 * off)
        act = ~conv & ~np.isnan(off)
        if not act.any() or sweep == JACOBI_SWEEPS:
            break
        for r in range(m - 1):
            p, q = jacobi_pairs(m, r)
            apq = np.where(act[:, None], W[:, p, q], 0.0)
            app, aqq = W[:, p, p], W[:, q, q]
            nz = apq != 0.0
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                th = (aqq - app) / (2 * np.where(nz, apq, 1.0))
                t = np.where(nz, np.copysign(1.0, th) / (np.abs(th) + np.sqrt(th * th + 1)), 0.0)
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            J = np.zeros((N, m, m))
            J[:, p, p] = c
            J[:, q, q] = c
            J[:, p, q] = s
            J[:, q, p] = -s
            W = np.transpose(J, (0, 2, 1)) @ W @ J
            W = (W + np.transpose(W, (0, 2, 1))) / 2
            W[:, p, p] = app - t * apq
            W[:, q, q] = aqq + t * apq
            W[:, p, q] = np.where(nz, 0.0, W[:, p, q])
            W[:, q, p] = np.where(nz, 0.0, W[:, q, p])
            Vv = Vv @ J
    return W[:, idx, idx], Vv[:, :n, :n], conv


class LAPACK:
    """numpy.linalg"""
    inv = staticmethod(np.linalg.inv)
    eigh = staticmethod(np.linalg.eigh)
    eigvalsh = staticmethod(np.linalg.eigvalsh)

    @staticmethod
    def min_eig(A):
        return np.min(np.linalg.eigvalsh(A), axis=-1)


class KERNEL:
    """the kernels' algorithms"""
    inv = staticmethod(chol_inverse)

    @staticmethod
    def eigh(A):
        w, v, conv = jacobi_eigh(A)
        assert conv.all()
        return w, v

    @staticmethod
    def eigvalsh(A):
        return KERNEL.eigh(A)[0]

    @staticmethod
    def min_eig(A):
        """0 where a Cholesky factorisation with every pivot above 2^-40 of the largest diagonal entry proves the matrix
        positive definite (any non-negative value gives psd's delta = 0), the smallest Jacobi eigenvalue elsewhere."""
        n = A.shape[-1]
        idx = np.arange(n)
        mx = np.maximum(np.max(A[:, idx, idx], axis=1), 0.0)
        _, ok = chol_lower(A, floor=np.ldexp(mx, -40))
        out = np.zeros(A.shape[0])
        if not ok.all():
            out[~ok] = np.min(KERNEL.eigvalsh(A[~ok]), axis=-1)
        return out


# ---------------------------------------------------------------------------------------------- the stages
def to_psd(A, eps, la=LAPACK):
    """psd() of (..., n, n)."""
    A = np.asarray(A, dtype=np.float64)
    shape = A.shape
    A = A.reshape((-1,) + shape[-2:])
    A = (A + np.transpose(A, (0, 2, 1))) / 2
    delta = np.minimum(la.min_eig(A), 0.0)
    trace = np.trace(A, axis1=1, axis2=2)
    eye = np.eye(shape[-1])
    return (A - delta[:, None, None] * eye + eps * trace[:, None, None] * eye).reshape(shape)


def reconstruct(V, H):
    """(T, M, M): sum_k H[k,t] V_k, without psd()."""
    return np.einsum("kt,kij->tij", H, V)


def model_inverse(V, H, eps, la=LAPACK):
    """Yi = psd(psd(sum_k H V_k)^-1), (T, M, M)."""
    return to_psd(la.inv(to_psd(reconstruct(V, H), eps, la)), eps, la)


def update_basis(X, V, H, eps, la=LAPACK):
    Yi = model_inverse(V, H, eps, la)
    Z = to_psd(Yi @ X @ Yi, eps, la)
    P = to_psd(np.einsum("kt,tij->kij", H, Yi), eps, la)
    Q = to_psd(np.einsum("kt,tij->kij", H, Z), eps, la)
    if la is LAPACK:
        L = np.linalg.cholesky(Q)
    else:
        L, ok = chol_lower(Q)
        if not ok.all():
            raise np.linalg.LinAlgError("Matrix is not positive definite")
    Lt = np.transpose(L, (0, 2, 1))
    G = V @ L
    C = to_psd(np.transpose(G, (0, 2, 1)) @ P @ G, eps, la)
    w, U = la.eigh(C)
    root = (U * np.sqrt(np.maximum(w, 0.0))[:, None, :]) @ np.transpose(U, (0, 2, 1))
    S = la.inv(to_psd(root, eps, la))
    return to_psd(V @ L @ S @ Lt @ V, eps, la)


def update_activation(X, V, H, eps, la=LAPACK):
    Yi = model_inverse(V, H, eps, la)
    W = Yi @ X @ Yi
    num = np.einsum("kij,tji->kt", V, W)
    den = np.einsum("kij,tji->kt", V, Yi)
    return H * np.sqrt(np.maximum(num, 0.0) / np.maximum(den, eps))


def normalize(V, H):
    tr = np.trace(V, axis1=1, axis2=2)
    return V / tr[:, None, None], H * tr[:, None]


def update(X, V, H, eps, norm=True, la=LAPACK):
    """One update; returns new (V, H) and leaves its inputs alone."""
    V = update_basis(X, V, H, eps, la)
    H = update_activation(X, V, H, eps, la)
    if norm:
        V, H = normalize(V, H)
    return V, H


def loss_frames(X, V, H, eps, la=LAPACK):
    Y = to_psd(reconstruct(V, H), eps, la)
    tr = np.einsum("tij,tji->t", X, la.inv(Y))
    ldx = np.sum(np.log(np.maximum(la.eigvalsh((X + np.transpose(X, (0, 2, 1))) / 2), eps)), axis=-1)
    ldy = np.sum(np.log(np.maximum(la.eigvalsh(Y), eps)), axis=-1)
    return tr - (ldx - ldy) - X.shape[-1]


def loss(X, V, H, eps, la=LAPACK):
    return float(np.sum(loss_frames(X, V, H, eps, la)))


def run(X, V, H, eps, n, norm=True, la=LAPACK):
    """The models and losses after 1..n updates."""
    states, losses = [], []
    for _ in range(n):
        V, H = update(X, V, H, eps, norm, la)
        states.append((V, H))
        losses.append(loss(X, V, H, eps, la))
    return states, losses


# ---------------------------------------------------------------------------------------------- metrics
def v_metric(a, b):
    """Largest max|a - b| / max|b| over the bases (K, M, M): off-diagonal entries pass through zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.max(np.abs(a - b), axis=(-2, -1)) / np.max(np.abs(b), axis=(-2, -1))))


def h_metric(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def loss_metric(a, b, n_bins, n_frames):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + n_bins * n_frames)))


def mat_metric(a, b):
    """max|a - b| / max|b| per matrix of (N, n, n), the largest."""
    return v_metric(a, b)


def one_ulp(a, rng):
    """Every entry moved to a neighbouring double, direction drawn per entry."""
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def sym_ulp(V, rng):
    """one_ulp of symmetric matrices (K, M, M) that keeps them symmetric."""
    U = np.triu(one_ulp(V, rng))
    return U + np.transpose(np.triu(U, 1), (0, 2, 1))


def synthetic(M, T, K, seed):
    """A target (T, M, M) and a model for shapes the fixtures do not cover (the fixtures' recipe)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((2, M, M))
    W = A @ np.transpose(A, (0, 2, 1)) / M
    x = rng.standard_normal((T, M, 2))
    X = np.einsum("kt,kij->tij", rng.random((2, T)) + 0.1, W) + 0.05 * x @ np.transpose(x, (0, 2, 1))
    d = rng.random((K, M))
    V = d[:, :, None] * np.eye(M)
    return X, V, rng.random((K, T))


def psd_cases(n, seed):
    """Seeded symmetric matrices for the to_psd tests: (name, (N, n, n)) for positive definite matrices, matrices with one
    well-separated negative eigenvalue, and exactly diagonal ones (both signs)."""
    rng = np.random.default_rng(seed)
    N = 3
    q = np.linalg.qr(rng.standard_normal((N, n, n)))[0]
    lam = 0.5 + rng.random((N, n))
    pd = (q * lam[:, None, :]) @ np.transpose(q, (0, 2, 1))
    lam2 = lam.copy()
    lam2[:, 0] = -0.75
    ind = (q * lam2[:, None, :]) @ np.transpose(q, (0, 2, 1))
    dg = np.zeros((N, n, n))
    idx = np.arange(n)
    dg[:, idx, idx] = lam
    dg[1, 0, 0] = -0.25
    return (("definite", pd), ("indefinite", ind), ("diagonal", dg))
