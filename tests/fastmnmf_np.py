"""NumPy restatement of FastMultichannelISNMF (reference: src/bss/mnmf.py:637-946), written from the update rules and
streamed bin by bin so that the full-size case (M = N = 4, F = 1025, T = 4096) fits in host memory.

State, as the model class holds it:  X (M,F,T) complex, W (N,F,K) basis, H (N,K,T) activation, g (N,F,M)
spatial_covariance, Q (F,M,M) diagonalizer.  x~[f,t,m] = |(Q_f x_ft)[m]|^2,  Lambda_n = W_n H_n,
R[f,t,m] = sum_n Lambda_n[f,t] g[n,f,m].

The GPU tests compare the HIP path with this module; tests/test_fastmnmf_cpu.py pins it to the reference's own output
(tests/golden/fastmnmf/*.npz).
"""
import numpy as np

EPS = 1e-12
THRESHOLD = 1e12


def initial_state(M, N, F):
    """Q = I and g = 1e-2 with g[m % N, :, m] = 1 (mnmf.py:662-665)."""
    Q = np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1))
    g = np.full((N, F, M), 1e-2)
    for m in range(M):
        g[m % N, :, m] = 1
    return Q, g


def _project(Q_f, X_f):
    """x~ of one bin, (T, M): |Q x|^2 (mnmf.py:785-786)."""
    return np.abs(Q_f @ X_f).T ** 2


def _mix(W_f, H, g_f):
    """Lambda (N, T) and R (T, M) of one bin (mnmf.py:791-793)."""
    lam = np.einsum("nk,nkt->nt", W_f, H)
    return lam, lam.T @ g_f


def update_nmf(X, W, H, g, Q, eps=EPS):
    """mnmf.py:775-815: the basis half per bin (reduce over t), then the activation half (reduce over f) with the new
    basis.  Returns new (W, H)."""
    N, F, K = W.shape
    W = W.copy()
    for f in range(F):
        xt = _project(Q[f], X[:, f])
        _, R = _mix(W[:, f], H, g[:, f])
        R = np.maximum(R, eps)
        gxR = g[:, f] @ (xt / R ** 2).T  # (N, T)
        gR = g[:, f] @ (1 / R).T
        num = np.einsum("nkt,nt->nk", H, gxR)
        den = np.maximum(np.einsum("nkt,nt->nk", H, gR), eps)
        W[:, f] = W[:, f] * np.sqrt(num / den)
    num = np.zeros_like(H)
    den = np.zeros_like(H)
    for f in range(F):
        xt = _project(Q[f], X[:, f])
        _, R = _mix(W[:, f], H, g[:, f])
        R = np.maximum(R, eps)
        gxR = g[:, f] @ (xt / R ** 2).T
        gR = g[:, f] @ (1 / R).T
        num += W[:, f, :, None] * gxR[:, None, :]
        den += W[:, f, :, None] * gR[:, None, :]
    H = H * np.sqrt(num / np.maximum(den, eps))
    return W, H


def update_scm(X, W, H, g, Q, eps=EPS):
    """mnmf.py:817-846.  Returns the new g."""
    g = g.copy()
    for f in range(W.shape[1]):
        xt = _project(Q[f], X[:, f])
        lam, R = _mix(W[:, f], H, g[:, f])
        R = np.maximum(R, eps)
        A = lam @ (xt / R ** 2)  # (N, M)
        B = np.maximum(lam @ (1 / R), eps)
        g[:, f] = g[:, f] * np.sqrt(A / B)
    return g


def update_diagonalizer(X, W, H, g, Q, eps=EPS, threshold=THRESHOLD):
    """mnmf.py:848-888: V_m = mean_t x x^H / max(R_m, eps); for every channel m, q = (Q V_m)^{-1} e_m and
    Q[m] = conj(q) / max(sqrt(q^H V_m q), eps) unless cond(Q V_m) >= threshold."""
    M = X.shape[0]
    T = X.shape[2]
    Q = Q.copy()
    for f in range(W.shape[1]):
        X_f = X[:, f]
        _, R = _mix(W[:, f], H, g[:, f])
        R = np.maximum(R, eps)
        Qf = Q[f]
        for m in range(M):
            V = (X_f / R[:, m]) @ X_f.conj().T / T
            QV = Qf @ V
            if np.linalg.cond(QV) < threshold:
                q = np.linalg.solve(QV, np.eye(M)[m])
                den = np.sqrt(q.conj() @ V @ q)  # complex, as the reference keeps it
                if den < eps:  # NumPy orders complex numbers by their real part first
                    den = eps
                Qf[m] = q.conj() / den
        Q[f] = Qf
    return Q


def normalize_power(W, H, g, Q, eps=EPS):
    """mnmf.py:748-769.  Returns new (W, H, g, Q)."""
    QQ = np.real((Q * Q.conj()).sum(axis=2).mean(axis=1))
    QQ = np.maximum(QQ, eps)
    Q = Q / np.sqrt(QQ)[:, None, None]
    g = g / QQ[None, :, None]
    gs = np.maximum(g.sum(axis=2), eps)
    g = g / gs[:, :, None]
    W = W * gs[:, :, None]
    Ws = np.maximum(W.sum(axis=1), eps)
    W = W / Ws[:, None]
    H = H * Ws[:, :, None]
    return W, H, g, Q


def loss(X, W, H, g, Q, eps=EPS):
    """mnmf.py:890-917: sum (x~ + eps) / (R + eps) + log(R + eps) - T sum_f log|det(Q Q^T)|."""
    T = X.shape[2]
    total = 0.0
    for f in range(W.shape[1]):
        xt = _project(Q[f], X[:, f]) + eps
        _, R = _mix(W[:, f], H, g[:, f])
        R = R + eps
        total += np.sum(xt / R + np.log(R))
    detQQ = np.abs(np.linalg.det(Q @ Q.transpose(0, 2, 1)))
    return total - T * np.sum(np.log(detQQ))


def separate(X, W, H, g, Q, reference_id=0, eps=EPS):
    """mnmf.py:919-946: (N, F, T) complex, x_hat[:, reference_id]."""
    N, F, _ = W.shape
    Y = np.empty((N, F, X.shape[2]), dtype=np.complex128)
    Qinv = np.linalg.inv(Q)
    for f in range(F):
        QX = Q[f] @ X[:, f]  # (M, T)
        lam, R = _mix(W[:, f], H, g[:, f])
        R = np.maximum(R, eps)
        LG = lam[:, :, None] * g[:, f][:, None, :]  # (N, T, M)
        Y[:, f] = np.einsum("m,ntm->nt", Qinv[f, reference_id], QX.T[None] * (LG / R[None]))
    return Y


def expand_partitioned(Z, W, H):
    """Partitioning function (mnmf.py:822-826): per-source basis Z[n,k] W[f,k] and shared activation."""
    N = Z.shape[0]
    return Z[:, None, :] * W[None], np.broadcast_to(H, (N,) + H.shape).copy()


def step(X, W, H, g, Q, normalize="power", eps=EPS, threshold=THRESHOLD):
    """update_once (mnmf.py:737-773)."""
    W, H = update_nmf(X, W, H, g, Q, eps)
    g = update_scm(X, W, H, g, Q, eps)
    Q = update_diagonalizer(X, W, H, g, Q, eps, threshold)
    if normalize:
        if normalize != "power":
            raise ValueError("Not support normalization based on {}. Choose 'power'".format(normalize))
        W, H, g, Q = normalize_power(W, H, g, Q, eps)
    return W, H, g, Q


def run(X, W0, H0, n_iter, N=None, normalize="power", reference_id=0, eps=EPS, threshold=THRESHOLD, record=None):
    """The loop of __call__ (mnmf.py:691-722) from basis W0 / activation H0.  record(i, state dict) after every
    iteration.  Returns (output, losses, final state)."""
    M, F, _ = X.shape
    N = W0.shape[0] if N is None else N
    Q, g = initial_state(M, N, F)
    W, H = W0.copy(), H0.copy()
    losses = [loss(X, W, H, g, Q, eps)]
    for i in range(n_iter):
        W, H, g, Q = step(X, W, H, g, Q, normalize, eps, threshold)
        losses.append(loss(X, W, H, g, Q, eps))
        if record is not None:
            record(i + 1, dict(basis=W, activation=H, spatial_covariance=g, diagonalizer=Q))
    state = dict(basis=W, activation=H, spatial_covariance=g, diagonalizer=Q)
    return separate(X, W, H, g, Q, reference_id, eps), losses, state
