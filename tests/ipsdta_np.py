"""NumPy restatement of GaussIPSDTA (Kondo's block-diagonal independent positive semidefinite tensor analysis), stage by
stage as the HIP kernels run it.

The n_bins bins are cut into n_blocks blocks: the first nlow = n_blocks - n_bins % n_blocks of nn = n_bins // n_blocks bins,
the others of nn + 1.  Source n has, per block, K Hermitian nb x nb bases U_k and an activation H (K, T); with y = W x the
block's output and psd(A) = (A + A^H)/2 - min(lambda_min, 0) I + eps tr(A) I after every constructed matrix:

    R = psd(sum_k H U_k),  Ri = psd(R^-1)                                       per (source, frame, block)
    basis       S_k = sum_t H Ri (y y^H + eps I) Ri,  T_k = sum_t H Ri,  s = psd(sqrt S_k),
                U_k <- psd(U s psd(psd(sqrt(psd(s U T U s)))^-1) s U)
    activation  num = sum_blocks Re tr(Ri U_k Ri psd(y y^H + eps I)),  den = sum_blocks Re tr(Ri U_k),
                H <- H sqrt(max(num, 0) / max(den, eps))
    normalise   U_k /= tr U_k (all blocks),  H[k,:] *= tr U_k
    spatial     Q[n,f] = psd(mean_t (Ri)_ii(t) psd(x_f(t) x_f(t)^H)) once; per sweep, sources in order, positions i of a
                block in order: gamma = mean_t sum_{j != i} (Ri)_ji x_i conj(y_j), zeta = (W_f Q)^-1 e_n,
                zeta_hat = Q^-1 gamma, eta = zeta^H Q zeta, eta_hat = zeta^H Q zeta_hat, |eta| floored at eps,
                weight = 1/sqrt(eta) where |eta_hat| < eps, else (eta_hat / 2 eta)(1 - sqrt(1 + 4 eta / |eta_hat|^2)),
                row n of W_f <- conj(weight zeta - zeta_hat)
    loss        sum (y^H Ri y + sum log max(lambda(R), eps)) - 2 T sum_f sum log max(|lambda(W_f)|, eps)

State in the public layouts: X (M, F, T), W (F, M, M), H (N, K, T), basis either (N, n_blocks, nb, nb, K) or the tuple
(low, high) of two such arrays.  Internally a basis is a list of parts (N, K, n, nb, nb), one per block size.  Every stage
takes `la`, the linear algebra it runs on: LAPACK (numpy.linalg, and psd of the rank-one matrices by eigenvalues, as the
formulas say) or KERNEL, NumPy models of what the kernels do differently (Cholesky inverse, cyclic Jacobi with the kernels'
stopping rule, the Cholesky shortcut of psd, min(lambda_min, 0) = 0 for x x^H and y y^H + eps I, log|det W| from an LU).
Written from the equations above; nothing is taken from another code base.
"""
import glob
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ipsdta")
N_ITER = 10
SNAP_ITERS = (1, 2, 4, 5, 9, 10)
START_ITERS = (0, 1, 4, 9)  # the recorded states whose successor is recorded too
JACOBI_SWEEPS = 12


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "ipsdta_*.npz")))


def tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as fh:
        return json.load(fh)


# ---------------------------------------------------------------------------------------------- geometry and layouts
def geometry(F, n_blocks):
    """(nn, nlow, n_remains)"""
    nn, rem = F // n_blocks, F % n_blocks
    return nn, n_blocks - rem, rem


def part_ranges(F, n_blocks):
    """[(first bin, number of blocks, block size)] for the block sizes present"""
    nn, nlow, rem = geometry(F, n_blocks)
    out = []
    if nlow:
        out.append((0, nlow, nn))
    if rem:
        out.append((nlow * nn, rem, nn + 1))
    return out


def to_parts(basis):
    """public basis -> list of (N, K, n, nb, nb)"""
    arrs = basis if isinstance(basis, (tuple, list)) else (basis,)
    return [np.ascontiguousarray(np.transpose(a, (0, 4, 1, 2, 3))) for a in arrs]


def from_parts(parts, F, n_blocks):
    """list of (N, K, n, nb, nb) -> public basis (array without remains, tuple with)"""
    arrs = [np.ascontiguousarray(np.transpose(p, (0, 2, 3, 4, 1))) for p in parts]
    return arrs[0] if geometry(F, n_blocks)[2] == 0 else tuple(arrs)


def pack(basis):
    """public basis -> the kernels' (N, K, P): the blocks row-major, end to end"""
    parts = to_parts(basis)
    N, K = parts[0].shape[:2]
    return np.ascontiguousarray(np.concatenate([p.reshape(N, K, -1) for p in parts], axis=2))


def unpack(packed, F, n_blocks):
    N, K, _ = packed.shape
    parts, o = [], 0
    for _, n, nb in part_ranges(F, n_blocks):
        parts.append(packed[:, :, o:o + n * nb * nb].reshape(N, K, n, nb, nb))
        o += n * nb * nb
    return from_parts(parts, F, n_blocks)


def fixture_basis(fx, tag):
    if "Ul_%s" % tag in fx:
        return fx["Ul_%s" % tag].copy(), fx["Uh_%s" % tag].copy()
    return fx["U_%s" % tag].copy()


def state(fx, tag):
    """(W, basis, H) of a fixture at a recorded state: '0', 'src1', 'sw1_<s>', or an iteration number"""
    tag = str(tag)
    return fx["W_%s" % tag].copy(), fixture_basis(fx, tag), fx["H_%s" % tag].copy()


def dims(fx):
    M, F, T = fx["X"].shape
    return M, F, T, int(fx["n_basis"]), int(fx["n_blocks"]), int(fx["spatial_iteration"])


# ---------------------------------------------------------------------------------------------- the kernels' algorithms
def ct(A):
    return np.conj(np.swapaxes(A, -2, -1))


def jacobi_eigh(A):
    """(w (N, n), vectors (N, n, n) as columns) of Hermitian (N, n, n): cyclic Jacobi, pairs (p, q) row by row, the
    off-diagonal mass tested before every sweep (stop at 1e-32 of the total), at most JACOBI_SWEEPS sweeps."""
    C = np.array(A, dtype=np.complex128)
    N, n, _ = C.shape
    U = np.tile(np.eye(n, dtype=np.complex128), (N, 1, 1))
    active = np.ones(N, dtype=bool)
    idx = np.arange(n)
    for _ in range(JACOBI_SWEEPS):
        off = np.sum(np.abs(np.tril(C, -1)) ** 2, axis=(1, 2))
        tot = np.sum(C[:, idx, idx].real ** 2, axis=1)
        active &= off > 1e-32 * (tot + 2.0 * off)
        if not active.any():
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                a = C[:, p, q]
                g = np.abs(a)
                m = active & (g != 0.0)
                if not m.any():
                    continue
                gs = np.where(m, g, 1.0)
                e = a / gs
                theta = (C[:, q, q].real - C[:, p, p].real) / (2.0 * gs)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                J = np.tile(np.eye(n, dtype=np.complex128), (N, 1, 1))
                J[m, p, p] = c[m]
                J[m, p, q] = s[m]
                J[m, q, p] = (-s * np.conj(e))[m]
                J[m, q, q] = (c * np.conj(e))[m]
                C = ct(J) @ C @ J
                U = U @ J
                C[m, p, q] = 0.0
                C[m, q, p] = 0.0
                C[m, p, p] = C[m, p, p].real
                C[m, q, q] = C[m, q, q].real
    return C[:, idx, idx].real.copy(), U


def chol_inverse(A):
    """A^-1 = Li^H Li of Hermitian positive definite (..., n, n); numpy.linalg.LinAlgError otherwise"""
    Li = np.linalg.inv(np.linalg.cholesky(A))
    return ct(Li) @ Li


def _flat(A):
    A = np.asarray(A)
    return A.reshape((-1,) + A.shape[-2:]), A.shape


class LAPACK:
    """numpy.linalg, and every psd() by its definition"""
    rank_one_shift = True
    inv = staticmethod(np.linalg.inv)
    eigvalsh = staticmethod(np.linalg.eigvalsh)

    @staticmethod
    def min_eig(A):
        return np.min(np.linalg.eigvalsh(A), axis=-1)

    @staticmethod
    def sqrtm(A):
        """eigenvalues clamped at 0 before the root"""
        w, v = np.linalg.eigh(A)
        return (v * np.sqrt(np.maximum(w, 0.0))[..., None, :]) @ np.linalg.inv(v)

    @staticmethod
    def logabsdet(W, eps):
        return np.sum(np.log(np.maximum(np.abs(np.linalg.eigvals(W)), eps)), axis=-1)


class KERNEL:
    """the kernels' algorithms"""
    rank_one_shift = False
    inv = staticmethod(chol_inverse)

    @staticmethod
    def eigvalsh(A):
        F, shape = _flat(A)
        return jacobi_eigh(F)[0].reshape(shape[:-1])

    @staticmethod
    def min_eig(A):
        """0 where a Cholesky factorisation with every pivot above 2^-40 of the largest diagonal entry proves the matrix
        positive definite (any non-negative value gives psd's delta = 0), the smallest Jacobi eigenvalue elsewhere"""
        F, shape = _flat(A)
        n = shape[-1]
        idx = np.arange(n)
        out = np.zeros(F.shape[0])
        mx = np.maximum(np.max(F[:, idx, idx].real, axis=1), 0.0)
        for i in range(F.shape[0]):
            try:
                L = np.linalg.cholesky(F[i])
                ok = bool(np.all(np.diagonal(L).real ** 2 > np.ldexp(mx[i], -40)))
            except np.linalg.LinAlgError:
                ok = False
            if not ok:
                out[i] = np.min(jacobi_eigh(F[i:i + 1])[0])
        return out.reshape(shape[:-2])

    @staticmethod
    def sqrtm(A):
        F, shape = _flat(A)
        w, v = jacobi_eigh(F)
        return ((v * np.sqrt(np.maximum(w, 0.0))[:, None, :]) @ ct(v)).reshape(shape)

    @staticmethod
    def logabsdet(W, eps):
        """log|det| (the kernel floors the pivots of its LU at eps, which matters for a singular W only)"""
        return np.linalg.slogdet(W)[1]


# ---------------------------------------------------------------------------------------------- the stages
def to_psd(A, eps, la=LAPACK, shift=True):
    """psd() of Hermitian (..., n, n); shift=False takes min(lambda_min, 0) as 0"""
    A = np.asarray(A, dtype=np.complex128)
    A = (A + ct(A)) / 2
    n = A.shape[-1]
    trace = np.trace(A, axis1=-2, axis2=-1).real
    eye = np.eye(n)
    if shift:
        delta = np.minimum(la.min_eig(A), 0.0)
        return A - delta[..., None, None] * eye + eps * trace[..., None, None] * eye
    return A + eps * trace[..., None, None] * eye


def separate(X, W):
    """Y (N, F, T) = W x"""
    return np.einsum("fnc,cft->nft", W, X)


def block_outputs(Y, f0, n, nb):
    """y of the blocks of one part: (N, T, n, nb)"""
    N, _, T = Y.shape
    return np.transpose(Y[:, f0:f0 + n * nb, :].reshape(N, n, nb, T), (0, 3, 1, 2))


def model_inverse(Up, H, eps, la=LAPACK, with_r=False):
    """Ri = psd(psd(sum_k H U_k)^-1) of one part: (N, T, n, nb, nb)"""
    R = to_psd(np.einsum("nkt,nkbij->ntbij", H, Up), eps, la)
    Ri = to_psd(la.inv(R), eps, la)
    return (Ri, R) if with_r else Ri


def update_basis(X, W, basis, H, eps, n_blocks, la=LAPACK):
    F = X.shape[1]
    Y = separate(X, W)
    out = []
    for (f0, n, nb), Up in zip(part_ranges(F, n_blocks), to_parts(basis)):
        Ri = model_inverse(Up, H, eps, la)
        y = block_outputs(Y, f0, n, nb)
        yy = y[..., :, None] * np.conj(y[..., None, :]) + eps * np.eye(nb)
        Z = Ri @ yy @ Ri
        S = np.einsum("nkt,ntbij->nkbij", H, Z)
        Tm = np.einsum("nkt,ntbij->nkbij", H, Ri)
        s = to_psd(la.sqrtm((S + ct(S)) / 2 if la is KERNEL else S), eps, la)
        C = to_psd(s @ Up @ Tm @ Up @ s, eps, la)
        Ci = to_psd(la.inv(to_psd(la.sqrtm(C), eps, la)), eps, la)
        out.append(to_psd(Up @ s @ Ci @ s @ Up, eps, la))
    return from_parts(out, F, n_blocks)


def update_activation(X, W, basis, H, eps, n_blocks, la=LAPACK, diag=None):
    F = X.shape[1]
    Y = separate(X, W)
    num, den = 0.0, 0.0
    for (f0, n, nb), Up in zip(part_ranges(F, n_blocks), to_parts(basis)):
        Ri = model_inverse(Up, H, eps, la)
        y = block_outputs(Y, f0, n, nb)
        yy = to_psd(y[..., :, None] * np.conj(y[..., None, :]) + eps * np.eye(nb), eps, la, shift=la.rank_one_shift)
        G = Ri @ yy @ Ri
        num = num + np.einsum("nkbij,ntbji->nkt", Up, G).real
        den = den + np.einsum("nkbij,ntbji->nkt", Up, Ri).real
    if diag is not None:
        diag["num_floored"] = bool(np.any(num < 0.0))
        diag["den_floored"] = bool(np.any(den < eps))
        diag["num_min"], diag["den_min"] = float(np.min(num)), float(np.min(den))
    return H * np.sqrt(np.maximum(num, 0.0) / np.maximum(den, eps))


def normalize(basis, H, F, n_blocks):
    parts = to_parts(basis)
    tr = sum(np.einsum("nkbii->nk", p).real for p in parts)
    return from_parts([p / tr[:, :, None, None, None] for p in parts], F, n_blocks), H * tr[:, :, None]


def update_source(X, W, basis, H, eps, n_blocks, norm=True, la=LAPACK):
    F = X.shape[1]
    basis = update_basis(X, W, basis, H, eps, n_blocks, la)
    H = update_activation(X, W, basis, H, eps, n_blocks, la)
    if norm:
        basis, H = normalize(basis, H, F, n_blocks)
    return basis, H


def inverse_parts(basis, H, eps, la=LAPACK):
    return [model_inverse(Up, H, eps, la) for Up in to_parts(basis)]


def q_matrices(X, Ri_parts, eps, n_blocks, la=LAPACK):
    """Q (N, F, M, M)"""
    M, F, T = X.shape
    xt = np.transpose(X, (1, 2, 0))  # (F, T, M)
    XX = to_psd(xt[..., :, None] * np.conj(xt[..., None, :]), eps, la, shift=la.rank_one_shift)
    w = np.empty((M, F, T))
    for (f0, n, nb), Ri in zip(part_ranges(F, n_blocks), Ri_parts):
        d = np.einsum("ntbii->ntbi", Ri).real  # (N, T, n, nb)
        w[:, f0:f0 + n * nb, :] = np.transpose(d, (0, 2, 3, 1)).reshape(M, n * nb, T)
    return to_psd(np.einsum("nft,ftcd->nfcd", w, XX) / T, eps, la)


def vcd_weight(eta, eta_hat, eps):
    """the step weight and the mask of the entries that took the IP branch"""
    eta = np.where(np.abs(eta) < eps, eps, eta).astype(np.complex128)
    ip = np.abs(eta_hat) < eps
    eh = np.where(ip, eps, eta_hat)
    weight = (eh / (2 * eta)) * (1 - np.sqrt(1 + 4 * eta / np.abs(eh) ** 2))
    return np.where(ip, 1 / np.sqrt(eta), weight), ip


def spatial_sweep(X, W, Ri_parts, Q, eps, n_blocks, diag=None):
    """one VCD sweep; returns the new W"""
    M, F, T = X.shape
    W = W.copy()
    for (f0, n, nb), Ri in zip(part_ranges(F, n_blocks), Ri_parts):
        Wp = W[f0:f0 + n * nb].reshape(n, nb, M, M).copy()
        Xp = X[:, f0:f0 + n * nb, :].reshape(M, n, nb, T)
        for src in range(M):
            e_n = np.zeros((n, M), dtype=np.complex128)
            e_n[:, src] = 1.0
            for i in range(nb):
                y = np.einsum("bjc,cbjt->bjt", Wp[:, :, src, :], Xp)
                r = np.transpose(Ri[src, :, :, :, i], (1, 2, 0))  # (n, nb [j], T)
                mask = np.ones(nb)
                mask[i] = 0.0
                s = np.einsum("j,bjt,bjt->bt", mask, r, np.conj(y))
                gamma = np.einsum("bt,cbt->bc", s, Xp[:, :, i, :]) / T
                Qi = Q[src, f0 + np.arange(n) * nb + i]
                zeta = np.linalg.solve(Wp[:, i] @ Qi, e_n[:, :, None])[:, :, 0]
                zeta_hat = np.linalg.solve(Qi, gamma[:, :, None])[:, :, 0]
                u = np.einsum("bc,bcd->bd", np.conj(zeta), Qi)
                eta, eta_hat = np.sum(u * zeta, axis=1), np.sum(u * zeta_hat, axis=1)
                weight, ip = vcd_weight(eta, eta_hat, eps)
                if diag is not None and nb > 1:
                    a = np.abs(eta_hat)  # exactly 0 for a diagonal model (gamma is exactly 0 there): far from the switch
                    diag["eta_hat_min"] = min(diag.get("eta_hat_min", np.inf), float(np.min(a[a > 0.0], initial=np.inf)))
                if diag is not None:
                    diag["eta_min"] = min(diag.get("eta_min", np.inf), float(np.min(np.abs(eta))))
                Wp[:, i, src, :] = np.conj(weight[:, None] * zeta - zeta_hat)
        W[f0:f0 + n * nb] = Wp.reshape(n * nb, M, M)
    return W


def update_spatial(X, W, basis, H, eps, n_blocks, n_sweeps, la=LAPACK, each=False, diag=None):
    """n_sweeps VCD sweeps on hoisted Ri and Q; each=True returns the list of W after every sweep"""
    Ri = inverse_parts(basis, H, eps, la)
    Q = q_matrices(X, Ri, eps, n_blocks, la)
    out = []
    for _ in range(n_sweeps):
        W = spatial_sweep(X, W, Ri, Q, eps, n_blocks, diag=diag)
        out.append(W)
    return out if each else W


def loss(X, W, basis, H, eps, n_blocks, la=LAPACK):
    M, F, T = X.shape
    Y = separate(X, W)
    total = 0.0
    for (f0, n, nb), Up in zip(part_ranges(F, n_blocks), to_parts(basis)):
        Ri, R = model_inverse(Up, H, eps, la, with_r=True)
        y = block_outputs(Y, f0, n, nb)
        total += np.sum(np.einsum("ntbi,ntbij,ntbj->ntb", np.conj(y), Ri, y).real)
        total += np.sum(np.log(np.maximum(la.eigvalsh(R), eps)))
    return float(total - 2 * T * np.sum(la.logabsdet(W, eps)))


def iterate(X, W, basis, H, eps, n_blocks, n_sweeps, norm=True, la=LAPACK):
    """one iteration: (W, basis, H, loss)"""
    basis, H = update_source(X, W, basis, H, eps, n_blocks, norm, la)
    W = update_spatial(X, W, basis, H, eps, n_blocks, n_sweeps, la)
    return W, basis, H, loss(X, W, basis, H, eps, n_blocks, la)


def projection_back_output(X, W, reference_id=0):
    """Y scaled per (source, bin) by x_ref Y^H (Y Y^H)^-1"""
    Y = separate(X, W)
    Yf = np.transpose(Y, (1, 0, 2))  # (F, N, T)
    G = Yf @ ct(Yf)
    scale = (X[reference_id][:, None, :] @ ct(Yf) @ np.linalg.inv(G))[:, 0, :]  # (F, N)
    return Y * np.transpose(scale)[:, :, None]


def max_cond(basis, H, eps):
    return max(float(np.max(np.linalg.cond(to_psd(np.einsum("nkt,nkbij->ntbij", H, Up), eps)))) for Up in to_parts(basis))


# ---------------------------------------------------------------------------------------------- metrics
def w_metric(a, b):
    """per bin max|a - b| / max|b|, the largest"""
    return float(np.max(np.max(np.abs(a - b), axis=(-2, -1)) / np.max(np.abs(b), axis=(-2, -1))))


def basis_metric(a, b):
    """per (source, basis) max|a - b| / max|b| over all its blocks, the largest"""
    pa, pb = pack(a), pack(b)
    return float(np.max(np.max(np.abs(pa - pb), axis=-1) / np.max(np.abs(pb), axis=-1)))


def h_metric(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def loss_metric(a, b, N, F, T):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + N * F * T)))


def out_metric(a, b):
    """per source max|a - b| / max|b|, the largest"""
    return float(np.max(np.max(np.abs(a - b), axis=(-2, -1)) / np.max(np.abs(b), axis=(-2, -1))))


def mat_metric(a, b):
    return w_metric(a, b)


def one_ulp(a, rng):
    """every real and imaginary part moved to a neighbouring double, direction drawn per entry"""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return one_ulp(a.real, rng) + 1j * one_ulp(a.imag, rng)
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def herm_ulp(basis, rng):
    """one_ulp of every block of a basis (public layout) that keeps the blocks Hermitian"""
    out = []
    for p in to_parts(basis):
        q = one_ulp(p, rng)
        low = np.tril(q, -1)
        d = np.einsum("...ii->...i", q).real
        q = low + ct(low)
        idx = np.arange(q.shape[-1])
        q[..., idx, idx] = d
        out.append(np.ascontiguousarray(np.transpose(q, (0, 2, 3, 4, 1))))
    return tuple(out) if isinstance(basis, (tuple, list)) else out[0]


def mixture(M, F, T, seed):
    """a seeded convolutive mixture (M, F, T): sources with a frame-varying power and a spectral envelope shared by
    neighbouring bins, one random mixing matrix per bin"""
    rng = np.random.default_rng(seed)
    S = (rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))) * (0.1 + rng.random((M, 1, T))) ** 2
    S = S + 0.5 * np.roll(S, 1, axis=1)
    A = rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))
    return np.ascontiguousarray(np.einsum("fmn,nft->mft", A, S))


def synthetic(M, F, T, K, n_blocks, seed):
    """(X, W, basis, H) for shapes the fixtures do not cover: the reference's start (identity W, diagonal bases)"""
    X = mixture(M, F, T, seed)
    rng = np.random.default_rng(seed + 1)
    parts = []
    for _, n, nb in part_ranges(F, n_blocks):
        parts.append((rng.random((M, K, n, nb))[..., None] * np.eye(nb)).astype(np.complex128))
    H = rng.random((M, K, T)) + 0.1
    W = np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1))
    basis, H = normalize(from_parts(parts, F, n_blocks), H, F, n_blocks)
    return X, W, basis, H


def psd_cases(n, seed):
    """seeded Hermitian matrices for the to_psd tests: (name, (N, n, n)) positive definite, one well-separated negative
    eigenvalue, rank one"""
    rng = np.random.default_rng(seed)
    N = 3
    q = np.linalg.qr(rng.standard_normal((N, n, n)) + 1j * rng.standard_normal((N, n, n)))[0]
    lam = 0.5 + rng.random((N, n))
    pd = (q * lam[:, None, :]) @ ct(q)
    lam2 = lam.copy()
    lam2[:, 0] = -0.75
    ind = (q * lam2[:, None, :]) @ ct(q)
    x = rng.standard_normal((N, n)) + 1j * rng.standard_normal((N, n))
    r1 = x[:, :, None] * np.conj(x[:, None, :])
    return (("definite", pd), ("indefinite", ind), ("rank_one", r1))
