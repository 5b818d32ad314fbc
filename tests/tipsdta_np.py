"""NumPy restatement of tIPSDTA (the Student-t, block-diagonal independent positive semidefinite tensor analysis), stage by
stage as the HIP kernels run it.  Geometry, layouts, psd(), the linear-algebra back ends (`la=LAPACK | KERNEL`), the
normalisation and the metrics are those of tests/ipsdta_np.py; this module adds what the Student-t model changes.

With R, Ri and y as in ipsdta_np, q[n,b,t] = y_b^H Ri_b y_b and

    pi[n,t]     = (nu + 2 n_bins) / (nu + 2 sum_blocks q[n,b,t])
    basis       S_k = sum_t H pi Ri (y y^H + eps I) Ri, T_k = sum_t H Ri, then the Gauss update
    activation  num = pi sum_blocks Re tr(Ri U_k Ri psd(y y^H + eps I)), den and the quotient as in the Gauss update
    spatial     Ri once per call; a sweep is the sequence of steps (source n; the low blocks at position 0..nn-1, then the high
                blocks at position 0..nn).  A step: pi_n from the current W and ALL blocks,
                Q = psd(mean_t pi_n (Ri)_ii psd(x x^H)), gamma = mean_t pi_n sum_{j != i} (Ri)_ji x_i conj(y_j), then the
                Gauss row update for every block of the group
    loss        sum log max(lambda(R), eps) + (nu + 2 n_bins)/2 sum_{n,t} log(1 + (2/nu) sum_blocks q)
                - 2 T sum_f sum log max(|lambda(W_f)|, eps)

With pi = 1 every stage runs the arithmetic of ipsdta_np on arrays of the same shapes, so nu = 1e30 (where pi rounds to
exactly 1.0) reproduces the Gauss restatement bit for bit.  `fault=` plants the three mistakes the fixtures must see:
'pi_per_source' (pi computed once per source instead of before every step), 'pi_own_block' (q of the stepped block alone),
'high_first' (the high group stepped before the low one).  Written from the equations above; nothing is taken from another
code base.
"""
import glob
import json
import os

import numpy as np

import ipsdta_np as ip
from ipsdta_np import KERNEL, LAPACK  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "tipsdta")
N_ITER, SNAP_ITERS, START_ITERS = ip.N_ITER, ip.SNAP_ITERS, ip.START_ITERS
FAULTS = ("pi_per_source", "pi_own_block", "high_first")


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "tipsdta_*.npz")))


def tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as fh:
        return json.load(fh)


def dims(fx):
    return ip.dims(fx)


def quad_parts(X, W, Ri_parts, n_blocks):
    """q per part: [(N, T, n)]"""
    F = X.shape[1]
    Y = ip.separate(X, W)
    out = []
    for (f0, n, nb), Ri in zip(ip.part_ranges(F, n_blocks), Ri_parts):
        y = ip.block_outputs(Y, f0, n, nb)
        out.append(np.einsum("ntbi,ntbij,ntbj->ntb", np.conj(y), Ri, y).real)
    return out


def pi_from_quad(q_parts, nu, F):
    """(N, T): the blocks added in index order"""
    s = 0.0
    for q in q_parts:
        for b in range(q.shape[2]):
            s = s + q[:, :, b]
    return (nu + 2 * F) / (nu + 2 * s)


def pi(X, W, basis, H, eps, n_blocks, nu, la=LAPACK):
    return pi_from_quad(quad_parts(X, W, ip.inverse_parts(basis, H, eps, la), n_blocks), nu, X.shape[1])


def update_basis(X, W, basis, H, eps, n_blocks, nu, la=LAPACK):
    F = X.shape[1]
    Y = ip.separate(X, W)
    parts = ip.to_parts(basis)
    Ris = [ip.model_inverse(Up, H, eps, la) for Up in parts]
    p = pi_from_quad(quad_parts(X, W, Ris, n_blocks), nu, F)
    out = []
    for (f0, n, nb), Up, Ri in zip(ip.part_ranges(F, n_blocks), parts, Ris):
        y = ip.block_outputs(Y, f0, n, nb)
        yy = y[..., :, None] * np.conj(y[..., None, :]) + eps * np.eye(nb)
        Z = p[:, :, None, None, None] * (Ri @ yy @ Ri)
        S = np.einsum("nkt,ntbij->nkbij", H, Z)
        Tm = np.einsum("nkt,ntbij->nkbij", H, Ri)
        s = ip.to_psd(la.sqrtm((S + ip.ct(S)) / 2 if la is KERNEL else S), eps, la)
        C = ip.to_psd(s @ Up @ Tm @ Up @ s, eps, la)
        Ci = ip.to_psd(la.inv(ip.to_psd(la.sqrtm(C), eps, la)), eps, la)
        out.append(ip.to_psd(Up @ s @ Ci @ s @ Up, eps, la))
    return ip.from_parts(out, F, n_blocks)


def update_activation(X, W, basis, H, eps, n_blocks, nu, la=LAPACK, diag=None):
    F = X.shape[1]
    Y = ip.separate(X, W)
    parts = ip.to_parts(basis)
    Ris = [ip.model_inverse(Up, H, eps, la) for Up in parts]
    p = pi_from_quad(quad_parts(X, W, Ris, n_blocks), nu, F)
    num, den = 0.0, 0.0
    for (f0, n, nb), Up, Ri in zip(ip.part_ranges(F, n_blocks), parts, Ris):
        y = ip.block_outputs(Y, f0, n, nb)
        yy = ip.to_psd(y[..., :, None] * np.conj(y[..., None, :]) + eps * np.eye(nb), eps, la, shift=la.rank_one_shift)
        G = Ri @ yy @ Ri
        num = num + np.einsum("nkbij,ntbji->nkt", Up, G).real
        den = den + np.einsum("nkbij,ntbji->nkt", Up, Ri).real
    num = p[:, None, :] * num
    if diag is not None:
        diag["num_floored"] = bool(np.any(num < 0.0))
        diag["den_floored"] = bool(np.any(den < eps))
        diag["num_min"], diag["den_min"] = float(np.min(num)), float(np.min(den))
    return H * np.sqrt(np.maximum(num, 0.0) / np.maximum(den, eps))


def update_source(X, W, basis, H, eps, n_blocks, nu, norm=True, la=LAPACK):
    F = X.shape[1]
    basis = update_basis(X, W, basis, H, eps, n_blocks, nu, la)
    H = update_activation(X, W, basis, H, eps, n_blocks, nu, la)
    if norm:
        basis, H = ip.normalize(basis, H, F, n_blocks)
    return basis, H


def spatial_sweep(X, W, Ri_parts, XX, eps, n_blocks, nu, la=LAPACK, diag=None, fault=None):
    """one VCD sweep; returns the new W.  XX (F, T, M, M) = psd(x x^H)."""
    M, F, T = X.shape
    W = W.copy()
    ranges = ip.part_ranges(F, n_blocks)
    groups = list(range(len(ranges)))
    if fault == "high_first":
        groups.reverse()
    for src in range(M):
        p_fixed = pi_from_quad(quad_parts(X, W, Ri_parts, n_blocks), nu, F) if fault == "pi_per_source" else None
        for gi in groups:
            f0, n, nb = ranges[gi]
            Ri = Ri_parts[gi]
            Xp = X[:, f0:f0 + n * nb, :].reshape(M, n, nb, T)
            e_n = np.zeros((n, M), dtype=np.complex128)
            e_n[:, src] = 1.0
            for i in range(nb):
                q_parts = quad_parts(X, W, Ri_parts, n_blocks)
                p = pi_from_quad(q_parts, nu, F) if p_fixed is None else p_fixed
                Wp = W[f0:f0 + n * nb].reshape(n, nb, M, M).copy()
                bins = f0 + np.arange(n) * nb + i
                if fault == "pi_own_block":
                    pb = (nu + 2 * F) / (nu + 2 * q_parts[gi][src])  # (T, n)
                    wq = pb * Ri[src, :, :, i, i].real
                    Qi = ip.to_psd(np.einsum("tb,btcd->bcd", wq, XX[bins]) / T, eps, la)
                    pg = np.transpose(pb)  # (n, T)
                else:
                    # Q of every (source, bin) by the arithmetic of ipsdta_np.q_matrices, the step's matrices taken out of it
                    w = np.empty((M, F, T))
                    for (g0, gn, gnb), Rg in zip(ranges, Ri_parts):
                        d = np.einsum("ntbii->ntbi", Rg).real * p[:, :, None, None]
                        w[:, g0:g0 + gn * gnb, :] = np.transpose(d, (0, 2, 3, 1)).reshape(M, gn * gnb, T)
                    Qi = ip.to_psd((np.einsum("nft,ftcd->nfcd", w, XX) / T)[src, bins], eps, la)
                    pg = p[src][None, :]
                y = np.einsum("bjc,cbjt->bjt", Wp[:, :, src, :], Xp)
                r = np.transpose(Ri[src, :, :, :, i], (1, 2, 0))  # (n, nb [j], T)
                mask = np.ones(nb)
                mask[i] = 0.0
                s = np.einsum("j,bjt,bjt->bt", mask, r, np.conj(y)) * pg
                gamma = np.einsum("bt,cbt->bc", s, Xp[:, :, i, :]) / T
                zeta = np.linalg.solve(Wp[:, i] @ Qi, e_n[:, :, None])[:, :, 0]
                zeta_hat = np.linalg.solve(Qi, gamma[:, :, None])[:, :, 0]
                u = np.einsum("bc,bcd->bd", np.conj(zeta), Qi)
                eta, eta_hat = np.sum(u * zeta, axis=1), np.sum(u * zeta_hat, axis=1)
                weight, _ = ip.vcd_weight(eta, eta_hat, eps)
                if diag is not None and nb > 1:
                    a = np.abs(eta_hat)
                    diag["eta_hat_min"] = min(diag.get("eta_hat_min", np.inf), float(np.min(a[a > 0.0], initial=np.inf)))
                if diag is not None:
                    diag["eta_min"] = min(diag.get("eta_min", np.inf), float(np.min(np.abs(eta))))
                W[bins, src, :] = np.conj(weight[:, None] * zeta - zeta_hat)
    return W


def rank_one(X, eps, la=LAPACK):
    """XX (F, T, M, M) = psd(x x^H)"""
    xt = np.transpose(X, (1, 2, 0))
    return ip.to_psd(xt[..., :, None] * np.conj(xt[..., None, :]), eps, la, shift=la.rank_one_shift)


def update_spatial(X, W, basis, H, eps, n_blocks, nu, n_sweeps, la=LAPACK, each=False, fault=None, diag=None):
    """n_sweeps VCD sweeps on the hoisted Ri; each=True returns the list of W after every sweep"""
    Ri = ip.inverse_parts(basis, H, eps, la)
    XX = rank_one(X, eps, la)
    out = []
    for _ in range(n_sweeps):
        W = spatial_sweep(X, W, Ri, XX, eps, n_blocks, nu, la, diag=diag, fault=fault)
        out.append(W)
    return out if each else W


def loss(X, W, basis, H, eps, n_blocks, nu, la=LAPACK):
    M, F, T = X.shape
    Ris, logdet = [], 0.0
    for Up in ip.to_parts(basis):
        Ri, R = ip.model_inverse(Up, H, eps, la, with_r=True)
        Ris.append(Ri)
        logdet += np.sum(np.log(np.maximum(la.eigvalsh(R), eps)))
    s = 0.0
    for q in quad_parts(X, W, Ris, n_blocks):
        for b in range(q.shape[2]):
            s = s + q[:, :, b]
    return float(logdet + (nu + 2 * F) / 2 * np.sum(np.log(1 + (2 / nu) * s)) - 2 * T * np.sum(la.logabsdet(W, eps)))


def iterate(X, W, basis, H, eps, n_blocks, nu, n_sweeps, norm=True, la=LAPACK, fault=None):
    """one iteration: (W, basis, H, loss)"""
    basis, H = update_source(X, W, basis, H, eps, n_blocks, nu, norm, la)
    W = update_spatial(X, W, basis, H, eps, n_blocks, nu, n_sweeps, la, fault=fault)
    return W, basis, H, loss(X, W, basis, H, eps, n_blocks, nu, la)
