"""Independent NumPy restatement of the closed-form spatial filters, written from the formulas of DESIGN.md section 20:
the delay-and-sum, ML and MVDR beamformers (reference src/bss/beamform.py:5-58), the per-bin PCA
(src/transform/pca.py:4-21) and the minimum distortion principle (src/algorithm/minimum_distortion_principle.py:3-31).
Nothing here is copied from the reference; tests/golden/beamform pins it to the reference's recorded output.

Shapes: X (M,F,T) complex, steering vectors A (F,M,N), covariance R (F,M,M), output (N,F,T).  The keyword flags are
planted faults for tests/test_beamform_cpu.py.
"""
import os

import numpy as np

EPS = 1e-12


def cgauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def mixture(M, F, T, seed):
    """Complex Gaussian channels scaled by 1 + m: the eigenvalues of every bin's covariance stay apart."""
    rng = np.random.default_rng(seed)
    return cgauss(rng, (M, F, T)) * (1.0 + np.arange(M))[:, None, None]


def steering(F, M, N, seed):
    return cgauss(np.random.default_rng(seed), (F, M, N)) / np.sqrt(M)


def covariance(X):
    """R[f,i,j] = mean_t X[i,f,t] conj(X[j,f,t])."""
    Xf = X.transpose(1, 0, 2)
    return Xf @ Xf.conj().transpose(0, 2, 1) / X.shape[2]


def reference_scale(A, ref, wrong_axis=False):
    """s[n,f] = A[f,ref,n]."""
    if wrong_axis:  # the reference index on the source axis
        F, M, N = A.shape
        return np.stack([A[:, n % M, ref % N] for n in range(N)])
    return A[:, ref, :].T


def delay_sum(X, A, ref=0, wrong_axis=False):
    Y = np.einsum("fmn,mft->nft", A.conj(), X)
    return reference_scale(A, ref, wrong_axis)[:, :, None] * Y


def floored(den, eps, floor_abs=False):
    """den = eps where den < eps in NumPy's order of complex numbers: the real parts, the imaginary parts on a tie."""
    den = np.array(den, dtype=np.complex128)
    below = np.abs(den) < eps if floor_abs else (den.real < eps) | ((den.real == eps) & (den.imag < 0))
    den[below] = eps
    return den, below


def ml_filter(A, R, eps=EPS, conj_filter=False, floor_abs=False):
    """W (F,N,M): W[f,n,m] = (R^-1 A)[f,m,n] / den[f,n], transposed and not conjugated."""
    num = np.linalg.solve(R, A)
    den, _ = floored(np.sum(A.conj() * num, axis=1), eps, floor_abs)
    W = (num / den[:, None, :]).transpose(0, 2, 1)
    return W.conj() if conj_filter else W


def ml(X, A, R, ref=0, eps=EPS, conj_filter=False, wrong_axis=False, floor_abs=False):
    W = ml_filter(A, R, eps, conj_filter, floor_abs)
    Y = (W @ X.transpose(1, 0, 2)).transpose(1, 0, 2)
    return reference_scale(A, ref, wrong_axis)[:, :, None] * Y


def mvdr(X, A, ref=0, eps=EPS, **fault):
    return ml(X, A, covariance(X), ref, eps, **fault)


def fix_phase(V):
    """Every column times the unit phase that makes its first entry real and non-negative."""
    a = V[..., 0:1, :]
    g = np.abs(a)
    return V * np.where(g > 0, a.conj() / np.where(g > 0, g, 1.0), 1.0)


def pca_basis(X, descending=False):
    """(V (F,M,M), w (F,M)): eigenvectors in columns, eigenvalues ascending, the phase convention applied."""
    w, V = np.linalg.eigh(covariance(X))
    V = fix_phase(V)
    if descending:
        w, V = w[:, ::-1], V[:, :, ::-1]
    return V, w


def project(X, V):
    """out[k,f,t] = sum_m X[m,f,t] conj(V[f,m,k])."""
    return np.einsum("mft,fmk->kft", X, V.conj())


def pca(X, descending=False):
    return project(X, pca_basis(X, descending)[0])


def eigen_gap(X):
    """The smallest gap between neighbouring eigenvalues over the largest eigenvalue, the least over the bins."""
    w = np.linalg.eigvalsh(covariance(X))
    return float(np.min(np.diff(w, axis=1).min(axis=1) / w[:, -1]))


def align_phase(out, ref):
    """`out` with every (component, bin) row turned by the phase of sum_t ref conj(out)."""
    ph = np.sum(ref * out.conj(), axis=-1, keepdims=True)
    g = np.abs(ph)
    return out * np.where(g > 0, ph / np.where(g > 0, g, 1.0), 1.0)


def mdp(Y, reference, conj_wrong=False):
    """scale[c,n,f] = sum_t conj(Y[n,f,t]) X[c,f,t] / sum_t |Y[n,f,t]|^2; a 2-D reference gives (N,F)."""
    Xr = reference[None] if reference.ndim == 2 else reference
    if Xr.ndim != 3:
        raise ValueError("reference.ndim is expected 2 or 3, but given {}.".format(reference.ndim))
    if conj_wrong:
        yx = np.einsum("nft,cft->cnf", Y, Xr.conj())
    else:
        yx = np.einsum("nft,cft->cnf", Y.conj(), Xr)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = yx / np.sum(np.abs(Y) ** 2, axis=2)
    return scale[0] if reference.ndim == 2 else scale


def chain(X, n_keep=2, iteration=5, phases=None):
    """pca(X)[:n_keep] -> AuxLaplaceIVA without projection back, `iteration` updates -> projection_back against X[0]
    (the reference's over-determined path, src/bss/iva.py:1092-1102).  phases (M,F): unit factors on the components, which
    the output must not depend on."""
    from oracle import oracle_np as orc
    Z = pca(X)
    if phases is not None:
        Z = Z * phases[:, :, None]
    Y = orc.auxiva(Z[:n_keep], iteration, "laplace", apply_projection_back=False, record_loss=False)["Y"]
    return Y * orc.projection_back(Y, X[0])[..., None]


# ---------------------------------------------------------------------------------------------------------- fixtures
def cases(golden):
    return sorted(f[:-4] for f in os.listdir(golden) if f.endswith(".npz") and ".part" not in f)


def load_case(golden, name):
    g = dict(np.load(os.path.join(golden, name + ".npz")))
    for i in range(1, int(g.get("n_parts", 1))):
        g.update(np.load(os.path.join(golden, "%s.part%d.npz" % (name, i))))
    return g
