"""Per-bin PCA on MI355X -- drop-in for `transform.pca.pca` of the reference (src/transform/pca.py:4-21).  NumPy in, NumPy
out; a device tensor in, a device tensor out.  The covariance mean_t x x^H (assx_cov_accumulate), its Hermitian
eigendecomposition by cyclic Jacobi (assx_pca_basis) and the projection (assx_bf_apply) run on the device.  float64, one
utterance, 2 <= n_channels <= 8.

Eigenvalues ascend: component 0 is the weakest, and `pca(x)[:n]` keeps the reference's quirk of taking the n weakest.
An eigenvector is fixed only up to a unit phase, and so is a component.  The convention here: the first entry of every
eigenvector, v[f, 0, k], is real and non-negative (LAPACK returns a real first row of either sign).
"""
from .. import _spatial as sp

__all__ = ["pca", "pca_basis"]


def _basis(what, input, dtype, device):
    if len(sp.shape(input)) != 3:
        raise ValueError("Invalid dimension.")
    sp.check_dtype(what, dtype)
    M, F, _ = sp.check_signal(what, "input", input, 2)
    eng = sp.engine(device)
    X = sp.on_device(input, eng)
    status = eng.new_status(1)
    V, w, Wf = eng.pca_basis(eng.cov_accumulate(X.unsqueeze(0)).reshape(F, M, M), status)
    return eng, X, V, w, Wf


def pca(input, *, dtype='float64', device=None):
    """
    Args:
        input (n_channels, n_bins, n_frames)
    Returns:
        output (n_channels, n_bins, n_frames): output[k,f,t] = sum_m input[m,f,t] conj(v[f,m,k])
    """
    eng, X, _, _, Wf = _basis("pca", input, dtype, device)
    return sp.give_back(input, eng.bf_apply(X, Wf))


def pca_basis(input, *, dtype='float64', device=None):
    """The basis `pca` projects on: (eigenvectors (n_bins, n_channels, n_channels), one per column, and eigenvalues
    (n_bins, n_channels) ascending) of the per-bin covariance.  No counterpart in the reference, which discards both."""
    import numpy as np
    _, _, V, w, _ = _basis("pca_basis", input, dtype, device)
    return sp.give_back(input, V), sp.give_back(input, w, np.float64)
