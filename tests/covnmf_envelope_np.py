"""Host side of the covariance-domain MNMF envelope sweep (tests/test_gpu_covnmf_envelope.py,
tools/covnmf_tolerance_probe.py): the grid, the seeded general state, the restatement's outputs per entry point, and the
measured tolerances.  The metrics, the perturbation and the rule 256 * d with a floor of 1e-13 are those of
tests/envelope_np.py, imported as they are.  NumPy only; nothing here touches a GPU.

The one exception, as for MNMF: with T < 2 M frames the sums over t that enter the Riccati equation rest on fewer
frames than the matrices have real dimensions, so `update_spatial` of such a case gets 256 x ITS OWN d
(D_SPATIAL_FEW_FRAMES) and stays out of the grid's figure.  Measured, these d are SMALLER than the grid's (the target
has full rank, so one frame already gives a positive-definite C; MNMF's rank-one x x^H does not): the exception makes
those two comparisons stricter, not weaker.  No other output and no other case has a tolerance of its own.
"""
import functools

import numpy as np

import covnmf_np as cv
import envelope_np as env

# name: (M, K, F, T, seed)
GRID = {
    "m2_k1_f3_t1": (2, 1, 3, 1, 111),
    "m2_k15_f1_t64": (2, 15, 1, 64, 112),
    "m2_k16_f33_t65": (2, 16, 33, 65, 113),
    "m2_k64_f17_t577": (2, 64, 17, 577, 114),
    "m3_k17_f3_t63": (3, 17, 3, 63, 115),
    "m3_k33_f17_t130": (3, 33, 17, 130, 116),
    "m3_k1_f1_t577": (3, 1, 1, 577, 117),
    "m4_k16_f17_t64": (4, 16, 17, 64, 118),
    "m4_k33_f33_t130": (4, 33, 33, 130, 119),
    "m4_k64_f3_t65": (4, 64, 3, 65, 120),
    "m4_k15_f1_t1": (4, 15, 1, 1, 121),
    "m5_k17_f17_t65": (5, 17, 17, 65, 122),
    "m5_k1_f33_t63": (5, 1, 33, 63, 123),
    "m5_k64_f1_t130": (5, 64, 1, 130, 124),
    "m6_k33_f3_t577": (6, 33, 3, 577, 125),
    "m6_k16_f17_t63": (6, 16, 17, 63, 126),
    "m6_k15_f33_t64": (6, 15, 33, 64, 127),
    "m7_k64_f3_t130": (7, 64, 3, 130, 128),
    "m7_k17_f1_t65": (7, 17, 1, 65, 129),
    "m7_k1_f17_t64": (7, 1, 17, 64, 130),
    "m8_k64_f17_t130": (8, 64, 17, 130, 131),
    "m8_k33_f3_t63": (8, 33, 3, 63, 132),
    "m8_k16_f1_t577": (8, 16, 1, 577, 133),
    "m8_k15_f33_t65": (8, 15, 33, 65, 134),
}

OUTPUTS = ("basis", "activation", "spatial_normalized", "spatial_plain", "reconstruct", "loss")

# ---------------------------------------------------------------------------------------------------------- measured
# Output of `python tools/covnmf_tolerance_probe.py` (the largest d over the grid, per output), rounded up to two digits.
# The K = 1 cases set the figures (m7_k1_f17_t64: spatial 1.3e-12, basis 6.5e-15; m5_k1_f33_t63: spatial 9.5e-13): with one
# basis P = (Tb V H)^-1 and every output carries cond(H); everywhere else spatial stays below 9e-14 and the rest below
# 2.1e-15.  The target has full rank, so the two T < 2 M cases are far less sensitive here than MNMF's rank-one case.
D = {
    "basis": 6.5e-15,
    "activation": 5.2e-15,
    "spatial": 1.3e-12,
    "reconstruct": 1.1e-15,
    "loss": 3.6e-15,
}
# update_spatial of the cases with T < 2 M: their own d (see the module docstring)
D_SPATIAL_FEW_FRAMES = {
    "m2_k1_f3_t1": 1.8e-15,
    "m4_k15_f1_t1": 2.8e-14,
}

METRIC = {
    "basis": env.elem, "activation": env.elem, "loss": env.elem,
    "spatial": lambda a, b: env.block(a, b, 2),       # (F, K, M, M): per (f, k) matrix
    "reconstruct": lambda a, b: env.block(a, b, 2),   # (F, T, M, M): per (f, t) matrix
}


def kind(output):
    return output.split("_")[0]


def few_frames(case):
    M, _, _, T, _ = GRID[case]
    return T < 2 * M


def tolerance(case, output):
    """The entry-wise tolerance of one output (OUTPUTS) of one grid case."""
    k = kind(output)
    if k == "spatial" and few_frames(case):
        return env.tolerance(D_SPATIAL_FEW_FRAMES[case])
    return env.tolerance(D[k])


def entrywise(k, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.isfinite(a)), "non-finite output"
    return METRIC[k](a, b)


# ---------------------------------------------------------------------------------------------------------- states
def state(M, K, F, T, seed):
    """(X, Tb, V, H): X = the mean of M consecutive outer products of complex Gaussian frames with a per-bin scale, plus
    0.1 x its mean diagonal entry x I; Tb, V uniform in [0.05, 1.05]; H = G G^H + 0.1 I per (f, k), G complex Gaussian,
    divided by its trace."""
    rng = np.random.default_rng(seed)
    x = env._cgauss(rng, (F, T + M - 1, M)) * (0.1 + rng.random((F, 1, 1)))
    outer = x[..., :, None] * x[..., None, :].conj()
    X = sum(outer[:, s:s + T] for s in range(M)) / M
    X = X + 0.1 * np.mean(np.trace(X, axis1=-2, axis2=-1).real / M) * np.eye(M)
    X = (X + X.conj().swapaxes(-1, -2)) / 2
    Tb, V = env._uniform(rng, (F, K)), env._uniform(rng, (K, T))
    G = env._cgauss(rng, (F, K, M, M))
    H = G @ G.conj().swapaxes(-1, -2) + 0.1 * np.eye(M)
    H = (H + H.conj().swapaxes(-1, -2)) / 2
    H = H / np.trace(H, axis1=-2, axis2=-1).real[..., None, None]
    return X, Tb, V, H


def case_state(case):
    return state(*GRID[case])


def reference(st):
    """Every entry point of covnmf_np on ONE state (not chained)."""
    X, Tb, V, H = st
    return dict(basis=cv.update_basis(X, Tb, V, H), activation=cv.update_activation(X, Tb, V, H),
                spatial_normalized=cv.update_spatial(X, Tb, V, H, normalize=True),
                spatial_plain=cv.update_spatial(X, Tb, V, H, normalize=False),
                reconstruct=cv.reconstruct(Tb, V, H), loss=np.float64(cv.loss(X, Tb, V, H)))


@functools.lru_cache(maxsize=None)
def grid_case(case):
    """(state, reference) of a grid case, with the host-side conditions asserted."""
    st = case_state(case)
    low = cv.denominators(*st)
    assert low > env.MIN_DENOMINATOR, "%s: a denominator of %.3e is too close to the eps clamp" % (case, low)
    ref = reference(st)
    assert all(np.all(np.isfinite(v)) for v in ref.values()), case
    return st, ref


# ---------------------------------------------------------------------------------------------------------- probe
def perturb_state(st, rng, u):
    X, Tb, V, H = (env.perturb(a, rng, u) for a in st)
    return (X + X.conj().swapaxes(-1, -2)) / 2, Tb, V, (H + H.conj().swapaxes(-1, -2)) / 2


def sensitivity(st, u=env.U64, draws=3, seed=0):
    """{output: d}: the largest entry-wise difference between reference(state) and reference(perturbed state)."""
    rng = np.random.default_rng(seed)
    base = reference(st)
    d = {k: 0.0 for k in base}
    for _ in range(draws):
        other = reference(perturb_state(st, rng, u))
        for k in base:
            d[k] = max(d[k], entrywise(kind(k), other[k], base[k]))
    return d
