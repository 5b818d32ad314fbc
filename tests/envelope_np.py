"""Shared host side of the envelope sweeps (tests/test_gpu_mnmf_envelope.py, tests/test_gpu_fastmnmf_envelope.py,
tests/test_envelope_cpu.py, tools/mnmf_tolerance_probe.py): the grids, the seeded general states, the restatements'
outputs per entry point, the entry-wise metrics, and the measured tolerances.  NumPy only; nothing here touches a GPU.

Metrics.  `rel` is the project's global one, max|a - b| / max|b| over a whole array: one wrong small entry hides behind
the largest entry of the array.  The entry-wise ones divide by something local instead:

    elem   max |a - b| / |b| element by element             basis, activation, latent, W, H, g (all positive)
    block  max |a - b| over a block / max |b| of that block  spatial per (f, n) matrix, Q per (f) matrix,
                                                             separate per (n, f) row
    scalar |a - b| / |b|                                     loss

Tolerances.  They are not read off a kernel.  `sensitivity` evaluates a restatement on a state and on three copies with
every real and imaginary part multiplied by 1 + s * u, s drawn from {-1, 0, 1} (spatial re-symmetrised), and returns
the largest entry-wise difference d per output: what ONE rounding of the inputs does to the output, a lower bound on
the difference between two correct implementations that sum in another order.  tools/mnmf_tolerance_probe.py runs it
over the whole grids; the D_* tables below are its output and `tolerance` turns them into 256 * d with a floor (sums
of up to 1000 frames x 64 bases in another order, and a Cholesky-based instead of a LAPACK inverse, account for two
orders of magnitude; more than that is a finding).  u = 2^-52 for float64, 2^-23 for float32 (the float64 restatement
on the float32-rounded state; it cannot run in float32 itself).  The floor is 1e-13 in float64, for a d of zero or a
few units of roundoff (the loss: a sum of up to 70 000 terms of mixed sign does not agree to the last bit), and the
same floor scaled by 2^29, the ratio of the unit roundoffs, in float32.

The one exception: with T < 2 M frames the MNMF spatial update is ill-posed (C = sum_t lam y y^H has rank T < M; the
matrix square root inside the Riccati solution turns a rounding u into sqrt(u)), so `update_spatial` of such a case
gets 256 x ITS OWN d (D_MNMF_SPATIAL_FEW_FRAMES).  No other output and no other case has a tolerance of its own.
"""
import functools

import numpy as np

import fastmnmf_np as fm
import mnmf_np as mn

U64 = 2.0 ** -52
U32 = 2.0 ** -23
FACTOR = 256.0
FLOOR64 = 1e-13
FLOOR32 = FLOOR64 * 2.0 ** 29
REL_TOL = 1e-9  # the project's existing bound on the global metric, float64
MIN_DENOMINATOR = 1e-6  # every clamped denominator of a grid case stays this far above eps = 1e-12
COND_Q_MAX = 1e3
COND_FAR = 1e3  # cond(Q V_m) of a grid case is below threshold / COND_FAR or above threshold * COND_FAR

# ---------------------------------------------------------------------------------------------------------- grids
# name: (M, N, K, F, T, seeds); more than one seed = one batched call with that many different states
MNMF_GRID = {
    "m2_n1_k1_f3_t1": (2, 1, 1, 3, 1, (11,)),
    "m2_n5_k15_f1_t64": (2, 5, 15, 1, 64, (12,)),
    "m2_n1_k16_f15_t65": (2, 1, 16, 15, 65, (13,)),
    "m2_n8_k64_f16_t577": (2, 8, 64, 16, 577, (14,)),
    "m3_n8_k48_f70_t63": (3, 8, 48, 70, 63, (15,)),
    "m3_n1_k17_f16_t130": (3, 1, 17, 16, 130, (16,)),
    "m3_n2_k8_f1_t1000": (3, 2, 8, 1, 1000, (17,)),
    "m4_n4_k10_f17_t1000": (4, 4, 10, 17, 1000, (18,)),
    "m4_n6_k33_f3_t65": (4, 6, 33, 3, 65, (19,)),
    "m4_n2_k8_f33_t64": (4, 2, 8, 33, 64, (20,)),
    "m5_n5_k17_f19_t200": (5, 5, 17, 19, 200, (21,)),
    "m5_n3_k16_f15_t63": (5, 3, 16, 15, 63, (22,)),
    "m5_n8_k33_f33_t130": (5, 8, 33, 33, 130, (23,)),
    "m6_n7_k33_f5_t67": (6, 7, 33, 5, 67, (24,)),
    "m6_n2_k64_f16_t130": (6, 2, 64, 16, 130, (25,)),
    "m6_n5_k1_f70_t64": (6, 5, 1, 70, 64, (26,)),
    "m7_n8_k64_f33_t577": (7, 8, 64, 33, 577, (27,)),
    "m7_n3_k15_f17_t65": (7, 3, 15, 17, 65, (28,)),
    "m8_n8_k64_f20_t130": (8, 8, 64, 20, 130, (29,)),
    "m8_n3_k17_f3_t577": (8, 3, 17, 3, 577, (30,)),
    "m8_n1_k64_f15_t63": (8, 1, 64, 15, 63, (31,)),
    "m5_n6_k17_f17_t130_b3": (5, 6, 17, 17, 130, (32, 33, 34)),
    "m7_n5_k16_f15_t65_b3": (7, 5, 16, 15, 65, (35, 36, 37)),
}

FASTMNMF_GRID = {
    "m2_n1_k1_f3_t1": (2, 1, 1, 3, 1, (51,)),
    "m2_n6_k16_f1_t64": (2, 6, 16, 1, 64, (52,)),
    "m2_n8_k64_f15_t577": (2, 8, 64, 15, 577, (53,)),
    "m3_n8_k48_f70_t63": (3, 8, 48, 70, 63, (54,)),
    "m3_n1_k17_f16_t130": (3, 1, 17, 16, 130, (55,)),
    "m4_n4_k10_f17_t1000": (4, 4, 10, 17, 1000, (56,)),
    "m4_n7_k33_f15_t65": (4, 7, 33, 15, 65, (57,)),
    "m4_n1_k64_f70_t64": (4, 1, 64, 70, 64, (58,)),
    "m5_n6_k17_f19_t200": (5, 6, 17, 19, 200, (59,)),
    "m5_n8_k64_f16_t130": (5, 8, 64, 16, 130, (60,)),
    "m6_n3_k16_f16_t65": (6, 3, 16, 16, 65, (61,)),
    "m6_n1_k16_f33_t577": (6, 1, 16, 33, 577, (62,)),
    "m7_n7_k33_f5_t67": (7, 7, 33, 5, 67, (63,)),
    "m7_n2_k15_f17_t64": (7, 2, 15, 17, 64, (64,)),
    "m8_n8_k64_f33_t577": (8, 8, 64, 33, 577, (65,)),
    "m8_n6_k1_f3_t63": (8, 6, 1, 3, 63, (66,)),
}

# ---------------------------------------------------------------------------------------------------------- measured
# Output of `python tools/mnmf_tolerance_probe.py` (the largest d over the grid, per output), rounded up to two digits.
# The N = 1 cases set the MNMF figures (m8_n1_k64_f15_t63: spatial 4.2e-12, separate 3.0e-14): with one source
# P = (lam H)^-1, so every output carries cond(H); everywhere else spatial stays below 2e-13 and the rest below 2e-15.
D_MNMF = {
    "basis": 9.3e-15,
    "activation": 1.1e-14,
    "latent": 1.2e-15,
    "spatial": 4.2e-12,
    "loss": 5.9e-16,
    "separate": 3.1e-14,
}
# update_spatial of the cases with T < 2 M: their own d (see the module docstring)
D_MNMF_SPATIAL_FEW_FRAMES = {
    "m2_n1_k1_f3_t1": 6.9e-8,
}
D_FASTMNMF = {
    "float64": {"loss": 1.4e-15, "W": 1.6e-15, "H": 1.4e-15, "g": 4.0e-15, "Q": 6.3e-16, "separate": 1.7e-15},
    "float32": {"loss": 4.2e-7, "W": 5.8e-7, "H": 5.8e-7, "g": 3.1e-7, "Q": 1.8e-7, "separate": 5.1e-7},
}


def tolerance(d, floor=FLOOR64):
    return max(FACTOR * d, floor)


def mnmf_tolerance(case, output):
    """The entry-wise tolerance of one MNMF output (keys of `mnmf_reference`) of one grid case."""
    kind = mnmf_kind(output)
    if kind == "spatial" and few_frames(case):
        return tolerance(D_MNMF_SPATIAL_FEW_FRAMES[case])
    return tolerance(D_MNMF[kind])


def fastmnmf_tolerance(output, dtype="float64"):
    return tolerance(D_FASTMNMF[dtype][fastmnmf_kind(output)], FLOOR64 if dtype == "float64" else FLOOR32)


def few_frames(case):
    M, _, _, _, T, _ = MNMF_GRID[case]
    return T < 2 * M


def mnmf_kind(output):
    return output.split("_")[0]


def fastmnmf_kind(output):
    """nmf_W, normalize_W -> W; diagonalizer_Q -> Q; separate_3 -> separate; ..."""
    head, _, tail = output.partition("_")
    return head if head in ("loss", "separate") else tail


# ---------------------------------------------------------------------------------------------------------- metrics
def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def elem(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def block(a, b, naxes):
    """max over the leading axes of (max|a - b| over the last `naxes` axes) / (max|b| over the same)."""
    a, b = np.asarray(a), np.asarray(b)
    ax = tuple(range(-naxes, 0))
    return float(np.max(np.max(np.abs(a - b), axis=ax) / np.maximum(np.max(np.abs(b), axis=ax), 1e-300)))


METRIC = {
    "basis": elem, "activation": elem, "latent": elem, "W": elem, "H": elem, "g": elem, "loss": elem,
    "spatial": lambda a, b: block(a, b, 2),   # (.., F, N, M, M): per (f, n) matrix
    "Q": lambda a, b: block(a, b, 2),         # (.., F, M, M): per (f) matrix
    "separate": lambda a, b: block(a, b, 1),  # (.., N, F, T): per (n, f) row
}


def entrywise(kind, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.isfinite(a)), "non-finite output"
    return METRIC[kind](a, b)


# ---------------------------------------------------------------------------------------------------------- states
def _cgauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _uniform(rng, shape):
    return 0.05 + rng.random(shape)


def mnmf_state(M, N, K, F, T, seed):
    """(X, Tb, V, Z, H): X complex Gaussian with a per-bin scale; Tb, V uniform in [0.05, 1.05]; Z positive with columns
    summing to one; H = G G^H + 0.1 I per (f, n), G complex Gaussian, divided by its trace."""
    rng = np.random.default_rng(seed)
    X = _cgauss(rng, (M, F, T)) * (0.1 + rng.random((1, F, 1)))
    Tb, V = _uniform(rng, (F, K)), _uniform(rng, (K, T))
    Z = _uniform(rng, (N, K))
    Z = Z / Z.sum(axis=0)
    G = _cgauss(rng, (F, N, M, M))
    H = mn._herm(G @ G.conj().swapaxes(-1, -2) + 0.1 * np.eye(M))
    H = H / np.trace(H, axis1=-2, axis2=-1).real[..., None, None]
    return X, Tb, V, Z, H


def fastmnmf_state(M, N, K, F, T, seed):
    """(X, W, H, g, Q): X as above; W, H, g uniform in [0.05, 1.05]; Q = I + 0.3 / sqrt(M) x complex Gaussian."""
    rng = np.random.default_rng(seed)
    X = _cgauss(rng, (M, F, T)) * (0.1 + rng.random((1, F, 1)))
    W, H, g = _uniform(rng, (N, F, K)), _uniform(rng, (N, K, T)), _uniform(rng, (N, F, M))
    Q = np.eye(M) + 0.3 / np.sqrt(M) * _cgauss(rng, (F, M, M))
    return X, W, H, g, Q


def round_to_float32(state):
    return tuple(a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a)
                 else a.astype(np.float32).astype(np.float64) for a in state)


def mnmf_states(case):
    M, N, K, F, T, seeds = MNMF_GRID[case]
    return [mnmf_state(M, N, K, F, T, s) for s in seeds]


def fastmnmf_states(case, dtype="float64"):
    M, N, K, F, T, seeds = FASTMNMF_GRID[case]
    states = [fastmnmf_state(M, N, K, F, T, s) for s in seeds]
    return [round_to_float32(s) for s in states] if dtype == "float32" else states


def reference_ids(M):
    """0, one in between (M > 2), M - 1."""
    return tuple(sorted({0, M // 2, M - 1}))


# ---------------------------------------------------------------------------------------------------------- references
def mnmf_denominators(X, Tb, V, Z, H, eps=mn.EPS):
    """The smallest of the denominators that `mnmf_np` clamps at eps (basis, activation, latent, latent column sum)."""
    F, K = Tb.shape
    db = np.empty((F, K))
    dv = np.zeros(V.shape)
    dz = np.zeros(Z.shape)
    for s in mn._chunks(F):
        _, _, _, _, b = mn._eval(X[:, s], Tb[s], V, Z, H[s], eps)
        db[s] = np.einsum("nk,kt,nft->fk", Z, V, b)
        dv += np.einsum("nk,fk,nft->kt", Z, Tb[s], b)
        dz += np.einsum("fk,kt,nft->nk", Tb[s], V, b)
    return float(min(db.min(), dv.min(), dz.min()))


def mnmf_reference(state):
    """Every entry point of mnmf_np on ONE state (not chained): basis, activation, latent, spatial_normalized,
    spatial_plain, loss, separate_<ref> for `reference_ids(M)`."""
    X, Tb, V, Z, H = state
    out = dict(basis=mn.update_basis(*state), activation=mn.update_activation(*state),
               latent=mn.update_latent(*state), spatial_normalized=mn.update_spatial(*state, normalize=True),
               spatial_plain=mn.update_spatial(*state, normalize=False), loss=np.float64(mn.loss(*state)))
    for r in reference_ids(X.shape[0]):
        out["separate_%d" % r] = mn.separate(*state, reference_id=r)
    return out


def fastmnmf_conds(X, W, H, g, Q, eps=fm.EPS):
    """cond(Q_f) (largest) and every cond(Q_f V_fm) that the diagonaliser update compares with its threshold, for the
    entry state (the first channel's value; later channels see rows of Q already updated, of the same size)."""
    M, F, T = X.shape
    conds = np.empty((F, M))
    with np.errstate(all="ignore"):
        for f in range(F):
            _, R = fm._mix(W[:, f], H, g[:, f])
            R = np.maximum(R, eps)
            for m in range(M):
                Vm = (X[:, f] / R[:, m]) @ X[:, f].conj().T / T
                conds[f, m] = np.linalg.cond(Q[f] @ Vm)
    return float(np.max(np.linalg.cond(Q))), conds


def fastmnmf_reference(state):
    """Every entry point of fastmnmf_np on ONE state: loss, nmf_W, nmf_H, scm_g, diagonalizer_Q, normalize_{W,H,g,Q},
    separate_<ref> for the non-zero ones of `reference_ids(M)`."""
    X, W, H, g, Q = state
    with np.errstate(all="ignore"):  # cond() of a rank-deficient Q V (T < M) divides by zero; the branch is asserted
        Qn = fm.update_diagonalizer(X, W, H, g, Q)
    out = dict(loss=np.float64(fm.loss(X, W, H, g, Q)), diagonalizer_Q=Qn, scm_g=fm.update_scm(X, W, H, g, Q))
    out["nmf_W"], out["nmf_H"] = fm.update_nmf(X, W, H, g, Q)
    for k, v in zip(("W", "H", "g", "Q"), fm.normalize_power(W, H, g, Q)):
        out["normalize_" + k] = v
    for r in reference_ids(X.shape[0])[1:]:
        out["separate_%d" % r] = fm.separate(X, W, H, g, Q, reference_id=r)
    return out


def fastmnmf_min_denominator(X, W, H, g, Q, eps=fm.EPS):
    """The smallest of R and of the denominators fastmnmf_np clamps at eps in update_nmf / update_scm."""
    N, F, K = W.shape
    low = np.inf
    denH = np.zeros(H.shape)
    for f in range(F):
        lam, R = fm._mix(W[:, f], H, g[:, f])
        gR = g[:, f] @ (1 / R).T
        denH += W[:, f, :, None] * gR[:, None, :]
        low = min(low, R.min(), np.einsum("nkt,nt->nk", H, gR).min(), (lam @ (1 / R)).min())
    return float(min(low, denH.min()))


@functools.lru_cache(maxsize=None)
def mnmf_case(case):
    """(states, references) of a grid case, with the host-side conditions asserted."""
    states = mnmf_states(case)
    for s in states:
        low = mnmf_denominators(*s)
        assert low > MIN_DENOMINATOR, "%s: a denominator of %.3e is too close to the eps clamp" % (case, low)
    refs = [mnmf_reference(s) for s in states]
    for r in refs:
        assert all(np.all(np.isfinite(v)) for v in r.values()), case
        Zu = r["latent"]
        assert Zu.min() > MIN_DENOMINATOR
    return states, refs


@functools.lru_cache(maxsize=None)
def fastmnmf_case(case, dtype="float64", threshold=fm.THRESHOLD):
    states = fastmnmf_states(case, dtype)
    for s in states:
        condQ, conds = fastmnmf_conds(*s)
        assert condQ < COND_Q_MAX, "%s: cond(Q) = %.3e" % (case, condQ)
        near = (conds > threshold / COND_FAR) & (conds < threshold * COND_FAR)
        assert not near.any(), "%s: cond(Q V) = %s is near the threshold" % (case, conds[near])
        low = fastmnmf_min_denominator(*s)
        assert low > MIN_DENOMINATOR, "%s: a denominator of %.3e is too close to the eps clamp" % (case, low)
    refs = [fastmnmf_reference(s) for s in states]
    for r in refs:
        assert all(np.all(np.isfinite(v)) for v in r.values()), case
    return states, refs


def diagonalizer_skips(case):
    """True where the float64 restatement leaves Q alone because cond(Q V) is beyond the threshold (V of rank T < M)."""
    M, _, _, _, T, _ = FASTMNMF_GRID[case]
    return T < M


# ---------------------------------------------------------------------------------------------------------- probe
def perturb(a, rng, u):
    """Every real and imaginary part times 1 + s * u, s in {-1, 0, 1}."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return a.real * (1 + rng.integers(-1, 2, a.shape) * u) + 1j * a.imag * (1 + rng.integers(-1, 2, a.shape) * u)
    return a * (1 + rng.integers(-1, 2, a.shape) * u)


def perturb_mnmf(state, rng, u):
    X, Tb, V, Z, H = (perturb(a, rng, u) for a in state)
    return X, Tb, V, Z, mn._herm(H)


def perturb_fastmnmf(state, rng, u):
    return tuple(perturb(a, rng, u) for a in state)


def sensitivity(reference, perturb_state, kind_of, state, u, draws=3, seed=0):
    """{output: d}: the largest entry-wise difference between reference(state) and reference(perturbed state)."""
    rng = np.random.default_rng(seed)
    base = reference(state)
    d = {k: 0.0 for k in base}
    for _ in range(draws):
        other = reference(perturb_state(state, rng, u))
        for k in base:
            d[k] = max(d[k], entrywise(kind_of(k), other[k], base[k]))
    return d


def mnmf_sensitivity(state, u=U64, draws=3, seed=0):
    return sensitivity(mnmf_reference, perturb_mnmf, mnmf_kind, state, u, draws, seed)


def fastmnmf_sensitivity(state, u=U64, draws=3, seed=0):
    return sensitivity(fastmnmf_reference, perturb_fastmnmf, fastmnmf_kind, state, u, draws, seed)


# ---------------------------------------------------------------------------------------------------------- fixtures
# Reference-recorded FastMNMF fixtures whose trajectory is ill-conditioned past iteration LAST_STABLE_ITERATION.  With
# N * K = 231 / 512 bases and the T <= 48 frames that a 1 MiB file allows (it holds five copies of the (N, K, T)
# activation) the model has far more parameters than X has numbers; the loss falls without bound (3897 -> -2737 in 20
# iterations at m8_n8_k64) and from about iteration 12 every rounding grows tenfold per iteration.  Measured with the
# restatement ALONE (`fastmnmf_trajectory_sensitivity`: the same run from a basis changed by one ulp): the diagonaliser
# after 20 iterations moves by 1.6e-5 (m7_n7_k33) and 6.1e-5 (m8_n8_k64), after 10 by less than 1e-12; restatement
# against reference differs by 2.6e-5 and 4.0e-5, the same size.  No other F in 5..9 and T within the size limit is
# better at m8_n8_k64 (nine combinations tried: 2e-7 .. 4e-4).  So for these fixtures the state and the loss up to
# iteration 10 are held to the usual tolerances, and what comes later to 256 x the measured sensitivity, which is weak
# and says so.  tests/test_fastmnmf_cpu.py asserts that exactly the fixtures listed here are ill-conditioned.
FASTMNMF_ILL_CONDITIONED = ("fastmnmf_m7_n7_k33", "fastmnmf_m8_n8_k64")
LAST_STABLE_ITERATION = 10
FASTMNMF_ATTRS = ("basis", "activation", "spatial_covariance", "diagonalizer")


def fastmnmf_trajectory_sensitivity(g, n_iter=20):
    """The restatement run from W0 against the same run from W0 with every entry times 1 + s * 2^-52, s in {-1, 0, 1}:
    ({attribute: global rel after n_iter iterations, "output": ..}, per-iteration loss difference over max |loss|)."""
    normalize = str(g["normalize"]) or False
    rng = np.random.default_rng(0)
    Y1, l1, s1 = fm.run(g["X"], g["W0"], g["H0"], n_iter, normalize=normalize)
    Y2, l2, s2 = fm.run(g["X"], perturb(g["W0"], rng, U64), g["H0"], n_iter, normalize=normalize)
    d = {a: rel(s2[a], s1[a]) for a in FASTMNMF_ATTRS}
    d["output"] = rel(Y2, Y1)
    return d, np.abs(np.asarray(l2) - np.asarray(l1)) / np.max(np.abs(l1))
