"""Host side of the beamformer / PCA / MDP envelope sweep (tests/test_gpu_beamform_envelope.py,
tools/beamform_tolerance_probe.py): the grid, the seeded state, the restatement's outputs per entry point, and the
measured tolerances.  The metrics, the perturbation and the rule 256 * d with a floor of 1e-13 are those of
tests/envelope_np.py, imported as they are.  NumPy only; nothing here touches a GPU.

Grid: every M in 2..8, N in {1, M - 1, M, 8}, F in {1, 3, 17}, and nine frame counts around the wave (63, 64, 65), the
workgroup (255, 256, 257) and the MDP pass's frame-chunk seam (FRAME_CHUNK - 1, + 0, + 1; FRAME_CHUNK follows the
library's named constant).  A state is checked here for the conditions under which two correct implementations agree
to rounding: every bin's smallest eigenvalue gap is at least 1e-3 of its largest eigenvalue and T >= 4 M (the fixtures'
condition for comparing PCA component by component), and no ML denominator lies near the floor.  T = 1 (TINY) is
compared on invariants only.
"""
import functools

import numpy as np

import envelope_np as env
import beamform_np as bf

try:
    from audio_source_separation_amd._lib import BF_FRAME_CHUNK as FRAME_CHUNK
except Exception:  # the probe may run where the library is not built; tests/test_beamform_cpu.py pins the two together
    FRAME_CHUNK = 1024

CHANNELS = (2, 3, 4, 5, 6, 7, 8)
BINS = (1, 3, 17)
FRAMES = (63, 64, 65, 255, 256, 257, FRAME_CHUNK - 1, FRAME_CHUNK, FRAME_CHUNK + 1)


def sources(M):
    return tuple(sorted({1, M - 1, M, 8}))


GRID = {"m%d_n%d_f%d_t%d" % (M, N, F, T): (M, N, F, T, 20000 + 1000 * M + 100 * a + 10 * i + j)
        for M in CHANNELS for a, N in enumerate(sources(M)) for i, F in enumerate(BINS) for j, T in enumerate(FRAMES)}
TINY = {"m%d_n%d_f3_t1" % (M, N): (M, N, 3, 1, 29000 + 10 * M + N) for M in CHANNELS for N in sources(M)}

# output of `reference` -> kind (the metric and the tolerance it is held to)
OUTPUTS = {"ds_W": "filter", "ds_s": "filter", "ds": "output", "ml_W": "filter", "ml": "output", "mvdr": "output",
           "pca_V": "basis", "pca_w": "eigenvalue", "pca": "component", "mdp": "scale", "mdp1": "scale"}
MIN_GAP = 1e-3
MIN_DENOMINATOR = 1e-6

# ---------------------------------------------------------------------------------------------------------- measured
# Output of `python tools/beamform_tolerance_probe.py`: the largest d over the grid per kind, rounded up to two digits.
# filter, basis: per bin, the largest entry difference over the bin's largest entry; output, component: the same per
# (source, bin) row of frames; eigenvalue: per bin over the bin's largest; scale: per (channel, source) row of bins.
# Worst cases: m8_n7_f17_t1025 ml for output, m6_n6_f17_t256 ml_W for filter, m8_n7_f3_t65 pca_V for basis,
# m8_n8_f17_t65 pca for component, m6_n6_f17_t257 pca_w for eigenvalue, m5_n5_f1_t1024 mdp for scale.
D = {
    "filter": 2.4e-15,
    "output": 4.0e-15,
    "basis": 1.9e-13,
    "eigenvalue": 1.8e-15,
    "component": 5.9e-14,
    "scale": 3.8e-14,
}
# The same for the recorded chain (tests/golden/beamform/beamform_m3_n2_f5_t70_chain: PCA, five AuxLaplaceIVA updates,
# projection back), X moved by one rounding, the largest of three draws.
D_CHAIN = 8.6e-15
# The restatement against the reference's recorded outputs (tests/test_beamform_cpu.py): two float64 programs that sum in
# different orders, held to the same tolerances; the largest distances `make_beamform.py` printed are ds 2.2e-16,
# ml 4.1e-16, mvdr 5.2e-16, pca 2.1e-15, eigenvalues 9.1e-16, mdp 7.4e-16, chain 4.6e-16.

METRIC = {"filter": lambda a, b: env.block(a, b, 2), "basis": lambda a, b: env.block(a, b, 2),
          "output": lambda a, b: env.block(a, b, 1), "component": lambda a, b: env.block(a, b, 1),
          "eigenvalue": lambda a, b: env.block(a, b, 1), "scale": lambda a, b: env.block(a, b, 1),
          "chain": lambda a, b: env.block(a, b, 1)}


def kind(output):
    return OUTPUTS[output]


def tolerance(output):
    return env.tolerance(D_CHAIN if output == "chain" else D[kind(output)])


def entrywise(k, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.isfinite(a)), "non-finite output"
    return METRIC[k](a, b)


def distance(output, got, ref):
    """The entry-wise distance of one output; PCA components are turned onto the reference's phases first."""
    if output == "pca":
        got = bf.align_phase(got, ref)
    return entrywise("chain" if output == "chain" else kind(output), got, ref)


# ---------------------------------------------------------------------------------------------------------- states
def state(M, N, F, T, seed):
    """(X, A, R, Ys, ref, eps): X complex Gaussian channels scaled by 1 + m; A complex Gaussian over sqrt(M); R a positive
    definite matrix plus a non-Hermitian part; Ys complex Gaussian sources with a scale per (source, bin)."""
    rng = np.random.default_rng(seed)
    X = bf.cgauss(rng, (M, F, T)) * (1.0 + np.arange(M))[:, None, None]
    A = bf.cgauss(rng, (F, M, N)) / np.sqrt(M)
    G = bf.cgauss(rng, (F, M, M))
    R = G @ G.conj().transpose(0, 2, 1) / M + 0.5 * np.eye(M) + 0.1 * bf.cgauss(rng, (F, M, M))
    Ys = bf.cgauss(rng, (N, F, T)) * (0.5 + rng.random((N, F, 1)))
    return X, A, R, Ys, int(rng.integers(0, M)), 1e-12


def reference(st, degenerate=False):
    """Every entry point of beamform_np on ONE state.  degenerate (T < 4 M): no MVDR and no PCA."""
    X, A, R, Ys, ref, eps = st
    out = {"ds_W": A.conj().transpose(0, 2, 1), "ds_s": A[:, ref, :], "ds": bf.delay_sum(X, A, ref),
           "ml_W": bf.ml_filter(A, R, eps), "ml": bf.ml(X, A, R, ref, eps),
           "mdp": bf.mdp(Ys, X), "mdp1": bf.mdp(Ys, X[ref])[None]}
    if not degenerate:
        V, w = bf.pca_basis(X)
        out.update(mvdr=bf.mvdr(X, A, ref, eps), pca_V=V, pca_w=w, pca=bf.project(X, V))
    return out


def check_state(case, st):
    X, A, R, Ys, ref, eps = st
    M, _, T = X.shape
    assert T >= 4 * M and bf.eigen_gap(X) >= MIN_GAP, "%s: eigenvalue gap %.1e" % (case, bf.eigen_gap(X))
    for C in (R, bf.covariance(X)):
        den = np.sum(A.conj() * np.linalg.solve(C, A), axis=1)
        assert den.real.min() >= MIN_DENOMINATOR, "%s: an ML denominator of %.1e" % (case, den.real.min())
    assert np.abs(bf.pca_basis(X)[0][:, 0, :]).min() >= 1e-6, "%s: an eigenvector whose first entry vanishes" % case


@functools.lru_cache(maxsize=None)
def grid_case(case):
    """(state, reference) of a grid case: the first seed from the case's own on whose state meets the host-side
    conditions (a case that misses one takes the next seed; none is skipped)."""
    M, N, F, T, seed = GRID[case]
    for s in range(seed, seed + 1000000, 100000):
        st = state(M, N, F, T, s)
        try:
            check_state(case, st)
            break
        except AssertionError:
            if s + 100000 >= seed + 1000000:
                raise
    ref = reference(st)
    assert all(np.all(np.isfinite(v)) for v in ref.values()), case
    return st, ref


@functools.lru_cache(maxsize=None)
def tiny_case(case):
    st = state(*TINY[case])
    return st, reference(st, degenerate=True)


# ---------------------------------------------------------------------------------------------------------- probe
def perturb_state(st, rng, u):
    X, A, R, Ys, ref, eps = st
    return env.perturb(X, rng, u), env.perturb(A, rng, u), env.perturb(R, rng, u), env.perturb(Ys, rng, u), ref, eps


def sensitivity(st, u=env.U64, draws=3, seed=0):
    """{output: d}: the largest entry-wise difference between reference(state) and reference(perturbed state)."""
    rng = np.random.default_rng(seed)
    base = reference(st)
    d = {k: 0.0 for k in base}
    for _ in range(draws):
        other = reference(perturb_state(st, rng, u))
        for k in base:
            d[k] = max(d[k], distance(k, other[k], base[k]))
    return d


def chain_sensitivity(X, u=env.U64, draws=3, seed=0):
    rng = np.random.default_rng(seed)
    base = bf.chain(X)
    return max(entrywise("chain", bf.chain(env.perturb(X, rng, u)), base) for _ in range(draws))
