"""Host side of the ProxLaplaceIVA envelope sweep (tests/test_gpu_pdsbss_envelope.py, tools/pdsbss_tolerance_probe.py): the
grid, the seeded general state, the restatement's outputs per entry point, and the measured tolerances.  The metrics, the
perturbation and the rule 256 * d with a floor of 1e-13 are those of tests/envelope_np.py, imported as they are.  NumPy
only; nothing here touches a GPU.

Grid: every M in 2..8, F in {1, 3, 17}, and nine frame counts around the wave (63, 64, 65), the workgroup (255, 256, 257) and
sweep 2's frame-chunk seam (FRAME_CHUNK - 1, + 0, + 1; FRAME_CHUNK follows the library's named constant): tails, the slice
sums over the bins, a chunk seam, and the row split at M >= 7.  Every state has a non-trivial W, y and parameters, and a
mu2 of its own, the reciprocal of the median group norm of its z, so that both branches of the shrinkage occur; the
state is checked here for the fixtures' conditions (no group norm within 1e-6 relative of 1 / mu2, sigma_min >= 1e-6
sigma_max for every matrix that goes into the SVD).
"""
import functools

import numpy as np

import envelope_np as env
import pdsbss_np as pd

try:
    from audio_source_separation_amd._lib import PDSBSS_FRAME_CHUNK as FRAME_CHUNK
except Exception:  # the probe may run where the library is not built; tests/test_pdsbss_cpu.py pins the two together
    FRAME_CHUNK = 1024

CHANNELS = (2, 3, 4, 5, 6, 7, 8)
BINS = (1, 3, 17)
FRAMES = (63, 64, 65, 255, 256, 257, FRAME_CHUNK - 1, FRAME_CHUNK, FRAME_CHUNK + 1)
GRID = {"m%d_f%d_t%d" % (M, F, T): (M, F, T, 9000 + 100 * M + 10 * i + j)
        for M in CHANNELS for i, F in enumerate(BINS) for j, T in enumerate(FRAMES)}

# output of `reference` -> kind (the metric and the tolerance it is held to)
OUTPUTS = {"norm": "norm", "adjoint": "G", "prox_logdet": "W", "forward": "y", "prox_group": "y", "update_W": "W",
           "update_y": "y", "loss": "loss"}
MIN_DEN_GAP = 1e-6
MIN_SIGMA_RATIO = 1e-6

# ---------------------------------------------------------------------------------------------------------- measured
# Output of `python tools/pdsbss_tolerance_probe.py`: the largest d over the grid per kind, rounded up to two digits.
# G, W: per bin, the largest entry difference over the bin's largest entry; y: the same per (f, n) row of frames; norm and
# loss relatively.  Worst cases: m2_f3_t64 norm, m2_f17_t255 adjoint, m8_f17_t1023 prox_logdet, m8_f3_t1024 prox_group,
# m3_f1_t63 loss.
D = {
    "norm": 6.2e-16,
    "G": 1.8e-15,
    "W": 5.0e-15,
    "y": 5.2e-14,
    "loss": 4.5e-16,
}
# The same for whole runs (`trajectory_sensitivity` over the recorded cases: 10 iterations from an X, a W0 and a norm moved
# by one rounding), the largest of three draws.  A run is as sensitive as the smallest singular values that its prox
# arguments go through: h(0) > 0, so the prox turns two singular directions s1, s2 near zero with a condition of
# (h(s1) + h(s2)) / (s1 + s2), once per iteration.  The maker keeps every recorded case below 1e-11 for W and y.
# Worst cases: proxlaplaceiva_m3_f4_t70 for W and y, proxlaplaceiva_m5_f3_t48 for the loss, proxlaplaceiva_m3_f4_t50_warm for
# the output.
D_TRAJECTORY = {
    "W": 1.2e-13,
    "y": 1.1e-12,
    "loss": 3.0e-15,
    "output": 7.5e-13,
}
# Distances measured on an MI355X (tests/test_gpu_pdsbss*.py print every one before they assert), the largest over the 189
# grid sizes and the 13 recorded cases, in the same metrics:
#   one call from one state   norm 6.7e-16, adjoint 1.4e-15, prox_logdet 4.9e-15, forward 5.9e-16, prox_group 9.0e-14,
#                             update W 7.1e-15, update y 2.4e-14, loss 4.0e-16
#   whole 10-iteration runs   W 4.7e-13, y 9.0e-13, loss 7.3e-15, output 3.1e-12 (against the reference's recorded runs)

METRIC = {"norm": env.elem, "loss": env.elem, "G": lambda a, b: env.block(a, b, 2), "W": lambda a, b: env.block(a, b, 2),
          "y": lambda a, b: env.block(a, b, 1), "output": lambda a, b: env.block(a, b, 1)}


def kind(output):
    return OUTPUTS[output]


def tolerance(output):
    return env.tolerance(D[kind(output)])


def trajectory_tolerance(what):
    return env.tolerance(D_TRAJECTORY[what])


def entrywise(k, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.isfinite(a)), "non-finite output"
    return METRIC[k](a, b)


# ---------------------------------------------------------------------------------------------------------- states
def state(M, F, T, seed):
    """(X, W, y, norm, par): X complex Gaussian with a per-bin scale; W = I + 0.3 / sqrt(M) x complex Gaussian; y complex
    Gaussian of the size of X / norm; C, mu1, alpha uniform in [0.5, 1.5]; mu2 = 1 / the median group norm of z."""
    rng = np.random.default_rng(seed)
    X = env._cgauss(rng, (M, F, T)) * (0.1 + rng.random((1, F, 1)))
    W = np.eye(M) + 0.3 / np.sqrt(M) * env._cgauss(rng, (F, M, M))
    norm = pd.operator_norm(X)
    y = env._cgauss(rng, (F, M, T)) * (np.sqrt(np.mean(np.abs(X) ** 2)) / norm)
    C, mu1, alpha = (float(v) for v in 0.5 + rng.random(3))
    mu2 = 1.0
    for _ in range(3):  # z depends on mu2 through the prox argument, weakly: a few passes settle it
        den = np.sort(pd.group_norm(pd.update(X / norm, W, y, C, mu1, mu2, alpha)[2]["z"]), axis=None)
        mu2 = float(2.0 / (den[den.size // 2 - 1] + den[den.size // 2]))  # between the two middle values
    return X, W, y, norm, dict(C=C, mu1=mu1, mu2=mu2, alpha=alpha)


def reference(st):
    """Every entry point of pdsbss_np on ONE state (not chained)."""
    X, W, y, norm, par = st
    Xn = X / norm
    Wn, yn, _ = pd.update(Xn, W, y, **par)
    return {"norm": np.float64(pd.operator_norm(X)), "adjoint": pd.adjoint(Xn, y), "prox_logdet": pd.prox_logdet(W, par["mu1"]),
            "forward": pd.forward(Xn, y, W), "prox_group": pd.prox_group(y, 1 / par["mu2"], par["C"]),
            "update_W": Wn, "update_y": yn, "loss": np.float64(pd.loss(X, W, par["C"]))}


def check_state(case, st):
    """The conditions under which two correct implementations agree to rounding: no cell next to the branch point of the
    shrinkage (of the update's z and of the y that prox_group is called on), no SVD argument close to rank-deficient, and
    both branches taken."""
    X, W, y, norm, par = st
    stages = pd.update(X / norm, W, y, **par)[2]
    moved, gap = pd.shrinking(stages["z"], 1 / par["mu2"])
    assert gap >= MIN_DEN_GAP, "%s: a group norm of z within %.1e of 1 / mu2" % (case, gap)
    assert moved.any() and not moved.all(), "%s: one branch of the shrinkage only" % case
    assert pd.shrinking(y, 1 / par["mu2"])[1] >= MIN_DEN_GAP, case
    for A in (W, stages["arg"]):
        sv = np.linalg.svd(A, compute_uv=False)
        assert np.all(sv[:, -1] >= MIN_SIGMA_RATIO * sv[:, 0]), "%s: an SVD argument close to rank-deficient" % case
    return float(moved.mean())


@functools.lru_cache(maxsize=None)
def grid_case(case):
    """(state, reference, share of shrinking cells) of a grid case: the first seed from the case's own on whose state
    meets the host-side conditions (a case that misses one takes the next seed; none is skipped)."""
    M, F, T, seed = GRID[case]
    for s in range(seed, seed + 1000000, 100000):
        st = state(M, F, T, s)
        try:
            share = check_state(case, st)
            break
        except AssertionError:
            if s + 100000 >= seed + 1000000:
                raise
    ref = reference(st)
    assert all(np.all(np.isfinite(v)) for v in ref.values()), case
    return st, ref, share


# ---------------------------------------------------------------------------------------------------------- probe
def perturb_state(st, rng, u):
    X, W, y, norm, par = st
    return (env.perturb(X, rng, u), env.perturb(W, rng, u), env.perturb(y, rng, u),
            float(env.perturb(np.float64(norm), rng, u)), par)


def sensitivity(st, u=env.U64, draws=3, seed=0):
    """{output: d}: the largest entry-wise difference between reference(state) and reference(perturbed state).  The norm
    output is probed through X; the other outputs take the norm as an input that is moved like the rest."""
    rng = np.random.default_rng(seed)
    base = reference(st)
    d = {k: 0.0 for k in base}
    for _ in range(draws):
        other = reference(perturb_state(st, rng, u))
        for k in base:
            d[k] = max(d[k], entrywise(kind(k), other[k], base[k]))
    return d


def trajectory(X, W0, norm, par, n_iter=pd.N_ITER, reference_id=0, projection_back=True):
    states, losses, _ = pd.run(X, W0, n_iter, norm, **par)
    W, y = states[n_iter]
    return {"W": W, "y": y, "loss": np.array(losses), "output": pd.separate(X, W, reference_id, projection_back)}


def trajectory_sensitivity(g, n_iter=pd.N_ITER):
    """The restatement's run of a recorded case against the same run with every real and imaginary part of X and W0, and
    the norm, times 1 + s 2^-52, the largest of three draws: {"W": .., "y": .., "loss": .., "output": ..} in the metrics above."""
    rng = np.random.default_rng(0)
    par, ref, pb = pd.params(g), int(g["reference_id"]), bool(g["projection_back"])
    a = trajectory(g["X"], g["W_0"], float(g["norm"]), par, n_iter, ref, pb)
    d = {k: 0.0 for k in a}
    for s in (1, -1, 0):  # three draws, the norm moved up, down and not at all
        b = trajectory(env.perturb(g["X"], rng, env.U64), env.perturb(g["W_0"], rng, env.U64),
                       float(g["norm"]) * (1 + s * env.U64), par, n_iter, ref, pb)
        d = {k: max(d[k], entrywise(k, b[k], a[k])) for k in a}
    return d
