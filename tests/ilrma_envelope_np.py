"""Host side of the Gauss-ILRMA / AuxIVA envelope sweeps (tests/test_gpu_ilrma_envelope.py,
tests/test_gpu_auxiva_envelope.py, tests/test_ilrma_envelope_cpu.py, tools/ilrma_tolerance_probe.py): the grids, the
seeded states, one dict of float64 outputs per state computed with oracle/oracle_np.py (every output from the ENTRY
state, nothing chained), and the measured tolerances.  NumPy only.  The metrics, `perturb`, `sensitivity` and the
256 x d rule are the ones of tests/envelope_np.py, imported, not copied.

States.  X = A_f S with S white complex Gaussian and A_f = I + (MIX / sqrt(M)) x complex Gaussian, multiplied by a
per-bin scale that spans 60 dB (logspace(0, -3, F), shuffled by the seed: real spectrograms are not flat, and a global
metric cannot see the quiet bins); W = (I + (0.3 / sqrt(M)) x complex Gaussian) / (the bin's scale), the size the rows
of a bin have after any IP sweep (w U w^H = 1 with U of the bin's scale squared) -- with rows of the entry size next
to swept rows a thousand times larger, cond(W U) inside the Gauss-Seidel sweep reached 6.7e4 at the quiet bins and no
mixing strength MIX could hold the cap below; Tb, V and the explicit covariance weights uniform in [0.05, 1.05]; a
complex Gaussian projection-back scale for `demix_scaled`.  AuxIVA states carry the oracle's `auxiva_weights` of
(X, W) as the input of the spatial updates.  A float32 state is the float64 one rounded to float32; the reference
always runs in float64 on the rounded state.

Conditions (asserted per case by `ilrma_case` / `auxiva_case`): every denominator the oracle clamps at eps stays above
1e-6; every cond(W_f U_nf) that the IP and IP2 sweeps compare with their threshold is below COND_MAX = 1e3 -- or, for
the cases with T < M only, beyond threshold x 1e3, where the reference keeps every row and W must come back unchanged;
every ISS denominator stays above 1e-6 of its bin's scale.  The largest cond(W U) of the two grids is 1.5e2
(MAX_COND_MEASURED, printed by the probe), so W after a sweep shares ONE bound over all the cond-capped cases.

The cases with T < M (FEW_FRAMES: T = 1 at M = 2, T = 2 at M = 3; no other case has T < 2 M).  Their weighted
covariances have rank T < M, so
  * IP and IP2 reject every row in float64 (cond >= 1e16 against a threshold of 1e12): W unchanged, bit for bit, and
    the status word says so (ASSX_STATUS_COND_REJECT; whether the elimination also meets an exact zero pivot is a
    rounding accident -- numpy.linalg.solve itself raises "Singular matrix" on the AuxIVA state m3_f70_t2 and not on
    m2_f3_t1 -- so the references of these cases come from the cond alone, not from a solve, and the tests do not
    look at ASSX_STATUS_SINGULAR there).  In float32 a rank-deficient W U has a computed cond of about 2^23 < 1e12 and
    cannot be told from a regular one, so the float32 runs of these cases drop W of the IP / IP2 sweeps and the power
    bins read off that W, and keep U and every other output;
  * the ISS sweep and projection back are ill-posed in the reference itself: the sweep removes from every row of Y
    its component along the steered one, and in a frame space of T < M dimensions the later rows have little or
    nothing left, so the denominators w U w^H that follow are differences of nearly equal numbers (measured, relative
    to T x the bin's mean |x|^2: 1.9e-32 at T = 1, where it is 0 / 0 up to rounding, and 1.4e-7 .. 2.6e-5 at T = 2,
    against 7.5e-4 or more in every other ILRMA case); and Y Y^H (M x M of rank T, cond 7e15 or more) has no inverse.
    `spatial_iss_W`, `pb_scale_*` and `normalize_pb_*` do not exist for these cases.
No case has a tolerance of its own: where the reference is defined at all, the tables below hold for every case.

Tolerances.  D_ILRMA / D_AUXIVA are the output of `python tools/ilrma_tolerance_probe.py`: the largest entry-wise
change of each output kind over the whole grid when every real and imaginary part of the state is multiplied by
1 + s u, s in {-1, 0, 1}, u = 2^-52 (float64) or 2^-23 (float32-rounded state), rounded up to two digits.  The bound
of a test is `tolerance(d)` = max(256 d, floor), the rule of tests/envelope_np.py.
"""
import functools

import numpy as np

from envelope_np import (FACTOR, FLOOR32, FLOOR64, METRIC, U32, U64, block, elem, entrywise, perturb,  # noqa: F401
                         reference_ids, round_to_float32, sensitivity, tolerance)
from oracle import oracle_np as orc

EPS = orc.EPS
THRESHOLD = orc.THRESHOLD
MIX = 0.3            # A_f = I + MIX / sqrt(M) x complex Gaussian
MIN_DENOMINATOR = 1e-6
COND_MAX = 1e3
COND_FAR = 1e3
MAX_COND_MEASURED = 1.5e2  # the largest cond(W_f U_nf) over both grids and both dtypes (the probe prints it)

# ---------------------------------------------------------------------------------------------------------- grids
# name: (M, K, domain, F, T, seeds); more than one seed = one batched call with that many different states
ILRMA_GRID = {
    "m2_k1_d2_f3_t1": (2, 1, 2, 3, 1, (101,)),
    "m2_k2_d2_f1_t64": (2, 2, 2, 1, 64, (102,)),
    "m2_k4_d1_f9_t63": (2, 4, 1, 9, 63, (103,)),
    "m2_k5_d2_f17_t65": (2, 5, 2, 17, 65, (104,)),
    "m2_k64_d2_f8_t130": (2, 64, 2, 8, 130, (105,)),
    "m3_k2_d2_f70_t2": (3, 2, 2, 70, 2, (106,)),
    "m3_k4_d15_f7_t33": (3, 4, 1.5, 7, 33, (107,)),
    "m3_k8_d1_f16_t577": (3, 8, 1, 16, 577, (108,)),
    "m3_k16_d2_f33_t32": (3, 16, 2, 33, 32, (109,)),
    "m3_k33_d2_f3_t1030": (3, 33, 2, 3, 1030, (110,)),
    "m4_k4_d2_f17_t1030": (4, 4, 2, 17, 1030, (111,)),
    "m4_k5_d15_f9_t130": (4, 5, 1.5, 9, 130, (112,)),
    "m4_k9_d2_f8_t31": (4, 9, 2, 8, 31, (113,)),
    "m4_k12_d2_f16_t64": (4, 12, 2, 16, 64, (114,)),
    "m4_k13_d2_f7_t65": (4, 13, 2, 7, 65, (115,)),
    "m4_k16_d2_f3_t63": (4, 16, 2, 3, 63, (116,)),
    "m4_k17_d2_f9_t577": (4, 17, 2, 9, 577, (117,)),
    "m4_k32_d2_f17_t33": (4, 32, 2, 17, 33, (118,)),
    "m4_k33_d2_f8_t130": (4, 33, 2, 8, 130, (119,)),
    "m4_k64_d2_f9_t65": (4, 64, 2, 9, 65, (120,)),
    "m4_k65_d2_f7_t64": (4, 65, 2, 7, 64, (121,)),
    # cov_wide_kernel's tile: CovWideGeom<R, 1>::lds_bytes(M K) = 2 x roundup(M K, 64 / LPR) x 64 sizeof(R) + 8 M K
    # sizeof(R) = 1088 M K bytes in float64, 544 M K in float32 (M K a multiple of 4).  M K = 4 x 70 = 280 gives
    # 304 640 and 152 320 bytes, both over 144 KiB = 147 456: the variance-map fallback runs in both precisions.
    # (M K = 256 and 260, the two cases above, fall back in float64 only; M K <= 135 fits in both.)
    "m4_k70_d1_f8_t130": (4, 70, 1, 8, 130, (122,)),
    "m5_k5_d2_f9_t65": (5, 5, 2, 9, 65, (123,)),
    "m5_k16_d2_f16_t63": (5, 16, 2, 16, 63, (124,)),
    "m6_k17_d2_f7_t130": (6, 17, 2, 7, 130, (125,)),
    "m6_k4_d1_f33_t32": (6, 4, 1, 33, 32, (126,)),
    "m7_k32_d2_f8_t64": (7, 32, 2, 8, 64, (127,)),
    "m7_k2_d2_f3_t577": (7, 2, 2, 3, 577, (128,)),
    "m8_k64_d2_f9_t130": (8, 64, 2, 9, 130, (129,)),
    "m8_k8_d15_f17_t31": (8, 8, 1.5, 17, 31, (130,)),
    "m9_k4_d2_f7_t65": (9, 4, 2, 7, 65, (131,)),
    "m17_k5_d2_f3_t130": (17, 5, 2, 3, 130, (132,)),
    "m32_k2_d2_f3_t130": (32, 2, 2, 3, 130, (133,)),
    "m4_k4_d2_f9_t63_b3": (4, 4, 2, 9, 63, (134, 135, 136)),
    "m3_k10_d2_f7_t577_b3": (3, 10, 2, 7, 577, (137, 138, 139)),
}
# name: (M, F, T, seeds)
AUXIVA_GRID = {
    "m2_f3_t1": (2, 3, 1, (201,)),
    "m2_f1_t64": (2, 1, 64, (202,)),
    "m3_f70_t2": (3, 70, 2, (203,)),
    "m3_f9_t63": (3, 9, 63, (204,)),
    "m4_f33_t1030": (4, 33, 1030, (205,)),
    "m4_f8_t31": (4, 8, 31, (206,)),
    "m5_f7_t130": (5, 7, 130, (207,)),
    "m6_f16_t32": (6, 16, 32, (208,)),
    "m7_f3_t577": (7, 3, 577, (209,)),
    "m8_f17_t33": (8, 17, 33, (210,)),
    "m9_f8_t64": (9, 8, 64, (211,)),
    "m17_f3_t130": (17, 3, 130, (212,)),
    "m32_f3_t65": (32, 3, 65, (213,)),
    "m4_f9_t65_b3": (4, 9, 65, (214, 215, 216)),
}
# the cases with T < 2 M, by name (all of them have T < M: see the module docstring)
FEW_FRAMES = ("m2_k1_d2_f3_t1", "m3_k2_d2_f70_t2")
AUXIVA_FEW_FRAMES = ("m2_f3_t1", "m3_f70_t2")
# the streaming entry points are run once more on these with the flat partitions squeezed into 3 workgroups
ILRMA_STREAM_CASES = ("m2_k4_d1_f9_t63", "m2_k5_d2_f17_t65", "m3_k8_d1_f16_t577", "m4_k4_d2_f17_t1030",
                      "m4_k4_d2_f9_t63_b3", "m3_k10_d2_f7_t577_b3")
AUXIVA_STREAM_CASES = ("m3_f9_t63", "m4_f33_t1030", "m4_f9_t65_b3")
KINDS = ("laplace", "gauss")
NMF_HALF_SUMS_MAX_K = 64  # assx_nmf_half_sums: n_basis <= 64 (include/assx.h)

# ---------------------------------------------------------------------------------------------------------- measured
# Output of `python tools/ilrma_tolerance_probe.py`: the largest d over the grid per output kind, rounded up to two
# digits.  Kinds: U = cov_* (explicit weights), ip_U = the covariance of the spatial update (weights (Tb V)^(2/domain):
# more rounded inputs per term); Tb / scaled_W = source update, applied sums, power normalisation; pb_Tb / pb_W / scale
# = projection back (a Gram inverse: they carry cond(Y Y^H)); power_map = |y|^2 element by element, where y = sum_m
# w_m x_m cancels to 1e-3 of its terms somewhere in 2e5 entries; ip2_W carries the 2 x 2 eigenproblem's gap.
D_ILRMA = {
    "float64": {"Tb": 1.6e-15, "U": 1.1e-15, "V": 1.8e-15, "demix": 2.2e-15, "ip2_W": 6.1e-13, "ip_U": 1.1e-15,
                "ip_W": 4.0e-15, "iss_W": 7.4e-15, "loss": 3.6e-15, "pb_Tb": 9.6e-14, "pb_W": 5.9e-14,
                "power": 9.2e-16, "power_bins": 4.9e-15, "power_map": 1.5e-13, "scale": 4.0e-14, "scaled_W": 7.0e-16,
                "sums": 3.2e-15},
    "float32": {"Tb": 9.6e-07, "U": 3.6e-07, "V": 8.3e-07, "demix": 1.2e-06, "ip2_W": 3.5e-06, "ip_U": 4.8e-07,
                "ip_W": 3.3e-07, "iss_W": 4.6e-07, "loss": 1.8e-06, "pb_Tb": 5.6e-06, "pb_W": 4.6e-06,
                "power": 2.5e-07, "power_bins": 1.8e-06, "power_map": 1.3e-04, "scale": 1.5e-06, "scaled_W": 2.1e-07,
                "sums": 1.7e-06},
}
D_AUXIVA = {
    "float64": {"ip2_W": 2.8e-13, "ip_W": 2.8e-15, "iss_W": 6.4e-15, "loss": 4.2e-16, "weights": 2.5e-15},
    "float32": {"ip2_W": 2.7e-06, "ip_W": 2.6e-07, "iss_W": 2.7e-07, "loss": 4.7e-08, "weights": 1.4e-06},
}


def cov_wide_lds_bytes(NK, dtype="float64"):
    """CovWideGeom<R, 1>::lds_bytes(NK) of csrc/assx_cov_wide.hpp."""
    size = 8 if dtype == "float64" else 4
    row_bytes = 64 * size
    rpi = 64 // (row_bytes // 16)
    return 2 * ((NK + rpi - 1) // rpi * rpi) * row_bytes + 8 * NK * size


COV_WIDE_LDS_LIMIT = 144 * 1024


def few_frames(case):
    g = ILRMA_GRID.get(case) or AUXIVA_GRID[case]
    M, T = g[0], g[-2]
    return T < 2 * M


def ilrma_kind(output):
    if output.startswith("cov_"):
        return "U"
    if output.startswith("demix_power") or output == "power_from_cov":
        return "power"
    if output.startswith("demix"):
        return "demix"
    if output.startswith("pb_scale"):
        return "scale"
    if output.startswith("half_sums") or output.startswith("ordered_sum"):
        return "sums"
    if output.startswith("spatial_ip2_W"):
        return "ip2_W"
    return {"power_map": "power_map", "source_Tb": "Tb", "source_V": "V", "source_loss_prev": "loss", "loss": "loss",
            "spatial_ip_U": "ip_U", "spatial_ip_W": "ip_W", "spatial_iss_W": "iss_W",
            "spatial_ip_power_bins": "power_bins", "normalize_bins_W": "scaled_W", "normalize_pb_W": "pb_W",
            "normalize_bins_Tb": "Tb", "normalize_pb_Tb": "pb_Tb", "apply_sums": "Tb"}[output]


def auxiva_kind(output):
    """weights_laplace -> weights; spatial_ip2_W_0_gauss -> ip2_W; ..."""
    for head, kind in (("weights", "weights"), ("loss", "loss"), ("spatial_ip2_W", "ip2_W"), ("spatial_ip_W", "ip_W"),
                       ("spatial_iss_W", "iss_W")):
        if output.startswith(head):
            return kind
    raise KeyError(output)


# this module's kinds join the table that envelope_np.entrywise (and so `sensitivity`) looks kinds up in; "loss" is the
# one name both have, with the same metric
ILRMA_METRIC = {
    "Tb": elem, "pb_Tb": elem, "V": elem, "power_map": elem, "power": elem, "power_bins": elem, "weights": elem,
    "sums": elem, "loss": elem,
    "U": lambda a, b: block(a, b, 2),          # (N, F, M, M): per (n, f) matrix
    "ip_U": lambda a, b: block(a, b, 2),
    "ip_W": lambda a, b: block(a, b, 1),       # (F, N, M): per (f, n) row
    "iss_W": lambda a, b: block(a, b, 1),
    "ip2_W": lambda a, b: block(a, b, 1),
    "scaled_W": lambda a, b: block(a, b, 1),
    "pb_W": lambda a, b: block(a, b, 1),
    "demix": lambda a, b: block(a, b, 1),      # (N, F, T): per (n, f) row
    "scale": lambda a, b: block(a, b, 1),      # (N, F): per n
}
assert all(METRIC[k] is f for k, f in ILRMA_METRIC.items() if k in METRIC)
METRIC.update(ILRMA_METRIC)


def ilrma_tolerance(output, dtype="float64"):
    return tolerance(D_ILRMA[dtype][ilrma_kind(output)], FLOOR64 if dtype == "float64" else FLOOR32)


def auxiva_tolerance(output, dtype="float64"):
    return tolerance(D_AUXIVA[dtype][auxiva_kind(output)], FLOOR64 if dtype == "float64" else FLOOR32)


# ---------------------------------------------------------------------------------------------------------- states
def _cgauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _uniform(rng, shape):
    return 0.05 + rng.random(shape)


def bin_scales(F, seed):
    """60 dB over the bins, in an order that depends on the seed."""
    return np.random.default_rng(seed + 7919).permutation(np.logspace(0, -3, F))


def _mixture_and_filters(rng, M, F, T, seed):
    S = _cgauss(rng, (M, F, T))
    A = np.eye(M) + MIX / np.sqrt(M) * _cgauss(rng, (F, M, M))
    scale = bin_scales(F, seed)
    X = np.einsum("fmn,nft->mft", A, S) * scale[None, :, None]
    W = (np.eye(M) + 0.3 / np.sqrt(M) * _cgauss(rng, (F, M, M))) / scale[:, None, None]
    return X, W


ILRMA_FIELDS = ("X", "W", "Tb", "V", "scale", "r_nt", "r_nft", "sum_weights")


def ilrma_state(M, K, F, T, seed):
    """(X, W, Tb, V, scale, r_nt, r_nft, sum_weights): see the module docstring; `scale` (M, F) complex for
    demix_scaled, r_nt (M, T) / r_nft (M, F, T) the explicit covariance weights, sum_weights (M,) for ordered_sum."""
    rng = np.random.default_rng(seed)
    X, W = _mixture_and_filters(rng, M, F, T, seed)
    Tb, V = _uniform(rng, (M, F, K)), _uniform(rng, (M, K, T))
    return X, W, Tb, V, _cgauss(rng, (M, F)), _uniform(rng, (M, T)), _uniform(rng, (M, F, T)), _uniform(rng, (M,))


AUXIVA_FIELDS = ("X", "W", "r_laplace", "r_gauss")


def auxiva_state(M, F, T, seed):
    """(X, W, r_laplace, r_gauss): the weights are the oracle's `auxiva_weights` of W X."""
    rng = np.random.default_rng(seed)
    X, W = _mixture_and_filters(rng, M, F, T, seed)
    Y = orc.separate(X, W)
    return X, W, orc.auxiva_weights(Y, "laplace"), orc.auxiva_weights(Y, "gauss")


def ilrma_states(case, dtype="float64"):
    M, K, _, F, T, seeds = ILRMA_GRID[case]
    states = [ilrma_state(M, K, F, T, s) for s in seeds]
    return [round_to_float32(s) for s in states] if dtype == "float32" else states


def auxiva_states(case, dtype="float64"):
    M, F, T, seeds = AUXIVA_GRID[case]
    states = [auxiva_state(M, F, T, s) for s in seeds]
    return [round_to_float32(s) for s in states] if dtype == "float32" else states


# ---------------------------------------------------------------------------------------------------------- pieces
def _floored(a, eps=EPS):
    return np.maximum(a, eps)


def bin_power(C, W):
    """pb[n, f] = w_nf C_f w_nf^H, the per-bin share of the power statistic (C (F, M, M), W (F, N, M))."""
    return np.einsum("fnm,fmk,fnk->nf", W, C, W.conj()).real


def iss_filters(X, W, R):
    """The ISS sweep of oracle_np.iss_update carried on the filters (Y = W X is linear in W, so the rank-one update of
    Y is the same update of W); no least-squares rebuild, which needs T >= M.  Returns (W, smallest w U w^H relative to
    T x the bin's mean |x|^2).  tests/test_ilrma_envelope_cpu.py checks W X against oracle_np.iss_update itself."""
    W = W.copy()
    Y = orc.separate(X, W)
    Rb = R if R.ndim == 3 else R[:, None, :]
    scale = X.shape[2] * np.mean(np.abs(X) ** 2, axis=(0, 2))
    low = np.inf
    with np.errstate(all="ignore"):
        for n in range(Y.shape[0]):
            U_n = np.sum(Y * Y[n].conj() / Rb, axis=2)
            D_n = np.sum(np.abs(Y[n]) ** 2 / Rb, axis=2)
            low = min(low, float(np.min(D_n / scale)))
            V_n = U_n / D_n
            V_n[n] = 1 - 1 / np.sqrt(D_n[n])
            W = W - V_n.T[:, :, None] * W[:, n, None, :]
            Y = Y - V_n[:, :, None] * Y[n]
    return W, low


def ip_conds(W, U, rejected):
    """(cond(W_f U_nf) as the Gauss-Seidel sweep of oracle_np.ip_update meets them, W after the sweep): source n sees
    the rows of the sources before it already updated (the replay is checked against oracle_np.ip_update by `_sweeps`).
    rejected = True (T < M): every row stays, so every source sees the entry W."""
    F, N, M = W.shape
    W = W.copy()
    conds = np.empty((N, F))
    with np.errstate(all="ignore"):
        for n in range(N):
            WU = W @ U[n]
            conds[n] = np.linalg.cond(WU)
            if not rejected:
                w = np.linalg.solve(WU, np.broadcast_to(np.eye(M)[:, n, None], (F, M, 1)))[..., 0]
                W[:, n, :] = w.conj() / np.sqrt(np.einsum("fi,fij,fj->f", w.conj(), U[n], w))[:, None]
    return conds, W


def _assert_conds(case, conds, rejected, threshold=THRESHOLD):
    if rejected:
        assert conds.min() > threshold * COND_FAR, "%s: cond(W U) = %.3e is near the threshold" % (case, conds.min())
    else:
        assert conds.max() < COND_MAX, "%s: cond(W U) = %.3e" % (case, conds.max())


def _sweeps(X, W, U, R, pairs, rejected, prefix="spatial_", suffix=""):
    """IP, ISS and IP2 of the entry W with the covariances U (N, F, M, M) and the (floored) ISS weights R; the largest
    regular cond and the smallest ISS denominator ride along under "_cond" / "_iss_low"."""
    out = {}
    c, replay = ip_conds(W, U, rejected)
    conds = [c]
    if rejected:
        out[prefix + "ip_W" + suffix] = W.copy()
        out["_iss_low" + suffix] = iss_filters(X, W, R)[1]  # for the record: see the module docstring
    else:
        out[prefix + "ip_W" + suffix], mask = orc.ip_update(W.copy(), U)
        assert mask.all() and np.allclose(replay, out[prefix + "ip_W" + suffix], rtol=1e-9, atol=0)
        out[prefix + "iss_W" + suffix], out["_iss_low" + suffix] = iss_filters(X, W, R)
    for i, (m, n) in enumerate(pairs):
        with np.errstate(all="ignore"):
            conds.append(np.stack([np.linalg.cond(W @ U[m]), np.linalg.cond(W @ U[n])]))
        if rejected:
            out[prefix + "ip2_W_%d" % i + suffix] = W.copy()
        else:
            out[prefix + "ip2_W_%d" % i + suffix], cm, cn = orc.ip2_update(W.copy(), U[m], U[n], m, n)
            assert cm.all() and cn.all()
    out["_cond" + suffix] = np.concatenate([c.ravel() for c in conds])
    return out


def ip2_pairs(M):
    return ((0, 1), (M - 1, 0))


# ---------------------------------------------------------------------------------------------------------- references
def ilrma_reference(state, domain=2):
    """Every ILRMA output from ONE entry state (not chained): demix, demix_scaled, power_map, cov_{nt,nft,none},
    source_{Tb,V,loss_prev}, loss, spatial_ip_{U,W,power_bins}, spatial_iss_W, spatial_ip2_W_{0,1} for `ip2_pairs(M)`,
    demix_power, power_from_cov, normalize_bins_{W,Tb}, normalize_pb_{W,Tb}, pb_scale_<ref> for `reference_ids(M)`,
    half_sums_{basis,act}, apply_sums, ordered_sum, ordered_sum_weighted.  Keys with a leading underscore are host-side
    extras: inputs of single entry points and the figures the case conditions are asserted on."""
    X, W, Tb, V, scale, r_nt, r_nft, sw = state
    M, F, T = X.shape
    K = Tb.shape[-1]
    d = domain
    rejected = T < M
    Y = orc.separate(X, W)
    P = np.abs(Y) ** 2
    out = dict(demix=Y, demix_scaled=Y * scale[..., None], power_map=P)
    out["cov_nt"] = orc.weighted_covariance(X, r_nt)
    out["cov_nft"] = orc.weighted_covariance(X, r_nft)
    out["cov_none"] = orc.weighted_covariance(X, np.ones((1, T)))
    C = out["cov_none"][0]
    out["source_Tb"], out["source_V"] = orc.ilrma_source_update(P, Tb.copy(), V.copy(), d)
    out["loss"] = out["source_loss_prev"] = np.float64(orc.ilrma_loss(X, W, Tb, V, d))
    R = _floored(orc.ilrma_variance(Tb, V, d))
    U = out["spatial_ip_U"] = orc.weighted_covariance(X, R)
    out.update(_sweeps(X, W, U, R, ip2_pairs(M), rejected))
    out["spatial_ip_power_bins"] = bin_power(C, out["spatial_ip_W"])
    out["demix_power"] = P.mean(axis=(1, 2))
    pb = bin_power(C, W)
    out["power_from_cov"] = pb.mean(axis=1)
    out["_power_bins_in"] = pb  # the input of assx_ilrma_normalize_power_bins
    out["normalize_bins_W"], out["normalize_bins_Tb"] = orc.ilrma_normalize(X, W, Tb, "power", d)
    if not rejected:
        out["normalize_pb_W"], out["normalize_pb_Tb"] = orc.ilrma_normalize(X, W, Tb, "projection-back", d, EPS, 0)
        for r in reference_ids(M):
            out["pb_scale_%d" % r] = orc.projection_back(Y, X[r])
    # IS-MM halves on the power map, stopped before they are applied (the first lines of oracle_np.ilrma_source_update)
    TV = _floored(Tb @ V)
    division, TVinv = P / TV ** ((d + 2) / d), 1 / TV
    Vt, Tt = V.transpose(0, 2, 1), Tb.transpose(0, 2, 1)
    basis = np.stack([division @ Vt, TVinv @ Vt])                  # (2, N, F, K)
    out["apply_sums"] = Tb * (basis[0] / _floored(basis[1])) ** (d / (d + 2))
    if K <= NMF_HALF_SUMS_MAX_K:
        out["half_sums_basis"] = basis
        out["half_sums_act"] = np.stack([Tt @ division, Tt @ TVinv])   # (2, N, K, T), with the entry basis
    out["_apply_sums_in"] = basis
    total, wtotal = np.zeros((F, T)), np.zeros((F, T))
    for n in range(M):  # ascending order, as assx_ordered_sum adds
        total = total + P[n]
        wtotal = wtotal + sw[n] * P[n]
    out["ordered_sum"], out["ordered_sum_weighted"] = total, wtotal
    dens = [TV.min(), basis[1].min(), _floored((out["source_Tb"] @ V)).min(),
            (out["source_Tb"].transpose(0, 2, 1) @ (1 / _floored(out["source_Tb"] @ V))).min(),
            orc.ilrma_variance(Tb, V, d).min(), r_nt.min(), r_nft.min(), np.sqrt(out["demix_power"]).min()]
    out["_min_denominator"] = float(min(dens))
    return out


def auxiva_reference(state):
    """weights_<kind>, loss_<kind> of (X, W); spatial_{ip,iss}_W_<kind>, spatial_ip2_W_<i>_<kind> with the state's
    weights, for both kinds."""
    X, W, r_l, r_g = state
    M, F, T = X.shape
    rejected = T < M
    Y = orc.separate(X, W)
    out = {"_min_denominator": float(min(r_l.min(), r_g.min()))}
    for kind, r in zip(KINDS, (r_l, r_g)):
        out["weights_" + kind] = orc.auxiva_weights(Y, kind)
        out["loss_" + kind] = np.float64(orc.auxiva_loss(X, W, kind))
        R = _floored(r)
        out.update(_sweeps(X, W, orc.weighted_covariance(X, R), R, ip2_pairs(M), rejected, suffix="_" + kind))
    return out


def public(ref):
    """The outputs of a reference dict without the host-side extras (keys that start with an underscore)."""
    return {k: v for k, v in ref.items() if not k.startswith("_")}


def _conditions(case, ref, rejected):
    assert ref["_min_denominator"] > MIN_DENOMINATOR, \
        "%s: a denominator of %.3e is too close to the eps clamp" % (case, ref["_min_denominator"])
    for k, v in ref.items():
        if k.startswith("_cond"):
            _assert_conds(case, v, rejected)
        elif k.startswith("_iss_low"):
            assert v > MIN_DENOMINATOR or rejected, "%s: an ISS denominator of %.3e of its bin's scale" % (case, v)
    assert all(np.all(np.isfinite(v)) for v in public(ref).values()), case


@functools.lru_cache(maxsize=None)
def ilrma_case(case, dtype="float64"):
    """(states, references) of a grid case, with the host-side conditions asserted."""
    M, K, domain, F, T, _ = ILRMA_GRID[case]
    states = ilrma_states(case, dtype)
    refs = [ilrma_reference(s, domain) for s in states]
    for r in refs:
        _conditions(case, r, T < M)
    return states, refs


@functools.lru_cache(maxsize=None)
def auxiva_case(case, dtype="float64"):
    M, F, T, _ = AUXIVA_GRID[case]
    states = auxiva_states(case, dtype)
    refs = [auxiva_reference(s) for s in states]
    for r in refs:
        _conditions(case, r, T < M)
    return states, refs


def max_cond(refs):
    """The largest regular cond(W U) among reference dicts (0 for a T < M case)."""
    c = [v.max() for r in refs for k, v in r.items() if k.startswith("_cond") and v.max() < THRESHOLD]
    return float(max(c)) if c else 0.0


# ---------------------------------------------------------------------------------------------------------- probe
def perturb_state(state, rng, u):
    return tuple(perturb(a, rng, u) for a in state)


def ilrma_sensitivity(state, domain=2, u=U64, draws=3, seed=0):
    return sensitivity(lambda s: public(ilrma_reference(s, domain)), perturb_state, ilrma_kind, state, u, draws, seed)


def auxiva_sensitivity(state, u=U64, draws=3, seed=0):
    return sensitivity(lambda s: public(auxiva_reference(s)), perturb_state, auxiva_kind, state, u, draws, seed)
