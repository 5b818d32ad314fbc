"""The host side of the Gauss-ILRMA / AuxIVA envelope sweeps without a GPU (tests/ilrma_envelope_np.py): the grids
cover the dispatch boundaries of csrc/, every case meets its conditions, the committed d tables bound what the probe
measures, and the entry-wise metrics at the new tolerances catch five faults that the Frobenius ratio of the stage
tests (conftest.rel_err at the tolerances of tests/test_gpu_ops.py) lets through."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ilrma_envelope_np as env  # noqa: E402
from conftest import rel_err  # noqa: E402
from oracle import oracle_np as orc  # noqa: E402

DTYPES = ("float64", "float32")
PROBED = ("m2_k1_d2_f3_t1", "m4_k70_d1_f8_t130", "m8_k8_d15_f17_t31")
PROBED_AUXIVA = ("m3_f70_t2", "m6_f16_t32", "m4_f9_t65_b3")


def test_grids_cover_the_dispatch_boundaries():
    G, A = list(env.ILRMA_GRID.values()), list(env.AUXIVA_GRID.values())
    both = [(c[0], c[3], c[4]) for c in G] + [(c[0], c[1], c[2]) for c in A]
    for grid_m in ({c[0] for c in G}, {c[0] for c in A}):
        assert set(range(2, 9)) | {9, 17, 32} <= grid_m
    assert {1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 64, 65} <= {c[1] for c in G}
    for K in (5, 16, 17, 32):
        assert any(c[1] == K and c[0] <= 4 for c in G), K
        assert any(c[1] == K and 5 <= c[0] <= 8 for c in G), K
    # the variance-map fallback behind cov_wide_kernel: a tile over 144 KiB in both precisions, at M <= 4 and K > 16
    assert env.cov_wide_lds_bytes(280, "float64") == 304640 and env.cov_wide_lds_bytes(280, "float32") == 152320
    assert any(c[0] <= 4 and c[1] > 16 and min(env.cov_wide_lds_bytes(c[0] * c[1], d) for d in DTYPES)
               > env.COV_WIDE_LDS_LIMIT for c in G)
    # ... cov_wide_kernel itself (K 17.. with a tile that fits) and cov_mfma_kernel at ceil(K / 4) = 2, 3, 4
    assert any(c[0] <= 4 and c[1] > 16 and env.cov_wide_lds_bytes(c[0] * c[1], "float64") <= env.COV_WIDE_LDS_LIMIT
               for c in G)
    assert {2, 3, 4} <= {(c[1] + 3) // 4 for c in G if c[0] <= 4 and 4 < c[1] <= 16}
    for K_set in ({4}, {c[1] for c in G if c[1] > 4}):
        assert {2, 1, 1.5} <= {c[2] for c in G if c[1] in K_set}
    assert {1, 2, 31, 32, 33, 63, 64, 65, 130, 577, 1030} <= {c[2] for c in both}
    assert {1, 3, 7, 8, 9, 16, 17, 33, 70} <= {c[1] for c in both}
    assert sum(len(c[-1]) == 3 for c in G + A) >= 2 and all(len(c[-1]) in (1, 3) for c in G + A)
    assert all(c[0] * c[1] * c[2] <= 2e5 for c in both)
    seeds = [s for c in G + A for s in c[-1]]
    assert len(set(seeds)) == len(seeds)  # every state has its own seed
    assert 28 <= len(G) <= 36 and 10 <= len(A) <= 14


def test_few_frames_cases_are_the_listed_ones():
    assert tuple(n for n in env.ILRMA_GRID if env.few_frames(n)) == env.FEW_FRAMES
    assert tuple(n for n in env.AUXIVA_GRID if env.few_frames(n)) == env.AUXIVA_FEW_FRAMES
    for n in env.FEW_FRAMES:  # every one of them is on the far side of the condition guard, none in between
        M, _, _, _, T, _ = env.ILRMA_GRID[n]
        assert T < M
    assert set(env.ILRMA_STREAM_CASES) <= set(env.ILRMA_GRID) and set(env.AUXIVA_STREAM_CASES) <= set(env.AUXIVA_GRID)
    assert {63, 65, 577} <= {env.ILRMA_GRID[n][4] for n in env.ILRMA_STREAM_CASES}
    assert any(len(env.ILRMA_GRID[n][5]) == 3 for n in env.ILRMA_STREAM_CASES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(env.ILRMA_GRID))
def test_ilrma_case_meets_its_conditions(case, dtype):
    states, refs = env.ilrma_case(case, dtype)  # asserts the denominators, the conds, the ISS denominators, finiteness
    M, K, domain, F, T, seeds = env.ILRMA_GRID[case]
    assert len(states) == len(refs) == len(seeds)
    assert env.max_cond(refs) <= env.MAX_COND_MEASURED < env.COND_MAX
    for state, ref in zip(states, refs):
        X, W, Tb, V = state[:4]
        assert X.shape == (M, F, T) and W.shape == (F, M, M) and Tb.shape == (M, F, K) and V.shape == (M, K, T)
        assert Tb.min() >= 0.05 and V.max() <= 1.05 + 1e-6
        if dtype == "float32":
            assert all(np.array_equal(a, env.round_to_float32((a,))[0]) for a in state)
        power = np.mean(np.abs(X) ** 2, axis=(0, 2))
        assert F < 3 or power.max() / power.min() > 1e5  # 60 dB over the bins
        if T < M:  # the guarded side: nothing moves, and the ill-posed outputs do not exist
            assert np.array_equal(ref["spatial_ip_W"], W) and np.array_equal(ref["spatial_ip2_W_1"], W)
            assert ref["_cond"].min() > env.THRESHOLD * env.COND_FAR
            assert not any(k.startswith(("spatial_iss", "pb_scale", "normalize_pb")) for k in ref)
        else:
            assert not np.any(ref["spatial_ip_W"] == W) and "pb_scale_%d" % (M - 1) in ref
            # the ISS sweep carried on the filters is oracle_np.iss_update on Y
            R = np.maximum(orc.ilrma_variance(Tb, V, domain), env.EPS)
            Y = orc.iss_update(orc.separate(X, W), R)
            assert env.entrywise("demix", orc.separate(X, ref["spatial_iss_W"]), Y) < 1e-9
        assert ("half_sums_act" in ref) == (K <= env.NMF_HALF_SUMS_MAX_K)
        for out in env.public(ref):
            env.ilrma_tolerance(out, dtype)  # every output has a kind and a measured d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(env.AUXIVA_GRID))
def test_auxiva_case_meets_its_conditions(case, dtype):
    states, refs = env.auxiva_case(case, dtype)
    M, F, T, seeds = env.AUXIVA_GRID[case]
    assert len(states) == len(refs) == len(seeds)
    assert env.max_cond(refs) <= env.MAX_COND_MEASURED
    for (X, W, r_l, r_g), ref in zip(states, refs):
        assert X.shape == (M, F, T) and r_l.shape == r_g.shape == (M, T)
        if dtype == "float64":  # the weights of the state are the oracle's
            assert np.array_equal(r_l, ref["weights_laplace"]) and np.array_equal(r_g, ref["weights_gauss"])
        for kind in env.KINDS:
            if T < M:
                assert np.array_equal(ref["spatial_ip_W_" + kind], W) and "spatial_iss_W_" + kind not in ref
            else:
                Y = orc.iss_update(orc.separate(X, W), np.maximum(r_l if kind == "laplace" else r_g, env.EPS))
                assert env.entrywise("demix", orc.separate(X, ref["spatial_iss_W_" + kind]), Y) < 1e-9
        for out in env.public(ref):
            env.auxiva_tolerance(out, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PROBED + PROBED_AUXIVA)
def test_tables_bound_the_probe(case, dtype):
    u = env.U64 if dtype == "float64" else env.U32
    if case in env.ILRMA_GRID:
        states, _ = env.ilrma_case(case, dtype)
        ds = [env.ilrma_sensitivity(s, env.ILRMA_GRID[case][2], u, seed=i) for i, s in enumerate(states)]
        table, kind_of, tol = env.D_ILRMA[dtype], env.ilrma_kind, env.ilrma_tolerance
    else:
        states, _ = env.auxiva_case(case, dtype)
        ds = [env.auxiva_sensitivity(s, u, seed=i) for i, s in enumerate(states)]
        table, kind_of, tol = env.D_AUXIVA[dtype], env.auxiva_kind, env.auxiva_tolerance
    for d in ds:
        for out, v in d.items():
            assert v <= table[kind_of(out)], (out, v)
            assert v < tol(out, dtype)


def test_tolerances_follow_from_the_tables():
    assert env.ilrma_tolerance("source_Tb") == 256 * env.D_ILRMA["float64"]["Tb"] < 1e-12
    assert env.auxiva_tolerance("loss_gauss", "float32") == env.FLOOR32  # 256 x 4.7e-8 is below the floor
    assert env.ilrma_tolerance("cov_nft", "float32") == 256 * 3.6e-7 < 1e-4
    assert env.ilrma_tolerance("spatial_ip_W", "float32") == 256 * 3.3e-7
    assert env.auxiva_tolerance("spatial_ip2_W_1_gauss") == 256 * env.D_AUXIVA["float64"]["ip2_W"]
    assert set(env.D_ILRMA["float64"]) == set(env.D_ILRMA["float32"]) <= set(env.ILRMA_METRIC)
    with pytest.raises(AssertionError):
        env.entrywise("Tb", np.array([np.inf]), np.array([1.0]))


def test_entrywise_metrics_catch_what_the_frobenius_ratio_lets_through():
    """Five faults planted into reference outputs at (M 4, F 33, T 257), K = 4, the third shape of the stage tests:
    each fails the entry-wise metric at the envelope tolerance of its dtype and passes `rel_err` at the tolerance of the
    stage test of that output in tests/test_gpu_ops.py (W after IP 2e-3, U 2e-5, V 5e-5 in float32; Tb 1e-11 in
    float64)."""
    state = env.ilrma_state(4, 4, 33, 257, 4033257)
    ref64 = env.ilrma_reference(state, 2)
    ref32 = env.ilrma_reference(env.round_to_float32(state), 2)
    level = np.argsort(np.mean(np.abs(state[0]) ** 2, axis=(0, 2)))
    quiet, median = int(level[0]), int(level[16])
    assert quiet != 32

    def plant(ref, out, index, factor):
        got = np.array(ref[out])
        got[index] *= factor
        return got, ref[out]

    faults = [  # output, where, factor, dtype, entry-wise size, the stage test's tolerance
        ("spatial_ip_W", (32, 3), 1.01, "float32", 1e-2, 2e-3),                  # last bin, last source
        ("cov_nft", (1, median), 1 + 1e-4, "float32", 1e-4, 2e-5),               # one (n, f) matrix, median level
        ("source_V", (slice(None), slice(None), 256), 1 + 4e-4, "float32", 4e-4, 5e-5),   # the last frame
        ("source_Tb", (2, 32), 1 + 1e-10, "float64", 1e-10, 1e-11),              # the last bin's row
        ("spatial_ip_U", (slice(None), quiet), 1.5, "float32", 0.5, 2e-5),       # the quietest of bins spanning 60 dB
    ]
    for out, index, factor, dtype, size, old_tol in faults:
        got, want = plant(ref64 if dtype == "float64" else ref32, out, index, factor)
        e, g = env.entrywise(env.ilrma_kind(out), got, want), rel_err(got, want)
        print("%-14s %s: rel_err %.1e (< %.0e passes)  entry-wise %.1e (> %.1e fails)"
              % (out, dtype, g, old_tol, e, env.ilrma_tolerance(out, dtype)))
        assert abs(e - size) < 1e-3 * size, (out, e)
        assert e > env.ilrma_tolerance(out, dtype), (out, e)
        assert g < old_tol, (out, g)
        assert env.entrywise(env.ilrma_kind(out), want, want) == 0
