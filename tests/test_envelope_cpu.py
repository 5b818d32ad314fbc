"""The host side of the envelope sweeps without a GPU (tests/envelope_np.py): the grids cover what their docstrings
claim, the state generators meet their conditions, the entry-wise metrics see one wrong small entry that the global
metric cannot, and the committed d tables are what the probe measures."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import envelope_np as env  # noqa: E402

SMALL_MNMF = ("m2_n1_k1_f3_t1", "m4_n6_k33_f3_t65", "m6_n7_k33_f5_t67", "m8_n3_k17_f3_t577")
SMALL_FAST = ("m2_n1_k1_f3_t1", "m3_n1_k17_f16_t130", "m7_n7_k33_f5_t67", "m8_n6_k1_f3_t63")


def test_mnmf_grid_covers_the_envelope():
    G = list(env.MNMF_GRID.values())
    for M in range(2, 9):
        assert any(c[0] == M and c[1] > 4 for c in G), M
        assert any(c[0] == M and c[1] < M for c in G), M
    assert {1, 8} <= {c[1] for c in G}
    assert {1, 15, 16, 17, 33, 64} <= {c[2] for c in G}
    NK = {c[1] * c[2] for c in G}
    assert {16, 17, 512} <= NK and any(256 < v < 512 for v in NK)
    assert {1, 63, 64, 65, 130, 577, 1000} <= {c[4] for c in G}
    assert {1, 3, 15, 16, 17, 33, 70} <= {c[3] for c in G}
    assert {c[0] for c in G if len(c[5]) == 3} == {5, 7}
    assert (8, 8, 64) in {c[:3] for c in G}
    assert len({s for c in G for s in c[5]}) == sum(len(c[5]) for c in G)  # every state has its own seed
    few = [n for n in env.MNMF_GRID if env.few_frames(n)]
    assert few == sorted(env.D_MNMF_SPATIAL_FEW_FRAMES) and len(few) <= 2
    for M in range(2, 9):
        ids = env.reference_ids(M)
        assert ids[0] == 0 and ids[-1] == M - 1 and (M == 2 or 0 < ids[1] < M - 1)


def test_fastmnmf_grid_covers_the_envelope():
    G = list(env.FASTMNMF_GRID.values())
    assert {c[0] for c in G} == set(range(2, 9))
    assert {1, 6, 7, 8} <= {c[1] for c in G}
    assert {1, 15, 16, 17, 33, 64} <= {c[2] for c in G}
    assert {16, 17, 512} <= {c[1] * c[2] for c in G}
    assert {1, 63, 64, 65, 130, 577, 1000} <= {c[4] for c in G}
    assert {1, 3, 15, 16, 17, 33, 70} <= {c[3] for c in G}
    assert [n for n in env.FASTMNMF_GRID if env.diagonalizer_skips(n)] == ["m2_n1_k1_f3_t1"]


def test_tolerances_follow_from_the_tables():
    assert env.mnmf_tolerance("m8_n8_k64_f20_t130", "basis") == 256 * env.D_MNMF["basis"]
    assert env.mnmf_tolerance("m8_n8_k64_f20_t130", "loss") == 256 * env.D_MNMF["loss"] < 2e-13
    assert env.tolerance(0.0) == env.tolerance(3e-16) == 1e-13  # the floor
    assert env.mnmf_tolerance("m8_n8_k64_f20_t130", "spatial_plain") == 256 * env.D_MNMF["spatial"]
    assert env.mnmf_tolerance("m2_n1_k1_f3_t1", "spatial_normalized") == 256 * 6.9e-8
    assert env.mnmf_tolerance("m2_n1_k1_f3_t1", "separate_1") == 256 * env.D_MNMF["separate"]  # spatial only
    assert env.fastmnmf_tolerance("normalize_Q", "float32") == env.FLOOR32
    assert env.fastmnmf_tolerance("nmf_W", "float32") == 256 * 5.8e-7 < 2e-4
    assert all(256 * d < 2e-4 for d in env.D_FASTMNMF["float32"].values())
    assert all(256 * d < 2e-12 for d in env.D_FASTMNMF["float64"].values())


@pytest.mark.parametrize("case", SMALL_MNMF)
def test_mnmf_state_is_general_and_the_tables_hold(case):
    states, refs = env.mnmf_case(case)  # asserts the denominators and that every output is finite
    X, Tb, V, Z, H = states[0]
    M = X.shape[0]
    assert np.allclose(Z.sum(axis=0), 1) and Z.min() > 0
    assert Tb.min() >= 0.05 and V.max() <= 1.05
    assert np.array_equal(H, H.conj().swapaxes(-1, -2))
    assert np.allclose(np.trace(H, axis1=-2, axis2=-1), 1)
    off = H[..., ~np.eye(M, dtype=bool)]
    assert np.all(off.real != 0) and np.all(off.imag != 0)
    assert np.linalg.eigvalsh(H).min() > 0
    # the restatement against itself on a one-rounding copy of the state stays inside the committed d, so inside
    # the tolerance by a factor of 256
    d = env.mnmf_sensitivity(states[0])
    for out, v in d.items():
        kind = env.mnmf_kind(out)
        if kind == "spatial" and env.few_frames(case):
            assert v <= env.D_MNMF_SPATIAL_FEW_FRAMES[case], (out, v)
        else:
            assert v <= env.D_MNMF[kind], (out, v)
        assert v < env.mnmf_tolerance(case, out)
        assert env.entrywise(kind, refs[0][out], refs[0][out]) == 0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", SMALL_FAST)
def test_fastmnmf_state_is_general_and_the_tables_hold(case, dtype):
    states, refs = env.fastmnmf_case(case, dtype)  # asserts cond(Q), the distance of cond(Q V) from the threshold
    if dtype == "float32":
        assert all(np.array_equal(a, env.round_to_float32((a,))[0]) for a in states[0])
    d = env.fastmnmf_sensitivity(states[0], env.U64 if dtype == "float64" else env.U32)
    for out, v in d.items():
        assert v <= env.D_FASTMNMF[dtype][env.fastmnmf_kind(out)], (out, v)
        assert v < env.fastmnmf_tolerance(out, dtype)
    assert "separate_0" not in refs[0] and "separate_%d" % (states[0][0].shape[0] - 1) in refs[0]


def test_diagonalizer_branch_is_not_decided_by_rounding():
    # T < M: V_m has rank T, the restatement's cond(Q V_m) is far beyond the threshold and Q stays
    (state,), (ref,) = env.fastmnmf_case("m2_n1_k1_f3_t1")
    assert np.array_equal(ref["diagonalizer_Q"], state[4])
    _, conds = env.fastmnmf_conds(*state)
    assert conds.min() > 1e15
    # everywhere else the update happens, far below it
    (state,), (ref,) = env.fastmnmf_case("m8_n6_k1_f3_t63")
    _, conds = env.fastmnmf_conds(*state)
    assert conds.max() < 1e9 and not np.any(ref["diagonalizer_Q"] == state[4])


def _decayed(want, index, blk):
    """`want` with one block scaled by 1e-4 (a component that has decayed, as NMF components do), and a copy of it
    with ONE entry of that block off by 1e-6."""
    want = np.array(want)
    want[blk] *= 1e-4
    got = want.copy()
    got[index] *= 1 + 1e-6
    return got, want


ALL = slice(None)


def test_entrywise_metrics_see_what_the_global_one_cannot():
    # output: (the ONE entry scaled by 1 + 1e-6, the block it lies in: one H_fn, one basis column, one output row, ...)
    picks = {"spatial_normalized": ((2, 3, 1, 4), (2, 3)), "basis": ((3, 20), (ALL, 20)), "activation": ((7, 11), (7,)),
             "latent": ((5, 30), (ALL, 30)), "separate_3": ((4, 1, 50), (4, 1))}
    fast = {"nmf_W": ((2, 3, 9), (2, ALL, 9)), "nmf_H": ((6, 32, 66), (6, 32)), "scm_g": ((1, 4, 6), (1, 4)),
            "diagonalizer_Q": ((2, 5, 1), (2,)), "separate_6": ((3, 2, 40), (3, 2))}
    _, (ref,) = env.mnmf_case("m6_n7_k33_f5_t67")
    _, (fref,) = env.fastmnmf_case("m7_n7_k33_f5_t67")
    todo = [(ref, out, env.mnmf_kind(out), env.mnmf_tolerance("m6_n7_k33_f5_t67", out), p) for out, p in picks.items()]
    todo += [(fref, out, env.fastmnmf_kind(out), env.fastmnmf_tolerance(out), p) for out, p in fast.items()]
    for r, out, kind, tol, (index, blk) in todo:
        # as the restatement gives it: the entry-wise metric fails
        got = np.array(r[out])
        got[index] *= 1 + 1e-6
        assert env.entrywise(kind, got, r[out]) > tol, out
        # where the entry is small, the global metric at 1e-9 passes and the entry-wise one still fails
        got, want = _decayed(r[out], index, blk)
        assert env.rel(got, want) < env.REL_TOL, out
        assert env.entrywise(kind, got, want) > tol, out
    # the loss is a scalar: relative
    assert env.entrywise("loss", np.float64(1 + 1e-12), np.float64(1)) > env.mnmf_tolerance("m6_n7_k33_f5_t67", "loss")
    # a non-finite output fails every metric
    with pytest.raises(AssertionError):
        env.entrywise("basis", np.array([np.nan]), np.array([1.0]))
