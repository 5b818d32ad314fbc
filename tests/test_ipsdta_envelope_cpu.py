"""The host side of the IPSDTA envelope sweeps without a GPU (tests/ipsdta_envelope_np.py): the grid covers what the
docstrings of the GPU files claim, the general states meet their conditions and have teeth, the entry-wise basis metric
sees one wrong entry of a small block that the pooled metric lets through, and the committed d tables are at least what
the probe measures."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ipsdta_envelope_np as ev  # noqa: E402
import ipsdta_np as ip  # noqa: E402

SMALL = ("m5_f5_t1_k1_b1", "m2_f300_t8_k1_b300", "m5_f12_t40_k16_b3")
TEETH = ("m6_f11_t64_k7_b2", "m5_f12_t40_k16_b3")


def test_grid_covers_the_envelope():
    G = ev.GRID
    for name, (M, F, T, K, nblk, seed, nu) in G.items():
        assert name == "m%d_f%d_t%d_k%d_b%d" % (M, F, T, K, nblk)
        assert nu in ev.NUS
    assert 8 <= len(G) <= 12
    assert {c[0] for c in G.values()} == set(range(2, 9))
    for M in (6, 7, 8):
        assert any(G[n][0] == M and max(ev.block_sizes(n)) >= 5 for n in G), M
    assert any(G[n][0] == 8 and ev.block_sizes(n) == [8] and G[n][4] > 1 for n in G)  # M = 8 with more than one block of 8
    assert {nb for n in G for nb in ev.block_sizes(n)} == set(range(1, 9))
    groups = {n: ip.geometry(G[n][1], G[n][4]) for n in G}  # (nn, nlow, n_remains)
    assert any(g[1] and g[2] for g in groups.values()) and any(g[2] == 0 for g in groups.values())
    assert any(g[2] == 1 for g in groups.values())  # a high group of one block
    assert any(c[4] > 256 for c in G.values()) and any(c[1] > 512 for c in G.values())
    assert {1, 7, 8, 9, 16, 17, 64} <= {c[3] for c in G.values()}
    assert {1, 8, 63, 64, 65, 257, 577} <= {c[2] for c in G.values()}
    assert len({c[5] for c in G.values()}) == len(G)  # every state has its own seed
    assert {c[6] for c in G.values()} == set(ev.NUS)
    # the exception: exactly one case, the single frame; it alone has no spatial reference and a basis d of its own
    few = [n for n in G if ev.single_frame(n)]
    assert few == ["m5_f5_t1_k1_b1"]
    assert all(sorted(ev.D_BASIS_SINGLE_FRAME[m]) == few for m in ev.MODELS)
    assert [n for n in G if n not in ev.SPATIAL_CASES] == few


def test_tolerances_follow_from_the_tables():
    assert ev.FACTOR == 256 and ev.FLOOR64 == 1e-13
    assert ev.tolerance(0.0) == ev.tolerance(3e-16) == 1e-13
    for m in ev.MODELS:
        assert sorted(ev.D[m]) == sorted(ev.KINDS)
        for name in ev.GRID:
            for out in ("basis", "activation", "normalize_U", "normalize_H", "spatial_1", "spatial_2", "loss"):
                tol = ev.entry_tolerance(name, m, out)
                if out == "basis" and name == "m5_f5_t1_k1_b1":
                    assert tol == 256 * ev.D_BASIS_SINGLE_FRAME[m][name] < 1e-5
                    assert ev.pooled_tolerance(name, m, out) == tol  # the pooled metric cannot ask for more
                else:
                    assert tol == max(256 * ev.D[m][ev.kind_of(out)], 1e-13)
        assert ev.entry_tolerance("m8_f16_t65_k9_b2", m, "basis") < 2e-11
        assert ev.entry_tolerance("m8_f16_t65_k9_b2", m, "activation") < 1e-12
        assert ev.entry_tolerance("m8_f16_t65_k9_b2", m, "spatial_2") < 3e-9
        assert ev.entry_tolerance("m8_f16_t65_k9_b2", m, "loss") < 3e-13
        assert ev.entry_tolerance("m5_f5_t1_k1_b1", m, "activation") == ev.entry_tolerance("m8_f16_t65_k9_b2", m, "activation")
    assert ev.pooled_tolerance("m8_f16_t65_k9_b2", "gauss", "basis") == ip.tolerances()["one_stage"]["U"]
    assert ev.round_up(1.234e-14) == 1.3e-14 and ev.round_up(1.2e-14) == 1.2e-14 and ev.round_up(0.0) == 0.0


@pytest.mark.parametrize("name", SMALL)
def test_state_is_general_and_the_tables_hold(name):
    M, F, T, K, nblk, seed, nu = ev.GRID[name]
    (X, W, U, H), rawU, rawH, refs = ev.case(name)  # asserts the host conditions
    assert X.shape == (M, F, T) and W.shape == (F, M, M) and H.shape == (M, K, T)
    # W: unitary up to the row scaling, never diagonally dominant in every bin, and the kernels' LU swaps rows
    G = W @ ip.ct(W)
    scale = np.sqrt(np.einsum("fii->fi", G).real)
    assert scale.min() >= 0.5 and scale.max() <= 1.5
    assert np.allclose(G, scale[:, :, None] * np.eye(M) * scale[:, None, :], atol=1e-12)
    off = np.sum(np.abs(W), axis=2) - np.abs(np.einsum("fii->fi", W))
    assert np.any(off > np.abs(np.einsum("fii->fi", W)))
    assert ev.lu_row_swaps(W) >= 1
    # U: Hermitian, positive definite, a real and an imaginary part off the diagonal, no two blocks equal, trace one
    blocks = []
    for p in ip.to_parts(U):
        nb = p.shape[-1]
        assert np.array_equal(p, ip.ct(p)) and np.linalg.eigvalsh(p).min() > 0
        o = p[..., ~np.eye(nb, dtype=bool)]
        assert np.all(o.real != 0) and np.all(o.imag != 0)
        blocks += [b.tobytes() for b in p.reshape(-1, nb, nb)]
    assert len(set(blocks)) == len(blocks)
    tr = sum(np.einsum("nkbii->nk", p).real for p in ip.to_parts(U))
    assert np.allclose(tr, 1.0, rtol=0, atol=1e-13)
    # the state before its normalisation: traces far from one and different per (source, basis)
    tr_raw = sum(np.einsum("nkbii->nk", p).real for p in ip.to_parts(rawU))
    assert tr_raw.min() > 1.5 and len(np.unique(tr_raw)) == tr_raw.size and rawH.min() >= 0.1 and rawH.max() <= 1.1
    for m in ev.MODELS:
        assert ev.entrywise(name, "normalize_U", refs[m]["normalize_U"], U) == 0
        # what the probe measures now stays inside the committed d, so inside the tolerance by a factor of 256
        for out, v in ev.measure(name, m).items():
            kind = ev.kind_of(out)
            d = ev.D_BASIS_SINGLE_FRAME[m][name] if kind == "basis" and ev.single_frame(name) else ev.D[m][kind]
            assert v <= d, (name, m, out, v, d)
            assert v < ev.entry_tolerance(name, m, out)


def test_lu_model_counts_the_bins_that_swap():
    eye = np.eye(3, dtype=np.complex128)
    assert ev.lu_row_swaps(np.stack([eye, 2 * eye])) == 0
    assert ev.lu_row_swaps(np.stack([eye, eye[[1, 0, 2]], eye[[0, 2, 1]]])) == 2
    # |re| + |im|, not the modulus: 0.8 + 0.8i (modulus 1.13, sum 1.6) wins over 1.5 (modulus 1.5, sum 1.5)
    A = np.array([[1.5, 0, 0], [0.8 + 0.8j, 1, 0], [0, 0, 1]], dtype=np.complex128)
    assert ev.lu_row_swaps(A[None]) == 1
    # a tie keeps the row in place
    B = np.array([[1.0, 2.0], [1.0j, 1.0]], dtype=np.complex128)
    assert ev.lu_row_swaps(B[None]) == 0


def test_entrywise_basis_metric_sees_what_the_pooled_one_cannot():
    name = "m6_f11_t64_k7_b2"  # one block of 5 and one of 6
    _, _, _, refs = ev.case(name)
    for m in ev.MODELS:
        tol, ptol = ev.entry_tolerance(name, m, "basis"), ev.pooled_tolerance(name, m, "basis")
        low, high = (np.array(a) for a in refs[m]["basis"])  # (N, n, nb, nb, K): the smallest block is the low one
        # as the restatement gives it: one entry of the small block off by 1e-9, both metrics fail
        bad = low.copy()
        bad[2, 0, 1, 1, 3] *= 1 + 1e-9
        assert ev.block_metric((bad, high), (low, high)) > tol
        # where the small block has decayed next to the large one, the pooled metric passes and the entry-wise one fails
        low = low * 1e-4
        bad = low.copy()
        bad[2, 0, 1, 1, 3] *= 1 + 1e-9
        assert ip.basis_metric((bad, high), (low, high)) < ptol
        assert ev.block_metric((bad, high), (low, high)) > tol
    # W per (bin, row): a row that is small next to the others of its bin
    want = np.array(refs["gauss"]["spatial_1"])
    want[4, 2] *= 1e-6
    bad = want.copy()
    bad[4, 2, 1] *= 1 + 1e-6
    assert ip.w_metric(bad, want) < ev.pooled_tolerance(name, "gauss", "spatial_1")
    assert ev.row_metric(bad, want) > ev.entry_tolerance(name, "gauss", "spatial_1")
    # a non-finite output fails
    with pytest.raises(AssertionError):
        ev.entrywise(name, "activation", np.array([np.nan]), np.array([1.0]))


@pytest.mark.parametrize("name", TEETH)
def test_states_have_teeth(name):
    """A kernel that read U transposed, or W_f transposed, would be seen: the references move by more than 1e3 x their
    tolerances (with identity W and real diagonal bases neither would change anything)."""
    (X, W, U, H), _, _, refs = ev.case(name)
    conj_u = tuple(np.conj(p) for p in U) if isinstance(U, tuple) else np.conj(U)
    w_t = np.ascontiguousarray(np.swapaxes(W, 1, 2))
    for m in ev.MODELS:
        for what, st, outs in (("conj(U)", (X, W, conj_u, H), ("basis", "activation", "loss")),
                               ("W^T", (X, w_t, U, H), ("basis", "activation", "loss", "spatial_1", "spatial_2"))):
            other = ev.references(name, m, st)
            for out in outs:
                moved, tol = ev.entrywise(name, out, other[out], refs[m][out]), ev.entry_tolerance(name, m, out)
                assert moved > 1e3 * tol, (name, m, what, out, moved, tol)
