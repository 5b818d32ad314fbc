"""Every (f15) entry point against the NumPy restatement over the size envelope (tests/beamform_envelope_np.py): every M in
2..8, N in {1, M - 1, M, 8}, F in {1, 3, 17}, and nine frame counts around the wave (63, 64, 65), the workgroup (255, 256,
257) and the MDP pass's frame-chunk seam (chunk - 1, chunk, chunk + 1); T = 1 on invariants only.  Entry-wise metrics,
tolerance 256 x the restatement's one-rounding sensitivity d (floor 1e-13)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import beamform_envelope_np as benv  # noqa: E402
from test_beamform_cpu import pca_invariants  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


def dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=eng.dev)


def host(t):
    return t.cpu().numpy()


def run(eng, st, degenerate=False):
    """Every entry point on one state, keyed like beamform_envelope_np.reference."""
    X, A, R, Ys, ref, eps = st
    M, F, T = X.shape
    Xd, Ad, Yd, status = dev(eng, X), dev(eng, A), dev(eng, Ys), eng.new_status(1)
    got = {}
    Wf, s = eng.bf_ds_weights(Ad, ref)
    got["ds_W"], got["ds_s"], got["ds"] = host(Wf), host(s), host(eng.bf_apply(Xd, Wf, s))
    Wf, s = eng.bf_ml_weights(Ad, dev(eng, R), ref, eps, status)
    got["ml_W"], got["ml"] = host(Wf), host(eng.bf_apply(Xd, Wf, s))
    got["mdp"] = host(eng.mdp_scale(Yd, Xd))
    got["mdp1"] = host(eng.mdp_scale(Yd, Xd[ref:ref + 1].contiguous()))
    C = eng.cov_accumulate(Xd.unsqueeze(0)).reshape(F, M, M)
    V, w, Wp = eng.pca_basis(C, status)
    got["pca_V"], got["pca_w"], got["pca"] = host(V), host(w), host(eng.bf_apply(Xd, Wp))
    if not degenerate:
        Wf, s = eng.bf_ml_weights(Ad, C, ref, eps, status)
        got["mvdr"] = host(eng.bf_apply(Xd, Wf, s))
    assert int(status.item()) == 0
    return got


def test_grid_follows_the_library_constant():
    from audio_source_separation_amd import _lib
    assert benv.FRAME_CHUNK == _lib.BF_FRAME_CHUNK
    assert {_lib.BF_FRAME_CHUNK + k for k in (-1, 0, 1)} <= set(benv.FRAMES)
    assert {63, 64, 65, 255, 256, 257} <= set(benv.FRAMES)
    assert len(benv.GRID) == sum(len(benv.sources(M)) for M in benv.CHANNELS) * 3 * 9


@pytest.mark.parametrize("case", list(benv.GRID))
def test_entry_points(eng, case):
    st, ref = benv.grid_case(case)
    got = run(eng, st)
    worst = {k: benv.distance(k, got[k], ref[k]) for k in ref}
    print(case, {k: "%.1e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= benv.tolerance(k), (k, v, benv.tolerance(k))


@pytest.mark.parametrize("case", list(benv.TINY))
def test_one_frame(eng, case):
    """T = 1: the filters and the scale are still functions of the input and are compared; the covariance has rank one, so
    PCA is held to its invariants and MVDR is left out."""
    st, ref = benv.tiny_case(case)
    got = run(eng, st, degenerate=True)
    for k in ref:
        d = benv.distance(k, got[k], ref[k])
        assert d <= benv.tolerance(k), (k, d)
    pca_invariants(st[0], got["pca_V"], got["pca_w"], got["pca"], benv.tolerance("pca_V"))
