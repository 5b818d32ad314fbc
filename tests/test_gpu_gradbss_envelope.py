"""Every (f13) entry point against the NumPy restatement over the size envelope (tests/gradbss_envelope_np.py): every M in
2..8, F in {1, 3, 17}, T in {1, 63, 64, 65, 257, 1000} and the frame-chunk length - 1, + 0, + 1 -- tails, a single-frame
reduction, a chunk seam and the row split at M >= 7.  Entry-wise metrics, tolerance 256 x the restatement's one-rounding
sensitivity d (floor 1e-13).  The solver is compared as exact integers on states that meet the 1e-8 gap condition
(re-seeded where the case's own seed misses it, never skipped)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gradbss_np as gb  # noqa: E402
import gradbss_envelope_np as genv  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


def dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=eng.dev)


def test_grid_follows_the_library_constant():
    from audio_source_separation_amd import _lib
    assert genv.FRAME_CHUNK == _lib.GRADBSS_FRAME_CHUNK
    assert {_lib.GRADBSS_FRAME_CHUNK + k for k in (-1, 0, 1)} <= set(genv.FRAMES)
    assert len(genv.GRID) == 7 * 3 * 9


@pytest.mark.parametrize("case", list(genv.GRID))
def test_updates_and_losses(eng, case):
    from audio_source_separation_amd import _lib
    (X, W), ref = genv.grid_case(case)
    M, F, T = X.shape
    Xd, ws, status = dev(eng, X), eng.gradbss_workspace(M, F, T), eng.new_status(1)
    code = {"iva": _lib.GRADBSS_IVA, "fdica": _lib.GRADBSS_FDICA}
    worst = {}
    for cls, (model, natural) in gb.CLASSES.items():
        Wd = dev(eng, W)
        eng.gradbss_update(code[model], natural, Xd, Wd, ws, status=status)
        worst[cls] = genv.entrywise("W", Wd.cpu().numpy(), ref[cls])
    for model in gb.MODELS:
        loss = eng.gradbss_loss(code[model], Xd, dev(eng, W), ws)
        worst["loss_" + model] = genv.entrywise("loss", float(loss.item()), ref["loss_" + model])
    # one iterate call = one update with the losses before and after it
    import torch
    for cls, (model, natural) in gb.CLASSES.items():
        Wd, block = dev(eng, W), torch.empty(2, dtype=torch.float64, device=eng.dev)
        eng.gradbss_iterate(1, code[model], natural, Xd, Wd, ws, loss=block, status=status)
        worst[cls] = max(worst[cls], genv.entrywise("W", Wd.cpu().numpy(), ref[cls]))
        worst["loss_" + model] = max(worst["loss_" + model],
                                     genv.entrywise("loss", float(block[0].item()), ref["loss_" + model]))
    print(case, {k: "%.1e" % v for k, v in worst.items()})
    assert int(status.item()) == 0
    for k, v in worst.items():
        assert v <= genv.tolerance(k), (k, v, genv.tolerance(k))


@pytest.mark.parametrize("case", list(genv.GRID))
def test_solver(eng, case):
    X, W, Wn, order, perm, seed = genv.solver_case(case)
    M, F, T = X.shape
    Wd = dev(eng, W)
    o, p = eng.fdica_solve_permutation(dev(eng, X), Wd, eng.gradbss_workspace(M, F, T))
    assert np.array_equal(o.cpu().numpy(), order), (seed, o.cpu().numpy(), order)
    assert np.array_equal(p.cpu().numpy(), perm), seed
    assert np.array_equal(Wd.cpu().numpy(), Wn)


def test_more_bins_than_a_grid_dimension_holds(eng):
    """F = 65 600 bins: the moment pass runs a flat grid of F x chunks workgroups, the finalize and the weight pass F in x."""
    from audio_source_separation_amd import _lib
    X, W = genv.state(2, 65600, 2, 4242)
    Xd, ws, status = dev(eng, X), eng.gradbss_workspace(2, 65600, 2), eng.new_status(1)
    for cls, code in (("GradLaplaceIVA", _lib.GRADBSS_IVA), ("NaturalGradLaplaceFDICA", _lib.GRADBSS_FDICA)):
        model, natural = gb.CLASSES[cls]
        Wd = dev(eng, W)
        eng.gradbss_update(code, natural, Xd, Wd, ws, status=status)
        d = genv.entrywise("W", Wd.cpu().numpy(), gb.update(model, natural, X, W))
        assert d <= genv.tolerance(cls), (cls, d)
    assert int(status.item()) == 0
    with pytest.raises(RuntimeError, match="at most 65536 bins"):
        eng.fdica_solve_permutation(Xd, dev(eng, W), ws)


def test_solver_orders_a_nan_bin_last_and_keeps_its_rows(eng):
    """Any input gives a valid order and valid permutations: a bin of NaN has a NaN correlation, is ordered last (by
    index among NaNs), scores NaN for every candidate and keeps the identity -- the host model's rule, exact integers."""
    X, W, _, _, _, _ = genv.solver_case("m3_f17_t65")
    X = X.copy()
    X[:, 5, :] = np.nan
    X[:, 11, :] = np.nan
    Wn, order, perm, _ = gb.solve_permutation(X, W)
    assert list(order[-2:]) == [5, 11] and np.array_equal(perm[5], np.arange(3)) and np.array_equal(perm[11], np.arange(3))
    Wd = dev(eng, W)
    o, p = eng.fdica_solve_permutation(dev(eng, X), Wd, eng.gradbss_workspace(*X.shape))
    o, p = o.cpu().numpy(), p.cpu().numpy()
    assert sorted(o) == list(range(17)) and all(sorted(r) == [0, 1, 2] for r in p)
    assert np.array_equal(o, order) and np.array_equal(p, perm) and np.array_equal(Wd.cpu().numpy(), Wn)
