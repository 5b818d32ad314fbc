"""GradLaplaceIVA, NaturalGradLaplaceIVA (bss/iva.py), GradLaplaceFDICA, NaturalGradLaplaceFDICA (bss/fdica.py) on the GPU:
every entry point and the classes against the reference's recorded runs (tests/golden/gradbss), the loop as one library
call against the stepwise loop bit for bit, determinism, and the reference's semantics.

Tolerances: one update or loss from a recorded state is held to gradbss_envelope_np.tolerance (256 x the one-rounding
sensitivity of the restatement over the envelope grid); a whole 10-iteration run to trajectory_tolerance (256 x the
restatement's own sensitivity to one rounding of X and W0 over these fixtures), floor 1e-13 in both.  The solver is
compared as exact integers and exact row copies.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gradbss_np as gb  # noqa: E402
import gradbss_envelope_np as genv  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "gradbss")
NAMES = [os.path.basename(f)[:-4] for f in gb.fixtures(GOLDEN)]
FDICA = [n for n in NAMES if "FDICA" in n]
SMALL = [n for n in NAMES if "_m3_f4_t70" in n]  # one fixture per class for the semantic tests


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def klass(name):
    from audio_source_separation_amd import bss
    return getattr(bss, name.split("_")[0])


def codes(name):
    from audio_source_separation_amd import _lib
    model, natural = gb.CLASSES[name.split("_")[0]]
    return (_lib.GRADBSS_IVA if model == "iva" else _lib.GRADBSS_FDICA), natural


def new(g, name, **kw):
    args = dict(lr=float(g["lr"]), reference_id=int(g["reference_id"]), eps=float(g["eps"]))
    if "IVA" in name:
        args["apply_projection_back"] = bool(g["projection_back"])
    args.update(kw)
    return klass(name)(**args)


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


def dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=eng.dev)


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_from_recorded_states(eng, name):
    """assx_gradbss_update and assx_gradbss_loss, one call from each recorded state, against the fixture."""
    g = load(name)
    model, natural = codes(name)
    M, F, T = g["X"].shape
    X, ws, status = dev(eng, g["X"]), eng.gradbss_workspace(M, F, T), eng.new_status(1)
    for a, b in ((0, 1), (1, 2)):
        W = dev(eng, g["W_%d" % a])
        eng.gradbss_update(model, natural, X, W, ws, lr=float(g["lr"]), eps=float(g["eps"]), status=status)
        d = genv.entrywise("W", W.cpu().numpy(), g["W_%d" % b])
        print("%s update %d -> %d: %.1e" % (name, a, b, d))
        assert d <= genv.tolerance("W"), (a, d)
    for it in (0,) + gb.SNAP_ITERS:
        loss = float(eng.gradbss_loss(model, X, dev(eng, g["W_%d" % it]), ws).item())
        d = genv.entrywise("loss", loss, g["loss"][it])
        print("%s loss %d: %.1e" % (name, it, d))
        assert d <= genv.tolerance("loss_iva"), (it, d)
    assert int(status.item()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_class_matches_reference(name):
    """The front door (one assx_gradbss_iterate call) and the stepwise loop (forced by a no-op callback): both against
    the recorded run, and against each other bit for bit, losses included."""
    g = load(name)
    calls = []
    front, step = new(g, name), new(g, name, callbacks=lambda m: calls.append(len(m.loss)))
    outs = [m(g["X"], iteration=gb.N_ITER, demix_filter=g["W_0"].copy()) for m in (front, step)]
    assert front._fast_loop_ok() and not step._fast_loop_ok()
    assert calls == list(range(1, gb.N_ITER + 2))
    for m in (front, step):
        assert len(m.loss) == gb.N_ITER + 1 and isinstance(m.loss, list)
    assert np.array_equal(front.demix_filter, step.demix_filter)
    assert np.array_equal(np.array(front.loss), np.array(step.loss))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(front.estimation, outs[0])
    W_ref = g["W_post"] if "FDICA" in name else g["W_%d" % gb.N_ITER]
    d = {"W": genv.entrywise("W", front.demix_filter, W_ref), "loss": genv.entrywise("loss", front.loss, g["loss"]),
         "output": genv.entrywise("output", outs[0], g["output"])}
    print(name, {k: "%.1e" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= genv.trajectory_tolerance(k), (k, v)
    if "FDICA" in name:
        assert np.array_equal(front.permutation_order.cpu().numpy(), g["order"])
        assert np.array_equal(front.permutation.cpu().numpy(), g["perm"])


@pytest.mark.parametrize("name", SMALL)
def test_two_runs_agree_bit_for_bit_and_a_second_call_continues(name):
    g = load(name)
    a, b = new(g, name), new(g, name)
    ya, yb = a(g["X"], iteration=gb.N_ITER), b(g["X"], iteration=gb.N_ITER)
    assert np.array_equal(ya, yb) and np.array_equal(a.demix_filter, b.demix_filter) and list(a.loss) == list(b.loss)
    if "IVA" in name:  # FDICA's solver permutes rows between the two calls; IVA continues exactly
        c = new(g, name)
        c(g["X"], iteration=4)
        yc = c(g["X"], iteration=gb.N_ITER - 4)
        assert len(c.loss) == gb.N_ITER + 2 and np.array_equal(c.demix_filter, a.demix_filter) and np.array_equal(yc, ya)
        assert c.loss[4] == c.loss[5] == a.loss[4] and c.loss[-1] == a.loss[-1]
    else:
        c = new(g, name)
        c(g["X"], iteration=4)
        W4 = np.array(c.demix_filter)
        c(g["X"], iteration=1)
        d = new(g, name)
        d(g["X"], iteration=1, demix_filter=W4.copy())
        assert np.array_equal(c.demix_filter, d.demix_filter) and len(c.loss) == 7


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("_warm")])
def test_warm_start_is_kept_and_not_modified(name):
    g = load(name)
    W0 = g["W_0"].copy()
    model = new(g, name)
    model.demix_filter = W0
    model(g["X"], iteration=1)
    assert np.array_equal(W0, g["W_0"])
    W1 = g["W_1"]
    if "FDICA" in name:  # the solver has run on W_1
        W1 = gb.solve_permutation(g["X"], W1)[0]
    assert genv.entrywise("W", model.demix_filter, W1) <= genv.tolerance("W")
    assert genv.entrywise("loss", model.loss, g["loss"][:2]) <= genv.tolerance("loss_iva")


@pytest.mark.parametrize("name", FDICA)
def test_solver_on_the_recorded_filters(eng, name):
    """order and perm as exact integers; the rows of W bit-identical to the permuted rows of the input."""
    g = load(name)
    M, F, T = g["X"].shape
    W = dev(eng, g["W_pre"])
    order, perm = eng.fdica_solve_permutation(dev(eng, g["X"]), W, eng.gradbss_workspace(M, F, T), eps=float(g["eps"]))
    order, perm, W = order.cpu().numpy(), perm.cpu().numpy(), W.cpu().numpy()
    assert order.dtype == np.int32 and perm.dtype == np.int32
    assert np.array_equal(order, g["order"]) and np.array_equal(perm, g["perm"])
    assert np.array_equal(W, g["W_post"])
    assert all(np.array_equal(W[f], g["W_pre"][f][perm[f]]) for f in range(F))


@pytest.mark.parametrize("cls", ("GradLaplaceIVA", "NaturalGradLaplaceIVA"))
def test_projection_back_both_ways(cls):
    g = load(cls + "_m3_f5_t45_nopb")
    plain, scaled = new(g, cls), new(g, cls, apply_projection_back=True)
    yp, ys = plain(g["X"], iteration=gb.N_ITER), scaled(g["X"], iteration=gb.N_ITER)
    assert np.array_equal(plain.demix_filter, scaled.demix_filter)
    assert genv.entrywise("output", yp, g["output"]) <= genv.trajectory_tolerance("output")
    ref = gb.separate(g["X"], g["W_%d" % gb.N_ITER], int(g["reference_id"]), True)
    assert genv.entrywise("output", ys, ref) <= genv.trajectory_tolerance("output")
    assert not np.allclose(yp, ys)


def test_a_zero_row_raises_for_the_inverting_classes_only(eng):
    """W^-1 of a filter with a zero row does not exist: LinAlgError, raised when the status is checked at the end of the
    call.  The natural forms never invert W: their update leaves no flag (the zero row stays zero, so the front door's
    projection back then meets a singular Y Y^H, as the reference's does; IVA without projection back returns)."""
    from audio_source_separation_amd import _lib
    g = load("GradLaplaceIVA_m3_f4_t70")
    X = g["X"]
    M, F, T = X.shape
    W0 = gb.identity(M, F)
    W0[1, 2, :] = 0
    for name in ("GradLaplaceIVA", "GradLaplaceFDICA"):
        with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
            klass(name)()(X, iteration=2, demix_filter=W0.copy())
    out = klass("NaturalGradLaplaceIVA")(apply_projection_back=False)(X, iteration=2, demix_filter=W0.copy())
    assert out.shape == X.shape and np.all(out[2, 1] == 0)
    ws, status = eng.gradbss_workspace(M, F, T), eng.new_status(1)
    for model in (_lib.GRADBSS_IVA, _lib.GRADBSS_FDICA):
        W = dev(eng, W0)
        eng.gradbss_update(model, True, dev(eng, X), W, ws, status=status)
        assert int(status.item()) == 0 and np.all(W.cpu().numpy()[1, 2] == 0)
        eng.gradbss_update(model, False, dev(eng, X), W, ws, status=status)
        assert int(status.item()) == _lib.STATUS_SINGULAR
        status.zero_()


def test_overridden_step_and_not_holonomic_keep_the_python_loop():
    g = load("NaturalGradLaplaceFDICA_m3_f4_t70")
    base = klass("NaturalGradLaplaceFDICA")
    seen = []

    class Counting(base):
        def update_once(self):
            seen.append(1)
            super().update_once()

    model, plain = Counting(), base()
    y = model(g["X"], iteration=3)
    assert len(seen) == 3 and np.array_equal(y, plain(g["X"], iteration=3)) and list(model.loss) == list(plain.loss)
    with pytest.raises(NotImplementedError, match="is_holonomic"):
        base(is_holonomic=False)(g["X"], iteration=1)
    with pytest.raises(NotImplementedError):
        klass("GradFDICAbase")()(g["X"], iteration=1)
    with pytest.raises(NotImplementedError):
        klass("GradIVAbase")(recordable_loss=False)(g["X"], iteration=1)
