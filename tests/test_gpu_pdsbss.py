"""ProxLaplaceIVA (bss/iva.py on bss/prox.py) on the GPU: every entry point and the class against the reference's recorded
runs (tests/golden/pdsbss), the loop as one library call against the stepwise loop bit for bit, the composed Python loop,
determinism, and the reference's semantics.

Tolerances: one stage, update or loss from a recorded state is held to pdsbss_envelope_np.tolerance (256 x the one-rounding
sensitivity of the restatement over the envelope grid); a whole 10-iteration run to trajectory_tolerance (256 x the
restatement's own sensitivity to one rounding of X, W0 and the norm over these cases), floor 1e-13 in both.  The loss is
never asserted to fall: primal-dual splitting is no descent method on it.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pdsbss_np as pd  # noqa: E402
import pdsbss_envelope_np as penv  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "pdsbss")
NAMES = pd.cases(GOLDEN)
SMALL = "proxlaplaceiva_m3_f4_t70"
OVER = "proxlaplaceiva_m3_f6_t50_over"  # every parameter off its default, a relaxation step above 1, both branches


def load(name):
    return pd.load_case(GOLDEN, name)


def new(g, **kw):
    from audio_source_separation_amd import bss
    args = dict(regularizer=float(g["C"]), step_prox_logdet=float(g["mu1"]), step_prox_penalty=float(g["mu2"]),
                step=float(g["alpha"]), reference_id=int(g["reference_id"]),
                apply_projection_back=bool(g["projection_back"]))
    args.update(kw)
    return bss.ProxLaplaceIVA(**args)


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


def dev(eng, a):
    import torch
    return torch.as_tensor(np.array(a), device=eng.dev)  # a copy: the recorded arrays are read-only


def state(g, it):
    """(W, y) as recorded after iteration `it` (y is zero before the first)."""
    return g["W_%d" % it], (g["y_%d" % it] if it else np.zeros_like(g["z_1"]))


def held(worst, what):
    print(what, {k: "%.1e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= penv.tolerance(k), (what, k, v, penv.tolerance(k))


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_from_recorded_states(eng, name):
    """The norm, the four stages, one update and the loss, one call from each recorded state, against the fixture."""
    import torch
    g = load(name)
    par = pd.params(g)
    M, F, T = g["X"].shape
    X, ws, status = dev(eng, g["X"]), eng.pdsbss_workspace(M, F, T), eng.new_status(1)
    worst = {"norm": penv.entrywise("norm", float(eng.pdsbss_operator_norm(X, ws, status=status).item()), g["norm"])}
    norm = torch.tensor([float(g["norm"])], dtype=torch.float64, device=eng.dev)
    for k in ("adjoint", "prox_logdet", "forward", "prox_group", "update_W", "update_y", "loss"):
        worst[k] = 0.0
    for it in pd.STAGE_ITERS:
        W0, y0 = state(g, it - 1)
        G = eng.pdsbss_adjoint(X, norm, dev(eng, y0), ws).cpu().numpy()
        worst["adjoint"] = max(worst["adjoint"], penv.entrywise("G", G, g["G_%d" % it]))
        Wt = eng.pdsbss_prox_logdet(dev(eng, W0 - par["mu1"] * par["mu2"] * g["G_%d" % it]), par["mu1"], status=status)
        worst["prox_logdet"] = max(worst["prox_logdet"], penv.entrywise("W", Wt.cpu().numpy(), g["Wt_%d" % it]))
        z = eng.pdsbss_forward(X, norm, dev(eng, y0), dev(eng, 2 * g["Wt_%d" % it] - W0))
        worst["forward"] = max(worst["forward"], penv.entrywise("y", z.cpu().numpy(), g["z_%d" % it]))
        p = eng.pdsbss_prox_group(dev(eng, g["z_%d" % it]), ws, C=par["C"], mu=1 / par["mu2"])
        worst["prox_group"] = max(worst["prox_group"],
                                  penv.entrywise("y", (dev(eng, g["z_%d" % it]) - p).cpu().numpy(), g["yt_%d" % it]))
    for a, b in ((0, 1), (1, 2)):
        W, y = (dev(eng, v) for v in state(g, a))
        eng.pdsbss_update(X, norm, W, y, ws, status=status, **par)
        worst["update_W"] = max(worst["update_W"], penv.entrywise("W", W.cpu().numpy(), g["W_%d" % b]))
        worst["update_y"] = max(worst["update_y"], penv.entrywise("y", y.cpu().numpy(), g["y_%d" % b]))
    for it in (0,) + pd.SNAP_ITERS:
        terms = torch.empty(2, dtype=torch.float64, device=eng.dev)
        loss = eng.pdsbss_loss(X, dev(eng, g["W_%d" % it]), ws, C=par["C"], terms=terms)
        worst["loss"] = max(worst["loss"], penv.entrywise("loss", float(loss.item()), g["loss"][it]))
        assert abs(float(terms.sum().item()) - float(loss.item())) <= 1e-13 * abs(float(loss.item()))
    assert int(status.item()) == 0
    held(worst, name)


@pytest.mark.parametrize("name", NAMES)
def test_stepwise_and_one_call_loops(eng, name):
    """update + loss stepwise against the 10 recorded iterations, and assx_pdsbss_iterate against the stepwise run bit for
    bit: W, y and every loss."""
    import torch
    g = load(name)
    par = pd.params(g)
    M, F, T = g["X"].shape
    X, ws, status = dev(eng, g["X"]), eng.pdsbss_workspace(M, F, T), eng.new_status(1)
    norm = torch.tensor([float(g["norm"])], dtype=torch.float64, device=eng.dev)
    W, y = (dev(eng, v) for v in state(g, 0))
    losses, d = [eng.pdsbss_loss(X, W, ws, C=par["C"])], {"W": 0.0, "y": 0.0}
    for it in range(1, pd.N_ITER + 1):
        eng.pdsbss_update(X, norm, W, y, ws, status=status, **par)
        losses.append(eng.pdsbss_loss(X, W, ws, C=par["C"]))
        if it in pd.SNAP_ITERS:
            d["W"] = max(d["W"], penv.entrywise("W", W.cpu().numpy(), g["W_%d" % it]))
            d["y"] = max(d["y"], penv.entrywise("y", y.cpu().numpy(), g["y_%d" % it]))
    losses = torch.cat(losses).cpu().numpy()
    d["loss"] = penv.entrywise("loss", losses, g["loss"])
    print(name, {k: "%.1e" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= penv.trajectory_tolerance(k), (k, v)

    W2, y2 = (dev(eng, v) for v in state(g, 0))
    block = torch.empty(pd.N_ITER + 1, dtype=torch.float64, device=eng.dev)
    eng.pdsbss_iterate(pd.N_ITER, X, norm, W2, y2, ws, loss=block, status=status, **par)
    assert torch.equal(W2, W) and torch.equal(y2, y) and np.array_equal(block.cpu().numpy(), losses)
    W3, y3 = (dev(eng, v) for v in state(g, 0))
    eng.pdsbss_iterate(pd.N_ITER, X, norm, W3, y3, ws, loss=None, status=status, **par)  # without the loss: the same bits
    assert torch.equal(W3, W) and torch.equal(y3, y)
    assert int(status.item()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_class_matches_reference(name):
    """The front door (one assx_pdsbss_iterate call) against the recorded run: W, y, the losses, the output, the norm."""
    g = load(name)
    model = new(g)
    out = model(g["X"], pd.N_ITER, demix_filter=g["W_0"].copy())
    assert model._fast_loop_ok() and len(model.loss) == pd.N_ITER + 1 and isinstance(model.loss, list)
    assert isinstance(out, np.ndarray) and np.array_equal(model.estimation, out)
    assert model.y.shape == (g["X"].shape[1], g["X"].shape[0], g["X"].shape[2])
    d = {"W": penv.entrywise("W", model.demix_filter, g["W_%d" % pd.N_ITER]),
         "y": penv.entrywise("y", model.y, g["y_%d" % pd.N_ITER]),
         "loss": penv.entrywise("loss", model.loss, g["loss"]), "output": penv.entrywise("output", out, g["output"])}
    print(name, {k: "%.1e" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= penv.trajectory_tolerance(k), (k, v)
    assert penv.entrywise("norm", model.norm, g["norm"]) <= penv.tolerance("norm")


def test_composed_python_loop_against_the_fused_one():
    """A no-op callback forces the Python loop, whose update is composed of the four stage entry points: callbacks run
    after each iteration and not before the loop, and the run agrees with the one-call loop within tolerance."""
    g = load(OVER)
    calls = []
    front, step = new(g), new(g, callbacks=lambda m: calls.append(len(m.loss)))
    outs = [m(g["X"], pd.N_ITER) for m in (front, step)]
    assert front._fast_loop_ok() and not step._fast_loop_ok()
    assert calls == list(range(2, pd.N_ITER + 2))
    d = {"W": penv.entrywise("W", step.demix_filter, front.demix_filter), "y": penv.entrywise("y", step.y, front.y),
         "loss": penv.entrywise("loss", step.loss, front.loss), "output": penv.entrywise("output", outs[1], outs[0])}
    print(OVER, {k: "%.1e" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= penv.trajectory_tolerance(k), (k, v)
    assert penv.entrywise("W", step.demix_filter, g["W_%d" % pd.N_ITER]) <= penv.trajectory_tolerance("W")


def test_tensor_in_tensor_out_and_the_prox_methods():
    import torch
    g = load(SMALL)
    a, b = new(g), new(g)
    ya = a(g["X"], pd.N_ITER)
    yb = b(torch.as_tensor(np.array(g["X"]), device="cuda:0"), pd.N_ITER)
    assert isinstance(yb, torch.Tensor) and yb.is_cuda and np.array_equal(yb.cpu().numpy(), ya)
    par = pd.params(g)
    for it in pd.STAGE_ITERS:
        arg = g["W_%d" % (it - 1)] - par["mu1"] * par["mu2"] * g["G_%d" % it]
        Wt = a.prox_logdet(arg, par["mu1"])
        assert isinstance(Wt, np.ndarray) and penv.entrywise("W", Wt, g["Wt_%d" % it]) <= penv.tolerance("prox_logdet")
        Wt_d = a.prox_logdet(torch.as_tensor(np.array(arg), device="cuda:0"), par["mu1"])
        assert isinstance(Wt_d, torch.Tensor) and np.array_equal(Wt_d.cpu().numpy(), Wt)
        p = a.prox_penalty(g["z_%d" % it], 1 / par["mu2"])
        assert isinstance(p, np.ndarray)
        assert penv.entrywise("y", g["z_%d" % it] - p, g["yt_%d" % it]) <= penv.tolerance("prox_group")
        p_d = a.prox_penalty(torch.as_tensor(np.array(g["z_%d" % it]), device="cuda:0"), 1 / par["mu2"])
        assert isinstance(p_d, torch.Tensor) and np.array_equal(p_d.cpu().numpy(), p)
    y = a.separate(g["X"], g["W_2"])
    assert penv.entrywise("output", y, pd.separate(g["X"], g["W_2"], 0, False)) <= penv.tolerance("forward")
    W = g["W_%d" % pd.N_ITER]
    assert abs(a.compute_penalty() - pd.penalty(g["X"], a.demix_filter, par["C"])) <= 1e-12 * abs(pd.penalty(g["X"], W))
    assert abs(a.compute_negative_logdet() - pd.negative_logdet(np.asarray(a.demix_filter))) <= 1e-12
    assert a.compute_negative_loglikelihood() == a.loss[-1]


def test_second_call_warm_starts_w_and_restarts_y():
    g = load(SMALL)
    a = new(g)
    a(g["X"], 4)
    W4, l4 = np.array(a.demix_filter), list(a.loss)
    a(g["X"], 3)
    b = new(g)
    b(g["X"], 3, demix_filter=W4.copy())   # the same filters, y = 0: the second call's run
    assert len(a.loss) == 4 + 1 + 3 + 1 and a.loss[:5] == l4
    assert a.loss[5] == a.loss[4] == b.loss[0]   # one more initial loss, that of the filters the first call left
    assert np.array_equal(a.demix_filter, b.demix_filter) and np.array_equal(a.y, b.y) and a.loss[5:] == list(b.loss)
    c = new(g)
    c(g["X"], 7)
    assert not np.array_equal(c.demix_filter, a.demix_filter)   # y was zero again: not a continuation


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("_warm")])
def test_warm_start_is_kept_and_not_modified(name):
    g = load(name)
    W0 = g["W_0"].copy()
    model = new(g)
    model.demix_filter = W0
    model(g["X"], 1)
    assert np.array_equal(W0, g["W_0"])
    assert penv.entrywise("W", model.demix_filter, g["W_1"]) <= penv.tolerance("update_W")
    assert penv.entrywise("loss", model.loss, g["loss"][:2]) <= penv.tolerance("loss")


def test_projection_back_both_ways_and_no_loss():
    g = load("proxlaplaceiva_m3_f5_t45_nopb")
    plain, scaled, silent = new(g), new(g, apply_projection_back=True), new(g, recordable_loss=False)
    yp, ys, yq = (m(g["X"], pd.N_ITER) for m in (plain, scaled, silent))
    assert np.array_equal(plain.demix_filter, scaled.demix_filter)
    assert penv.entrywise("output", yp, g["output"]) <= penv.trajectory_tolerance("output")
    ref = pd.separate(g["X"], g["W_%d" % pd.N_ITER], int(g["reference_id"]), True)
    assert penv.entrywise("output", ys, ref) <= penv.trajectory_tolerance("output")
    assert not np.allclose(yp, ys)
    # recordable_loss=False (a crash in the reference): the same run, no loss
    assert silent._fast_loop_ok() and silent.loss is None and np.array_equal(yq, yp)
    assert np.array_equal(silent.demix_filter, plain.demix_filter) and np.array_equal(silent.y, plain.y)


def test_subclass_with_its_own_prox_penalty_takes_the_python_loop():
    """The reference's extension point: the same shrinkage written in torch on a PDSBSSbase subclass, and on a
    ProxLaplaceIVA subclass that counts its updates."""
    import torch
    from audio_source_separation_amd import bss
    g = load(OVER)
    seen = []

    def shrink(self, z, mu=1):
        den = torch.sqrt(torch.sum(torch.abs(z) ** 2, dim=0))
        den = torch.where(den <= 0, torch.full_like(den, mu), den)
        return self.regularizer * torch.clamp(1 - mu / den, min=0) * z

    class Torch(bss.PDSBSSbase):
        prox_penalty = shrink

        def compute_penalty(self):
            Y = torch.as_tensor(self.separate(self.input, self.demix_filter))
            return float(self.regularizer * torch.sqrt(torch.sum(torch.abs(Y) ** 2, dim=1)).sum())

    class Counting(bss.ProxLaplaceIVA):
        def update_once(self):
            seen.append(1)
            super().update_once()

    par = dict(regularizer=float(g["C"]), step_prox_logdet=float(g["mu1"]), step_prox_penalty=float(g["mu2"]),
               step=float(g["alpha"]))
    own, counting, plain = Torch(**par), Counting(**par), new(g, apply_projection_back=False)
    assert not own._fast_loop_ok() and not counting._fast_loop_ok()
    yo, yc, yp = own(g["X"], pd.N_ITER), counting(g["X"], pd.N_ITER), plain(g["X"], pd.N_ITER)
    assert len(seen) == pd.N_ITER and len(own.loss) == len(counting.loss) == pd.N_ITER + 1
    for m in (own, counting):
        assert penv.entrywise("W", m.demix_filter, g["W_%d" % pd.N_ITER]) <= penv.trajectory_tolerance("W")
        assert penv.entrywise("y", m.y, g["y_%d" % pd.N_ITER]) <= penv.trajectory_tolerance("y")
        assert penv.entrywise("loss", m.loss, g["loss"]) <= penv.trajectory_tolerance("loss")
    assert penv.entrywise("output", yo, yp) <= penv.trajectory_tolerance("output")
    with pytest.raises(NotImplementedError, match="prox_penalty"):
        bss.PDSBSSbase(recordable_loss=False)(g["X"], 1)


def test_two_runs_agree_bit_for_bit():
    g = load(OVER)
    a, b = new(g), new(g)
    ya, yb = a(g["X"], pd.N_ITER), b(g["X"], pd.N_ITER)
    assert np.array_equal(ya, yb) and np.array_equal(a.demix_filter, b.demix_filter) and np.array_equal(a.y, b.y)
    assert list(a.loss) == list(b.loss) and a.norm == b.norm


def test_all_zero_frames_stay_finite_and_keep_y_zero():
    """den = 0 on those frames: the shrinkage replaces it by 1 / mu2 and leaves the zero alone."""
    g = load(OVER)
    X = g["X"].copy()
    X[:, :, 7:12] = 0
    X[:, :, -1] = 0
    model = new(g)
    out = model(X, pd.N_ITER)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(model.demix_filter)) and np.all(np.isfinite(model.loss))
    assert np.all(model.y[:, :, 7:12] == 0) and np.all(model.y[:, :, -1] == 0) and np.any(model.y != 0)
    states, losses, _ = pd.run(X, pd.identity(*X.shape[:2]), pd.N_ITER, None, **pd.params(g))
    assert penv.entrywise("W", model.demix_filter, states[pd.N_ITER][0]) <= penv.trajectory_tolerance("W")
    assert np.all(states[pd.N_ITER][1][:, :, 7:12] == 0)


def test_rank_deficient_prox_argument(eng):
    """Two equal rows: any choice of the null-space vectors is a valid prox, so only the singular values are asserted,
    h(sigma) with h(0) = sqrt(mu); W = 0 gives sqrt(mu) times a unitary matrix; W = I gives h(1) I."""
    rng = np.random.default_rng(3)
    status = eng.new_status(1)
    for M in (2, 3, 5, 8):
        W = rng.standard_normal((4, M, M)) + 1j * rng.standard_normal((4, M, M))
        W[:, 1] = W[:, 0]
        W[2] = 0
        W[3] = np.eye(M)
        for mu in (0.4, 1.0):
            V = eng.pdsbss_prox_logdet(dev(eng, W), mu, status=status).cpu().numpy()
            assert np.all(np.isfinite(V))
            want = pd.h(np.linalg.svd(W, compute_uv=False), mu)
            got = np.linalg.svd(V, compute_uv=False)
            assert np.max(np.abs(got - want) / want) <= penv.tolerance("prox_logdet"), (M, mu)
            assert np.abs(got[:2, -1] - np.sqrt(mu)).max() <= penv.tolerance("prox_logdet") and np.allclose(got[2], np.sqrt(mu))
            assert np.abs(V[3] - pd.h(1.0, mu) * np.eye(M)).max() <= penv.tolerance("prox_logdet")
    assert int(status.item()) == 0


def test_a_nan_in_x_raises_and_does_not_hang(eng):
    from audio_source_separation_amd import _lib
    g = load(SMALL)
    X = g["X"].copy()
    X[1, 2, 5] = np.nan
    for kw in ({}, {"callbacks": lambda m: None}):
        with pytest.raises(np.linalg.LinAlgError, match="SVD did not converge"):
            new(g, **kw)(X, 3)
    status = eng.new_status(1)
    W = np.full((2, 3, 3), np.inf, dtype=complex)
    eng.pdsbss_prox_logdet(dev(eng, W), 1.0, status=status)
    assert int(status.item()) == _lib.STATUS_NOT_CONVERGED


def test_c_abi_refusals_outside_the_envelope(eng):
    import ctypes
    import torch
    from audio_source_separation_amd import _lib
    from audio_source_separation_amd._device import ptr
    L, ctx, null = _lib.lib, eng.ctx, ctypes.c_void_p(0)
    E_ARG, E_UNSUPPORTED, E_NULL = -1, -2, -3
    buf = torch.zeros(4096, dtype=torch.complex128, device=eng.dev)
    p = ptr(buf)
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 9, 2, 2, null, null) == E_UNSUPPORTED
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 1, 2, 2, null, null) == E_UNSUPPORTED
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 4, 0, 2, null, null) == E_ARG
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 8, 4096, 8192, null, null) == E_UNSUPPORTED
    assert L.assx_pdsbss_update(ctx, 1, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 2, 2, 2, null, null) == E_ARG     # the penalty
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 0.0, 1.0, 1.0, 2, 2, 2, null, null) == E_ARG     # mu1 > 0
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 1.0, -1.0, 1.0, 2, 2, 2, null, null) == E_ARG    # mu2 > 0
    assert L.assx_pdsbss_update(ctx, 0, p, p, p, p, p, 1.0, 1.0, 1.0, float("nan"), 2, 2, 2, null, null) == E_ARG
    assert L.assx_pdsbss_update(ctx, 0, p, p, null, p, p, 1.0, 1.0, 1.0, 1.0, 2, 2, 2, null, null) == E_NULL
    assert L.assx_pdsbss_iterate(ctx, -1, 0, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, null, 2, 2, 2, null, null) == E_ARG
    assert L.assx_pdsbss_iterate(ctx, 1, 2, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, null, 2, 2, 2, null, null) == E_ARG
    assert L.assx_pdsbss_iterate(ctx, 1, 1, 0, p, p, p, p, p, 1.0, 1.0, 1.0, 1.0, null, 2, 2, 2, null, null) == E_NULL
    assert L.assx_pdsbss_loss(ctx, 3, p, p, p, 1.0, p, null, 2, 2, 2, null) == E_ARG
    assert L.assx_pdsbss_prox_group(ctx, 0, p, p, p, 1.0, 0.0, 2, 2, 2, null) == E_ARG
    assert L.assx_pdsbss_prox_group(ctx, 2, p, p, p, 1.0, 1.0, 2, 2, 2, null) == E_ARG
    assert L.assx_pdsbss_prox_logdet(ctx, p, p, -1.0, 2, 2, null, null) == E_ARG
    assert L.assx_pdsbss_prox_logdet(ctx, p, p, 1.0, 9, 2, null, null) == E_UNSUPPORTED
    assert L.assx_pdsbss_operator_norm(ctx, p, p, null, 2, 2, 2, null, null) == E_NULL
    assert L.assx_pdsbss_adjoint(ctx, p, p, p, p, p, 10, 2, 2, null) == E_UNSUPPORTED
    assert L.assx_pdsbss_forward(ctx, p, p, p, p, p, 2, 2, -1, null) == E_ARG
    # the wrappers refuse arrays that do not fit before anything is launched
    X, ws = dev(eng, load(SMALL)["X"]), eng.pdsbss_workspace(3, 4, 70)
    norm = torch.ones(1, dtype=torch.float64, device=eng.dev)
    with pytest.raises(ValueError, match="demix_filter"):
        eng.pdsbss_update(X, norm, buf[:27].reshape(3, 3, 3), buf[:840].reshape(4, 3, 70), ws)
    with pytest.raises(ValueError, match="workspace"):
        eng.pdsbss_update(X, norm, buf[:36].reshape(4, 3, 3), buf[:840].reshape(4, 3, 70), ws[:64])
    with pytest.raises(ValueError, match="supports"):
        eng.pdsbss_workspace(9, 4, 70)
