"""ComplexEUCNMF on the GPU: every entry point against the reference's recorded states (tests/golden/cnmf) and the
NumPy restatement (tests/cnmf_np.py), the class against the reference, and the determinism of the HIP path.

Whole runs are not comparable entry by entry (a one-ulp change grows by about x50 per iteration), so models are
compared one update at a time; tolerances come from tests/golden/cnmf/tolerances.json (tools/cnmf_tolerance_probe.py).
Every figure is printed before it is asserted (pytest -s shows them)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnmf_np as cn  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [os.path.basename(f)[:-4] for f in cn.fixture_files()]
TOL = cn.tolerances()
E_ARG, E_UNSUPPORTED = -1, -2


def load(name):
    return np.load(os.path.join(cn.GOLDEN, name + ".npz"))


def cls():
    from audio_source_separation_amd.algorithm.nmf import ComplexEUCNMF
    return ComplexEUCNMF


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(dtype="float64")


def up(eng, *arrays):
    """NumPy arrays with their batch axis -> device tensors"""
    from audio_source_separation_amd._device import to_device, torch
    return [to_device(a, torch.complex128 if np.iscomplexobj(a) else torch.float64, eng.dev) for a in arrays]


def down(*tensors):
    from audio_source_separation_amd._device import to_numpy
    return [to_numpy(t) for t in tensors]


def device_updates(eng, X, model, reg, p, eps, n=1, iterate=False, loss=False):
    """n updates of a batch (X (B,F,T) and model arrays with a batch axis); returns the model and the loss block"""
    from audio_source_separation_amd._device import torch
    Xd, Td, Vd, Pd = up(eng, X, *model)
    B, F, K = Td.shape
    ws = eng.cnmf_workspace(B, F, Xd.shape[2], K)
    block = eng.empty((n, B), dtype=torch.float64) if loss else None
    if iterate:
        eng.cnmf_iterate(n, Xd, Td, Vd, Pd, ws, regularizer=reg, p=p, eps=eps, loss=block)
    else:
        for i in range(n):
            eng.cnmf_update(Xd, Td, Vd, Pd, ws, regularizer=reg, p=p, eps=eps)
            if loss:
                eng.cnmf_loss(Xd, Td, Vd, Pd, ws, eps=eps, loss=block[i])
    return down(Td, Vd, Pd), (down(block)[0] if loss else None)


def one_update(eng, X, model, reg, p, eps):
    got, _ = device_updates(eng, X[None], [a[None] for a in model], reg, p, eps)
    return [a[0] for a in got]


def check(got, want, X, tol, what):
    figures = cn.compare(got, want, X)
    print(what, {k: "%.2e (tol %.2e)" % (v, tol[k]) for k, v in figures.items()})
    for metric, err in figures.items():
        assert err <= tol[metric], (what, metric, err, tol[metric])


# ---- entry points against the fixtures -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_update_from_every_recorded_state(eng, name):
    fx = load(name)
    X, (reg, p, eps) = fx["X"], cn.params(fx)
    for it in cn.start_iters(fx):
        got = one_update(eng, X, cn.state(fx, it), reg, p, eps)
        check(got, cn.state(fx, it + 1), X, TOL["one_update"], "%s %d->%d" % (name, it, it + 1))
        assert np.all(np.abs(got[2]) <= np.pi)


@pytest.mark.parametrize("name", NAMES)
def test_loss_beta_reconstruct_against_restatement(eng, name):
    fx = load(name)
    X, eps = fx["X"], float(fx["eps"])
    for it in (0, 20):
        T, V, Phi = cn.state(fx, it)
        Xd, Td, Vd, Pd = up(eng, X[None], T[None], V[None], Phi[None])
        F, K = T.shape
        ws = eng.cnmf_workspace(1, F, X.shape[1], K)
        loss, beta, rec = down(eng.cnmf_loss(Xd, Td, Vd, Pd, ws, eps=eps), eng.cnmf_beta(Td, Vd, eps=eps),
                               eng.cnmf_reconstruct(Td, Vd, Pd))
        e_loss = cn.rel(loss[0], cn.loss(X, T, V, Phi))
        e_rec = cn.rel(rec[0], cn.reconstruct(T, V, Phi))
        e_beta = cn.rel(beta[0], cn.beta(T, V, eps))
        # Beta is a product over a K-term sum: K + 2 roundings of 2^-53 each, whatever the order of the sum
        tol_beta = (K + 2) * 2.0 ** -53
        print(name, it, "loss %.2e reconstruct %.2e beta %.2e (tol %.2e)" % (e_loss, e_rec, e_beta, tol_beta))
        assert e_loss <= TOL["one_update"]["loss"] and e_rec <= TOL["one_update"]["components"]
        assert e_beta <= tol_beta
        if it == 20:
            assert cn.rel(loss[0], fx["loss"][19]) <= TOL["one_update"]["loss"]
        assert all(np.array_equal(a, b[None]) for a, b in zip(down(Td, Vd, Pd), (T, V, Phi)))  # read-only calls


def test_silent_entries_keep_phase_zero(eng):
    fx = load("cnmf_f17_t40_k1_p1_r0p1_silent")
    X, (reg, p, eps) = fx["X"], cn.params(fx)
    quiet = X == 0
    assert quiet.sum() == 40 + 2 * 16
    for it in (0, 1, 19):
        got = one_update(eng, X, cn.state(fx, it), reg, p, eps)
        assert np.all(got[2][:, 0, :][quiet] == 0), it  # Zbar is exactly 0 there; angle(0) = 0


# ---- the class against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_class_matches_reference(name):
    fx = load(name)
    X, (reg, p, eps) = fx["X"], cn.params(fx)
    F, K = fx["T0"].shape
    n_frames = X.shape[1]
    for n_iter in (1, 2):
        np.random.seed(int(fx["seed"]))
        model = cls()(n_basis=K, regularizer=reg, p=p)
        out = model(X, iteration=n_iter)
        assert np.random.rand() == float(fx["rng_next"])  # the three draws of the reference's _reset, nothing else
        assert [a.shape for a in out] == [(F, K), (K, n_frames), (F, K, n_frames)]
        assert all(a.dtype == np.float64 for a in out)
        assert all(np.array_equal(a, b) for a, b in zip(out, (model.basis, model.activation, model.phase)))
        check(out, cn.state(fx, n_iter), X, TOL["whole_run"][str(n_iter)], "%s class, iteration %d" % (name, n_iter))
        assert len(model.loss) == n_iter
    np.random.seed(int(fx["seed"]))
    model = cls()(n_basis=K, regularizer=reg, eps=eps)
    model(X, iteration=20, p=p)  # kwargs are applied by _reset, as in the reference
    loss = np.asarray(model.loss)
    assert loss.shape == (20,)
    tol = {1: TOL["whole_run"]["1"]["loss"], 2: TOL["whole_run"]["2"]["loss"], 5: TOL["whole_run"]["5"]["loss"],
           20: TOL["loss_20"][name]}
    for it, t in tol.items():
        err = abs(loss[it - 1] - fx["loss"][it - 1]) / abs(fx["loss"][it - 1])
        print(name, "loss[%d] %.2e (tol %.2e)" % (it, err, t))
        assert err <= t, (it, err, t)
    assert cn.rel(model.reconstruct(), cn.reconstruct(model.basis, model.activation, model.phase)) \
        <= TOL["one_update"]["components"]
    assert model.Beta.shape == (F, K, n_frames)
    # get followed by set round-trips the angles exactly
    phase = model.phase.copy()
    model.phase = phase
    model._dev("Phi", False)
    model._touch("Phi")
    assert np.array_equal(model.phase, phase)


# ---- bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cnmf_f17_t40_k7_p1_r0p1_silent", "cnmf_f5_t257_k16_p0p7_r0p01"])
def test_one_call_loop_equals_update_once_bit_for_bit(name):
    fx = load(name)
    X, (reg, p, eps) = fx["X"], cn.params(fx)
    K = fx["T0"].shape[1]
    runs = []
    for mode in ("loop", "loop", "steps", "no loss"):
        np.random.seed(int(fx["seed"]))
        model = cls()(n_basis=K, regularizer=reg, p=p, recordable_loss=mode != "no loss")
        if mode == "steps":
            model.target = X
            model._reset()
            for _ in range(20):
                model.update_once()
                model._record_loss()
        else:
            model(X, iteration=20)
        runs.append((model.basis.copy(), model.activation.copy(), model.phase.copy(), list(model.loss)))
    first = runs[0]
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(first[:3], other[:3]))
    assert first[3] == runs[1][3] and len(first[3]) == 20 and runs[3][3] == []
    # include/assx.h: loss[i] of assx_cnmf_iterate equals assx_cnmf_loss bit for bit
    assert first[3] == runs[2][3]


def test_batch_of_two_equals_two_singles_bit_for_bit(eng):
    fx = load("cnmf_f33_t65_k6_p1p2_r0p001")
    X, (reg, p, eps) = fx["X"], cn.params(fx)
    states = [cn.state(fx, 0), cn.state(fx, 5)]
    Xb = np.stack([X, X[::-1].copy()])
    batch, batch_loss = device_updates(eng, Xb, [np.stack(a) for a in zip(*states)], reg, p, eps, n=3, iterate=True,
                                       loss=True)
    for b, st in enumerate(states):
        for iterate in (True, False):
            single, loss = device_updates(eng, Xb[b:b + 1], [a[None] for a in st], reg, p, eps, n=3, iterate=iterate,
                                          loss=True)
            assert all(np.array_equal(x[b], y[0]) for x, y in zip(batch, single)), (b, iterate)
            assert np.array_equal(batch_loss[:, b], loss[:, 0]), (b, iterate)


# ---- tile edges beyond the fixtures ----------------------------------------------------------------------------------
EDGES = [(9, t, 3, 1) for t in (63, 64, 65, 255, 256, 257)] + [(f, 70, 3, 1) for f in (1, 2, 15, 16, 17)] \
    + [(9, 65, k, 1.2) for k in (1, 7, 8, 9, 16, 17, 33, 64)]  # 16 | 17: the kernels take n_basis in chunks of 16


@pytest.mark.parametrize("F,T,K,p", EDGES)
def test_tile_edges_against_restatement(eng, F, T, K, p):
    X, Tb, V, Phi = cn.synthetic(F, T, K, seed=F * 1000 + T * 7 + K)
    want = cn.update(X, Tb, V, Phi, 0.1, p, 1e-12)
    got = one_update(eng, X, (Tb, V, Phi), 0.1, p, 1e-12)
    check(got, want, X, TOL["one_update"], "F=%d T=%d K=%d" % (F, T, K))


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from audio_source_separation_amd import _lib
    from audio_source_separation_amd._device import ptr, torch
    X, Tb, V, Phi = cn.synthetic(5, 12, 64, seed=3)  # arrays large enough for every size named below
    Xd, Td, Vd, Pd = up(eng, X[None], Tb[None], V[None], Phi[None])
    ws = eng.cnmf_workspace(1, 5, 12, 64)
    kept = down(Td, Vd, Pd)

    def raw(K, dtype):
        return eng._L.assx_cnmf_update(eng.ctx, ptr(Xd), ptr(Td), ptr(Vd), ptr(Pd), 0.1, 1.0, 1e-12, ptr(ws), 1, 5, 12, K,
                                       dtype, eng._st())

    assert raw(0, _lib.F64) == E_ARG and raw(65, _lib.F64) == E_ARG
    assert raw(3, _lib.F32) == E_UNSUPPORTED and raw(3, 7) == E_ARG
    assert raw(65, _lib.F64) == E_ARG and b"n_basis" in _lib.lib.assx_last_error(eng.ctx)
    assert eng._L.assx_cnmf_iterate(eng.ctx, -1, ptr(Xd), ptr(Td), ptr(Vd), ptr(Pd), 0.1, 1.0, 1e-12, None, ptr(ws), 1, 5,
                                    12, 3, _lib.F64, eng._st()) == E_ARG
    torch.cuda.synchronize(eng.dev)
    assert all(np.array_equal(a, b) for a, b in zip(kept, down(Td, Vd, Pd)))  # a refused call touches nothing
    X, Tb, V, Phi = cn.synthetic(5, 12, 3, seed=4)
    Xd, Td, Vd, Pd = up(eng, X[None], Tb[None], V[None], Phi[None])
    strided = torch.empty((1, 5, 3, 24), dtype=torch.float64, device=eng.dev)[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        eng.cnmf_update(Xd, Td, Vd, strided, ws)
    with pytest.raises(ValueError, match="workspace"):
        eng.cnmf_update(Xd, Td, Vd, Pd, ws[:eng._L.assx_cnmf_workspace_bytes(1, 5, 12, 3, _lib.F64) - 1])
    with pytest.raises(ValueError, match="n_basis"):
        eng.cnmf_beta(Td[:, :, :0].contiguous(), Vd[:, :0].contiguous())
    with pytest.raises(ValueError, match="shape"):
        eng.cnmf_update(Xd, Td, Vd[:, :2].contiguous(), Pd, ws)
    with pytest.raises(ValueError, match="float64"):
        cls()(dtype="float32")
    with pytest.raises(ValueError, match="n_basis"):
        cls()(n_basis=65)(X, iteration=1)
