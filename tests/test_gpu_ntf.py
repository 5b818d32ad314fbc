"""EUCNTF on the GPU: every entry point against the reference's recorded states (tests/golden/ntf) and the NumPy
restatement (tests/ntf_np.py), the class against the reference, and the determinism of the HIP path.

Every sum of the model is a sum of non-negative terms, so models are compared entry by entry (|a - b| / |b|), single
updates and whole 20-iteration runs alike; tolerances come from tests/golden/ntf/tolerances.json
(tools/ntf_tolerance_probe.py).  Every figure is printed before it is asserted (pytest -s shows them)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ntf_np as nt  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [os.path.basename(f)[:-4] for f in nt.fixture_files()]
CLASS_NAMES = ["ntf_n2_i17_j40_k3", "ntf_n3_i33_j65_k6_silent", "ntf_n4_i5_j257_k16", "ntf_n8_i8_j64_k64",
               "ntf_n6_i7_j9_k3_floor"]
TOL = nt.tolerances()
E_ARG, E_UNSUPPORTED = -1, -2


def load(name):
    return np.load(os.path.join(nt.GOLDEN, name + ".npz"))


def cls():
    from audio_source_separation_amd.algorithm.ntf import EUCNTF
    return EUCNTF


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(dtype="float64")


def up(eng, *arrays):
    """NumPy arrays with their batch axis -> device tensors"""
    from audio_source_separation_amd._device import to_device, torch
    return [to_device(np.ascontiguousarray(a), torch.float64, eng.dev) for a in arrays]


def down(*tensors):
    from audio_source_separation_amd._device import to_numpy
    return [to_numpy(t) for t in tensors]


def device_updates(eng, X, model, eps, n=1, iterate=False, loss=False):
    """n updates of a batch (X (B,N,I,J) and model arrays with a batch axis); returns the model and the loss block"""
    from audio_source_separation_amd._device import torch
    Xd, Zd, Td, Vd = up(eng, X, *model)
    B, N, K = Zd.shape
    ws = eng.ntf_workspace(B, N, Td.shape[1], Vd.shape[2], K)
    block = eng.empty((n, B), dtype=torch.float64) if loss else None
    if iterate:
        eng.ntf_iterate(n, Xd, Zd, Td, Vd, ws, eps=eps, loss=block)
    else:
        for i in range(n):
            eng.ntf_update(Xd, Zd, Td, Vd, ws, eps=eps)
            if loss:
                eng.ntf_loss(Xd, Zd, Td, Vd, ws, loss=block[i])
    return down(Zd, Td, Vd), (down(block)[0] if loss else None)


def one_update(eng, X, model, eps):
    got, _ = device_updates(eng, X[None], [a[None] for a in model], eps)
    return [a[0] for a in got]


def check(got, want, X, tol, what):
    figures = nt.compare(got, want, X)
    print(what, {k: "%.2e (tol %.2e)" % (v, tol[k]) for k, v in figures.items()})
    for metric, err in figures.items():
        assert err <= tol[metric], (what, metric, err, tol[metric])


# ---- entry points against the fixtures -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_update_from_every_recorded_state(eng, name):
    fx = load(name)
    X, eps = fx["X"], float(fx["eps"])
    for it in nt.START_ITERS:
        got = one_update(eng, X, nt.state(fx, it), eps)
        check(got, nt.state(fx, it + 1), X, TOL["one_update"], "%s %d->%d" % (name, it, it + 1))


@pytest.mark.parametrize("name", NAMES)
def test_loss_and_reconstruct_against_restatement(eng, name):
    fx = load(name)
    X = fx["X"]
    N, I, J = X.shape
    # X_hat is a sum of K positive products of three factors: K + 2 roundings of 2^-53 each, whatever the order
    tol_rec = (fx["Z0"].shape[1] + 2) * 2.0 ** -53
    for it in (0, 20):
        model = nt.state(fx, it)
        Xd, Zd, Td, Vd = up(eng, X[None], *[a[None] for a in model])
        ws = eng.ntf_workspace(1, N, I, J, model[0].shape[1])
        loss, rec = down(eng.ntf_loss(Xd, Zd, Td, Vd, ws), eng.ntf_reconstruct(Zd, Td, Vd))
        e_loss = nt.rel_entry(loss[0], nt.loss(X, *model))
        e_rec = nt.rel_entry(rec[0], nt.reconstruct(*model))
        print(name, it, "loss %.2e (tol %.2e) reconstruct %.2e (tol %.2e)" % (e_loss, TOL["one_update"]["loss"], e_rec,
                                                                            tol_rec))
        assert loss.shape == (1,) and rec.shape == (1, N, I, J)
        assert e_loss <= TOL["one_update"]["loss"] and e_rec <= tol_rec
        if it == 20:
            e_fx = nt.rel_entry(loss[0], fx["loss"][19])
            print(name, "loss at 20 against the recorded list %.2e" % e_fx)
            assert e_fx <= TOL["one_update"]["loss"]
        assert all(np.array_equal(a, b[None]) for a, b in zip(down(Zd, Td, Vd), model))  # read-only calls


@pytest.mark.parametrize("name", NAMES)
def test_iterate_20_against_the_recorded_run(eng, name):
    fx = load(name)
    X, eps = fx["X"], float(fx["eps"])
    got, loss = device_updates(eng, X[None], [a[None] for a in nt.state(fx, 0)], eps, n=20, iterate=True, loss=True)
    tol = TOL["whole_run"]
    figures = {k: nt.rel_entry(a[0], b) for k, a, b in zip(("Z", "T", "V"), got, nt.state(fx, 20))}
    figures["loss"] = nt.rel_entry(loss[:, 0], fx["loss"])
    print(name, {k: "%.2e (tol %.2e)" % (v, tol[k]) for k, v in figures.items()})
    for metric, err in figures.items():
        assert err <= tol[metric], (metric, err, tol[metric])


# ---- bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ntf_n3_i33_j65_k6_silent", "ntf_n4_i5_j257_k16", "ntf_n5_i129_j7_k10"])
def test_iterate_equals_updates_and_runs_repeat_bit_for_bit(eng, name):
    fx = load(name)
    X, eps = fx["X"][None], float(fx["eps"])
    start = [a[None] for a in nt.state(fx, 0)]
    runs = [device_updates(eng, X, start, eps, n=5, iterate=it, loss=ls)
            for it, ls in ((True, True), (True, True), (False, True), (True, False))]
    first, first_loss = runs[0]
    for other, _ in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(first, other))
    assert np.array_equal(first_loss, runs[1][1])  # two runs are identical
    assert np.array_equal(first_loss, runs[2][1])  # loss[i] of assx_ntf_iterate equals assx_ntf_loss bit for bit
    assert first_loss.shape == (5, 1) and runs[3][1] is None


def test_batch_of_three_equals_three_singles_bit_for_bit(eng):
    fx = load("ntf_n3_i33_j65_k6_silent")
    X, eps = fx["X"], float(fx["eps"])
    states = [nt.state(fx, 0), nt.state(fx, 5), nt.state(fx, 19)]
    Xb = np.stack([X, X[:, ::-1].copy(), 2 * X[::-1] + 0.5])
    batch, batch_loss = device_updates(eng, Xb, [np.stack(a) for a in zip(*states)], eps, n=3, iterate=True, loss=True)
    for b, st in enumerate(states):
        for iterate in (True, False):
            single, loss = device_updates(eng, Xb[b:b + 1], [a[None] for a in st], eps, n=3, iterate=iterate, loss=True)
            assert all(np.array_equal(x[b], y[0]) for x, y in zip(batch, single)), (b, iterate)
            assert np.array_equal(batch_loss[:, b], loss[:, 0]), (b, iterate)


# ---- the class against the reference ---------------------------------------------------------------------------------
def check_run(model, out, fx, what):
    X = fx["X"]
    tol = TOL["whole_run"]
    figures = {k: nt.rel_entry(a, b) for k, a, b in zip(("Z", "T", "V"), out, nt.state(fx, 20))}
    figures["loss"] = nt.rel_entry(np.asarray(model.loss)[-20:], fx["loss"])
    print(what, {k: "%.2e (tol %.2e)" % (v, tol[k]) for k, v in figures.items()})
    for metric, err in figures.items():
        assert err <= tol[metric], (what, metric, err, tol[metric])


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_class_matches_reference(name):
    fx = load(name)
    X, eps = fx["X"], float(fx["eps"])
    (N, I, J), K = X.shape, fx["Z0"].shape[1]
    np.random.seed(int(fx["seed"]))
    model = cls()(K, eps)
    out = model(X, iteration=20)
    assert np.random.rand() == float(fx["rng_next"])  # the three draws of the reference, nothing else
    assert [a.shape for a in out] == [(N, K), (I, K), (K, J)] and all(a.dtype == np.float64 for a in out)
    assert all(np.array_equal(a, b) for a, b in zip(out, (model.partitioning, model.basis, model.activation)))
    assert model.target is X and model.n_basis == K and len(model.loss) == 20
    check_run(model, out, fx, name + " class")
    e_rec = nt.rel_entry(model.reconstruct(), nt.reconstruct(*out))
    print(name, "reconstruct %.2e" % e_rec)
    assert e_rec <= (K + 2) * 2.0 ** -53

    # a second call redraws (no warm start) and appends to the same list
    np.random.seed(int(fx["seed"]))
    again = model(X, iteration=20)
    assert np.random.rand() == float(fx["rng_next"])
    assert len(model.loss) == 40 and all(np.array_equal(a, b) for a, b in zip(out, again))
    assert list(model.loss)[:20] == list(model.loss)[20:]


@pytest.mark.parametrize("name", CLASS_NAMES[:2])
def test_class_steps_by_hand_and_overridden_step(name):
    fx = load(name)
    X, eps = fx["X"], float(fx["eps"])
    K = fx["Z0"].shape[1]
    np.random.seed(int(fx["seed"]))
    fast = cls()(K, eps)
    want = fast(X, iteration=20)

    by_hand = cls()(K, eps)
    by_hand(X, iteration=0)
    assert len(by_hand.loss) == 0
    by_hand.partitioning, by_hand.basis, by_hand.activation = nt.state(fx, 0)
    losses = []
    for _ in range(20):
        by_hand.update_once()
        losses.append(by_hand.compute_loss())
    assert all(isinstance(v, np.float64) for v in losses) and len(by_hand.loss) == 0
    got = (by_hand.partitioning, by_hand.basis, by_hand.activation)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and losses == list(fast.loss)

    calls = []

    class Counting(cls()):
        def update_once(self):
            calls.append(1)
            super().update_once()

    np.random.seed(int(fx["seed"]))
    slow = Counting(K, eps)
    assert not slow._fast_loop_ok() and fast._fast_loop_ok()
    out = slow(X, iteration=20)
    assert len(calls) == 20 and len(slow.loss) == 20
    assert all(np.array_equal(a, b) for a, b in zip(out, want)) and list(slow.loss) == list(fast.loss)
    check_run(slow, out, fx, name + " Python loop")


def test_class_extensions():
    from audio_source_separation_amd._device import to_device, torch
    fx = load("ntf_n2_i17_j40_k3")
    X, eps, seed = fx["X"], float(fx["eps"]), int(fx["seed"])
    np.random.seed(seed)
    plain = cls()(3, eps)
    want = plain(X, iteration=20)

    np.random.seed(seed)
    quiet = cls()(3, eps, recordable_loss=False)
    out = quiet(X, iteration=20)
    assert quiet.loss == [] and all(np.array_equal(a, b) for a, b in zip(out, want))

    np.random.seed(seed)
    on_device = cls()(3, eps)
    Xd = to_device(X, torch.float64, on_device._ensure_engine().dev)
    out = on_device(Xd, iteration=20)
    assert on_device.target is Xd and on_device._X.data_ptr() == Xd.data_ptr()  # no copy, no trip to the host
    assert all(np.array_equal(a, b) for a, b in zip(out, want)) and list(on_device.loss) == list(plain.loss)

    # a batch of two: the draws carry a leading B; each item equals its single run from the same draws
    Xb = np.stack([X, X[::-1].copy()])
    np.random.seed(seed)
    batched = cls()(3, eps)
    Zb, Tb, Vb = batched(Xb, iteration=20)
    assert Zb.shape == (2, 2, 3) and Tb.shape == (2, 17, 3) and Vb.shape == (2, 3, 40)
    assert len(batched.loss) == 20 and all(np.shape(v) == (2,) for v in batched.loss)
    assert batched.compute_loss().shape == (2,) and batched.reconstruct().shape == (2, 2, 17, 40)
    np.random.seed(seed)
    draws = [np.random.rand(2, 2, 3), np.random.rand(2, 17, 3), np.random.rand(2, 3, 40)]
    for b in range(2):
        single = cls()(3, eps)
        single(Xb[b], iteration=0)
        single.partitioning, single.basis, single.activation = (d[b] for d in draws)
        for _ in range(20):
            single.update_once()
        assert np.array_equal(single.partitioning, Zb[b]) and np.array_equal(single.basis, Tb[b])
        assert np.array_equal(single.activation, Vb[b]) and single.compute_loss() == batched.loss[19][b]


# ---- the size envelope -----------------------------------------------------------------------------------------------
BASE = dict(N=2, I=5, J=70, K=3)
ENVELOPE = [dict(BASE, K=k) for k in (1, 4, 15, 16, 17, 33, 64)] \
    + [dict(BASE, J=j) for j in (1, 63, 64, 65, 255, 256, 257, 513)] \
    + [dict(BASE, I=i) for i in (1, 2, 31, 33)] + [dict(BASE, N=n) for n in (1, 7, 32)]


@pytest.mark.parametrize("dims", ENVELOPE, ids=lambda d: "N%(N)d-I%(I)d-J%(J)d-K%(K)d" % d)
def test_envelope_against_restatement(eng, dims):
    N, I, J, K = dims["N"], dims["I"], dims["J"], dims["K"]
    X, Z, T, V = nt.synthetic(N, I, J, K, seed=N * 100000 + I * 1000 + J * 7 + K)
    want = nt.update(X, Z, T, V, 1e-12)
    got = one_update(eng, X, (Z, T, V), 1e-12)
    check(got, want, X, TOL["one_update"], "N=%d I=%d J=%d K=%d" % (N, I, J, K))


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from audio_source_separation_amd import _lib
    from audio_source_separation_amd._device import ptr, torch
    X, Z, T, V = nt.synthetic(33, 5, 12, 65, seed=3)  # arrays large enough for every size named below
    Xd, Zd, Td, Vd = up(eng, X[None], Z[None], T[None], V[None])
    ws = torch.empty(eng._L.assx_ntf_workspace_bytes(1, 32, 5, 12, 64, _lib.F64) * 2, dtype=torch.uint8, device=eng.dev)
    loss = eng.empty((4, 1), dtype=torch.float64)
    kept = down(Zd, Td, Vd)

    def raw(N, K, dtype, n_iter=None):
        if n_iter is None:
            return eng._L.assx_ntf_update(eng.ctx, ptr(Xd), ptr(Zd), ptr(Td), ptr(Vd), 1e-12, ptr(ws), 1, N, 5, 12, K,
                                          dtype, eng._st())
        return eng._L.assx_ntf_iterate(eng.ctx, n_iter, ptr(Xd), ptr(Zd), ptr(Td), ptr(Vd), 1e-12, ptr(loss), ptr(ws), 1,
                                       N, 5, 12, K, dtype, eng._st())

    for n_iter in (None, 2):
        assert raw(2, 0, _lib.F64, n_iter) == E_ARG and raw(2, 65, _lib.F64, n_iter) == E_ARG
        assert b"n_basis" in _lib.lib.assx_last_error(eng.ctx)
        assert raw(0, 3, _lib.F64, n_iter) == E_ARG and raw(33, 3, _lib.F64, n_iter) == E_ARG
        assert b"n_channels" in _lib.lib.assx_last_error(eng.ctx)
        assert raw(2, 3, _lib.F32, n_iter) == E_UNSUPPORTED and raw(2, 3, 7, n_iter) == E_ARG
    assert raw(2, 3, _lib.F64, -1) == E_ARG
    assert eng._L.assx_ntf_loss(eng.ctx, ptr(Xd), ptr(Zd), ptr(Td), ptr(Vd), ptr(loss), ptr(ws), 1, 2, 5, 12, 65,
                                _lib.F64, eng._st()) == E_ARG
    assert eng._L.assx_ntf_reconstruct(eng.ctx, ptr(Zd), ptr(Td), ptr(Vd), ptr(Xd), 1, 33, 5, 12, 3, _lib.F64,
                                       eng._st()) == E_ARG
    torch.cuda.synchronize(eng.dev)
    assert all(np.array_equal(a, b) for a, b in zip(kept, down(Zd, Td, Vd)))  # a refused call touches nothing

    X, Z, T, V = nt.synthetic(2, 5, 12, 3, seed=4)
    Xd, Zd, Td, Vd = up(eng, X[None], Z[None], T[None], V[None])
    need = eng._L.assx_ntf_workspace_bytes(1, 2, 5, 12, 3, _lib.F64)
    ws = eng.ntf_workspace(1, 2, 5, 12, 3)
    assert ws.numel() == need
    kept = down(Zd, Td, Vd)
    with pytest.raises(ValueError, match="workspace"):
        eng.ntf_update(Xd, Zd, Td, Vd, ws[:need - 1])
    with pytest.raises(ValueError, match="workspace"):
        eng.ntf_iterate(2, Xd, Zd, Td, Vd, ws[:need - 1])
    strided = torch.empty((1, 3, 24), dtype=torch.float64, device=eng.dev)[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        eng.ntf_update(Xd, Zd, Td, strided, ws)
    with pytest.raises(ValueError, match="shape"):
        eng.ntf_update(Xd, Zd, Td[:, :4].contiguous(), Vd, ws)
    with pytest.raises(ValueError, match="shape"):
        eng.ntf_loss(Xd, Zd, Td, Vd[:, :2].contiguous(), ws)
    with pytest.raises(ValueError, match="float64"):
        eng.ntf_update(Xd.float(), Zd, Td, Vd, ws)
    with pytest.raises(ValueError, match="loss"):
        eng.ntf_iterate(2, Xd, Zd, Td, Vd, ws, loss=eng.empty((1, 1), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_iter"):
        eng.ntf_iterate(-1, Xd, Zd, Td, Vd, ws)
    with pytest.raises(ValueError, match="n_basis"):
        eng.ntf_reconstruct(Zd[:, :, :0].contiguous(), Td[:, :, :0].contiguous(), Vd[:, :0].contiguous())
    with pytest.raises(ValueError, match="n_basis"):
        eng.ntf_workspace(1, 2, 5, 12, 65)
    torch.cuda.synchronize(eng.dev)
    assert all(np.array_equal(a, b) for a, b in zip(kept, down(Zd, Td, Vd)))
