"""Covariance-domain MultichannelISNMF (algorithm/nmf.py) on the GPU: the class against the reference's recorded output
(tests/golden/covnmf) and the NumPy restatement (tests/covnmf_np.py), the reference's semantics, the C-ABI's refusals and
the determinism of the HIP path.

Bounds: states within 1e-9 of the reference up to iteration 5 and within 1e-6 at iteration 20, every loss within 1e-9
relative -- the bounds of tests/test_gpu_mnmf.py, caps far above what the restatement itself shows on the CPU (3.1e-13,
1.2e-11 and 2.0e-12).  Measured on the MI355X over the ten fixtures (the test prints them per fixture): states up to
iteration 5 within 3.5e-12 (covnmf_m8_f3_t70_k2_s9_nonorm; 6.5e-14 with the normalisation on), at iteration 20 within
2.5e-10 (covnmf_m2_f3_t20_k64_s2: 64 bases on 20 frames; 2.6e-11 for the next one), every loss within 2.0e-12.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import covnmf_np as cv  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "covnmf")
NAMES = [os.path.basename(f)[:-4] for f in cv.fixtures(GOLDEN)]
ATTRS = (("spatial", "H"), ("basis", "T"), ("activation", "V"))


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def cls():
    from audio_source_separation_amd.algorithm.nmf import MultichannelISNMF
    return MultichannelISNMF


def recording_cls(snaps):
    """The class with a callback after every `update_once`: a subclass, so the loop is the stepwise one."""
    class Recording(cls()):
        def update_once(self):
            super().update_once()
            self.n_done = getattr(self, "n_done", 0) + 1
            if self.n_done in cv.SNAP_ITERS:
                snaps[self.n_done] = {a: np.array(getattr(self, a)) for a, _ in ATTRS}
    return Recording


def new(g, klass=None, **kw):
    np.random.seed(int(g["seed"]))
    return (klass or cls())(n_basis=int(g["n_basis"]), normalize=bool(g["normalize"]), eps=float(g["eps"]), **kw)


def state(g, it):
    return g["T_%d" % it], g["V_%d" % it], g["H_%d" % it]


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


@pytest.mark.parametrize("name", NAMES)
def test_class_matches_reference(name):
    """Through the front door (one assx_covnmf_iterate call) and with a callback after every iteration (the stepwise
    loop): both against the fixture, and against each other bit for bit."""
    g = load(name)
    front = new(g)
    out = front(g["X"], iteration=cv.N_ITER)
    assert np.random.rand() == float(g["rng_next"])
    snaps = {}
    step = new(g, recording_cls(snaps))
    assert not step._fast_loop_ok() and front._fast_loop_ok()
    step(g["X"], iteration=cv.N_ITER)
    worst = {}
    for it in cv.SNAP_ITERS:
        tol = 1e-9 if it <= 5 else 1e-6
        for a, n in ATTRS:
            d = cv.rel(snaps[it][a], g["%s_%d" % (n, it)])
            worst["early" if it <= 5 else "late"] = max(worst.get("early" if it <= 5 else "late", 0.0), d)
            assert d < tol, (it, a, d)
    dl = float(np.max(np.abs(np.asarray(step.loss) - g["loss"]) / np.abs(g["loss"])))
    print("%-36s states <= it 5 %.1e, it 20 %.1e, loss %.1e" % (name, worst["early"], worst["late"], dl))
    assert len(step.loss) == cv.N_ITER and dl < 1e-9
    for (a, n), o in zip(ATTRS, out):
        assert cv.rel(o, g["%s_%d" % (n, cv.N_ITER)]) < 1e-6, a
        assert np.array_equal(getattr(front, a), snaps[cv.N_ITER][a]), a  # the fast loop is the stepwise loop
        assert np.array_equal(o, getattr(front, a))
    assert list(front.loss) == list(step.loss)


def test_two_runs_give_the_same_bits():
    g = load("covnmf_m4_f6_t64_k4_s5")
    runs = []
    for _ in range(2):
        model = new(g)
        runs.append(model(g["X"], iteration=5) + (np.asarray(model.loss),))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ("covnmf_m3_f4_t33_k2_s3", "covnmf_m8_f3_t70_k2_s9_nonorm", "covnmf_m2_f3_t20_k64_s2"))
def test_stand_alone_methods_match_restatement(name):
    """Every public step on its own from the recorded state after iteration 2, against the restatement: within 1e-9, the
    bound of a state up to iteration 5 (tests/test_gpu_covnmf_envelope.py holds single steps to measured tolerances).
    reconstruct: a sum of K <= 64 products whose absolute values add up to no more than the largest diagonal entry (the
    weights are positive, the H_k positive semi-definite), so it is within (K + 1) 2^-53 < 1e-14 of that entry."""
    g = load(name)
    X, eps, norm = g["X"], float(g["eps"]), bool(g["normalize"])
    Tb, V, H = state(g, 2)

    def fresh():
        model = new(g)
        model(X, iteration=0, spatial=H, basis=Tb, activation=V)
        assert np.array_equal(model.spatial, H) and np.array_equal(model.basis, Tb) and model.loss == []
        return model

    m = fresh()
    m.update_basis()
    assert cv.rel(m.basis, cv.update_basis(X, Tb, V, H, eps)) < 1e-9
    assert np.array_equal(m.activation, V) and np.array_equal(m.spatial, H)
    m = fresh()
    m.update_activation()
    assert cv.rel(m.activation, cv.update_activation(X, Tb, V, H, eps)) < 1e-9
    m = fresh()
    m.update_spatial()
    assert cv.rel(m.spatial, cv.update_spatial(X, Tb, V, H, norm, eps)) < 1e-9
    assert np.array_equal(m.spatial, m.spatial.conj().swapaxes(-1, -2))
    m = fresh()
    assert cv.rel(m.reconstruct(), cv.reconstruct(Tb, V, H)) < 1e-14
    m.update_once()
    for got, want in zip((m.basis, m.activation, m.spatial), cv.update_once(X, Tb, V, H, norm, eps)):
        assert cv.rel(got, want) < 1e-9
    assert m.loss == []
    m = fresh()
    m.update(iteration=1)
    assert len(m.loss) == 1
    assert abs(m.loss[0] - cv.loss(X, m.basis, m.activation, m.spatial, eps)) < 1e-9 * abs(m.loss[0])


def test_warm_start_loss_accumulation_and_copies():
    g = load("covnmf_m2_f5_t40_k3_s3")
    X = g["X"]
    model = new(g)
    out = model(X, iteration=2)
    for o, (a, n) in zip(out, ATTRS):
        assert cv.rel(o, g["%s_2" % n]) < 1e-9
        assert o is not getattr(model, a) and not np.shares_memory(o, getattr(model, a))
        o[...] = 0  # a copy: the model does not see it
        assert cv.rel(getattr(model, a), g["%s_2" % n]) < 1e-9
    assert len(model.loss) == 2
    state_rng = np.random.get_state()[1].copy()
    model(X, iteration=3)  # warm start through hasattr: no draw, the run goes on
    assert np.array_equal(np.random.get_state()[1], state_rng)
    assert len(model.loss) == 5 and np.max(np.abs(np.asarray(model.loss) - g["loss"][:5]) / np.abs(g["loss"][:5])) < 1e-9
    for a, n in ATTRS:
        assert cv.rel(getattr(model, a), g["%s_5" % n]) < 1e-9
    # keywords become attributes; a warm start given at the call
    other = cls()(n_basis=3)
    other(X, iteration=0, basis=g["T_1"], activation=g["V_1"], spatial=g["H_1"], note="kept")
    assert other.note == "kept" and other.spatial.dtype == np.complex128
    other.update(iteration=1)
    for a, n in ATTRS:
        assert cv.rel(getattr(other, a), g["%s_2" % n]) < 1e-9
    real_start = cls()(n_basis=3)
    real_start(X, iteration=0, spatial=np.tile(np.eye(2), (5, 3, 1, 1)))
    assert real_start.spatial.dtype == np.complex128


def test_singular_model_raises_at_the_end_of_the_call():
    g = load("covnmf_m2_f5_t40_k3_s3")
    F, T = g["X"].shape[:2]
    model = cls()(n_basis=3, eps=0.0)
    with pytest.raises(np.linalg.LinAlgError):
        model(g["X"], iteration=2, basis=np.zeros((F, 3)))
    assert len(model.loss) == 2  # the whole call ran; the status word, not a fault, refused it
    good = new(g)
    good(g["X"], iteration=1)  # the device is as usable as before
    assert cv.rel(good.basis, g["T_1"]) < 1e-9


def test_engine_refuses_wrong_arrays(eng):
    import torch
    g = load("covnmf_m2_f5_t40_k3_s3")
    dev = eng.dev
    X = torch.from_numpy(g["X"]).to(dev)
    Tb, V, H = (torch.from_numpy(a).to(dev) for a in state(g, 1))
    ws = eng.covnmf_workspace(2, 5, 40, 3)
    eng.covnmf_update_basis(X, Tb.clone(), V, H, ws)
    with pytest.raises(ValueError):
        eng.covnmf_update_basis(X, Tb.clone(), V[:, :-1].contiguous(), H, ws)
    with pytest.raises(ValueError):
        eng.covnmf_update_basis(X, Tb.float(), V, H, ws)
    with pytest.raises(ValueError):
        eng.covnmf_update_basis(X, Tb.clone(), V, H, ws[:16])
    with pytest.raises(ValueError):
        eng.covnmf_loss(X, Tb, V, H, ws, loss=torch.zeros(1, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        eng.covnmf_iterate(3, X, Tb.clone(), V.clone(), H.clone(), ws, loss=torch.zeros(2, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        eng.covnmf_workspace(9, 5, 40, 3)
    with pytest.raises(ValueError):
        eng.covnmf_workspace(2, 5, 40, 65)


def test_c_abi_refuses_what_lies_outside_the_envelope(eng):
    """cv_check: ASSX_E_ARG for sizes and codes that mean nothing, ASSX_E_UNSUPPORTED outside the envelope, before any
    pointer is looked at; then ASSX_E_NULL for the pointers."""
    from audio_source_separation_amd import _lib
    L, ctx, null = _lib.lib, eng.ctx, ctypes.c_void_p(0)
    E_ARG, E_UNSUPPORTED, E_NULL = -1, -2, -3

    def basis(M, F, T, K, dt):
        return L.assx_covnmf_update_basis(ctx, null, null, null, null, 1e-12, null, null, M, F, T, K, dt, null)

    for M, F, T, K in ((4, 0, 5, 2), (4, 5, 0, 2), (4, -1, 5, 2)):
        assert basis(M, F, T, K, _lib.F64) == E_ARG, (M, F, T, K)
    assert basis(4, 5, 6, 2, 7) == E_ARG
    assert basis(4, 5, 6, 2, _lib.F32) == E_UNSUPPORTED
    for M, F, T, K in ((1, 5, 6, 2), (9, 5, 6, 2), (4, 5, 6, 0), (4, 5, 6, 65), (8, 2048, 2048, 2),
                       (2, 2 ** 31 - 1, 2 ** 31 - 1, 2)):
        assert basis(M, F, T, K, _lib.F64) == E_UNSUPPORTED, (M, F, T, K)
    assert basis(8, 5, 6, 64, _lib.F64) == E_NULL and basis(2, 1, 1, 1, _lib.F64) == E_NULL
    sizes = (4, 5, 6, 2, _lib.F64, null)
    assert L.assx_covnmf_update_activation(ctx, null, null, null, null, 1e-12, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_update_spatial(ctx, null, null, null, null, 1, 1e-12, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_reconstruct(ctx, null, null, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_loss(ctx, null, null, null, null, 1e-12, null, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_iterate(ctx, 1, 1, null, null, null, null, 1e-12, null, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_iterate(ctx, -1, 1, null, null, null, null, 1e-12, null, null, null, *sizes) == E_ARG
    assert L.assx_covnmf_reconstruct(ctx, null, null, null, null, 9, 5, 6, 2, _lib.F64, null) == E_UNSUPPORTED
    assert L.assx_covnmf_loss(ctx, null, null, null, null, 1e-12, null, null, null, 4, 5, 6, 2, _lib.F32,
                              null) == E_UNSUPPORTED
    # normalize is 0 or 1: checked once the arrays are there
    import torch
    g = load("covnmf_m2_f5_t40_k3_s3")
    X = torch.from_numpy(g["X"]).to(eng.dev)
    Tb, V, H = (torch.from_numpy(a).to(eng.dev) for a in state(g, 1))
    ws = eng.covnmf_workspace(2, 5, 40, 3)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.assx_covnmf_update_spatial(ctx, p(X), p(Tb), p(V), p(H), 2, 1e-12, null, p(ws), 2, 5, 40, 3, _lib.F64,
                                        null) == E_ARG
    assert L.assx_covnmf_iterate(ctx, 1, 2, p(X), p(Tb), p(V), p(H), 1e-12, null, null, p(ws), 2, 5, 40, 3, _lib.F64,
                                 null) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(H.cpu().numpy(), g["H_1"])  # refused before anything was launched
