"""MultichannelISNMF on the GPU: the class against the reference's recorded output (tests/golden/mnmf) and the NumPy
restatement (tests/mnmf_np.py), the reference's semantics, and the determinism of the HIP path."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mnmf_np as mn  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "mnmf")
NAMES = [os.path.basename(f)[:-4] for f in sorted(glob.glob(os.path.join(GOLDEN, "mnmf_*.npz")))]
ATTRS = ("basis", "activation", "latent", "spatial")


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def cls():
    from audio_source_separation_amd.bss.mnmf import MultichannelISNMF
    return MultichannelISNMF


def sizes(g):
    return g["Z0"].shape[0], g["Z0"].shape[1]  # N, K


@pytest.mark.parametrize("name", NAMES)
def test_class_matches_reference(name):
    g = load(name)
    N, K = sizes(g)
    snaps = {}

    def record(model):
        it = len(model.loss) - 1
        if it in (0, 1, 2, 5, 20):
            snaps[it] = {a: np.array(getattr(model, a)) for a in ATTRS + ("estimation",)}

    np.random.seed(int(g["seed"]))
    model = cls()(n_basis=K, n_sources=N, normalize=bool(g["normalize"]), callbacks=record)
    Y = model(g["X"], iteration=20)
    assert Y.shape == g["output"].shape and Y.dtype == np.complex128
    assert rel(snaps[0]["latent"], g["Z0"]) < 1e-15 and rel(snaps[0]["basis"], g["T0"]) == 0
    for it in (1, 2, 5, 20):
        tol = 1e-9 if it <= 5 else 1e-6
        for a in ATTRS:
            assert rel(snaps[it][a], g["%s_%d" % (a, it)]) < tol, (it, a)
        if it < 20:
            assert rel(snaps[it]["estimation"], g["estimation_%d" % it]) < 1e-9, it
    assert rel(Y, g["output"]) < 1e-6
    loss = np.asarray(model.loss)
    # the reference's loss carries ~1e-6 relative noise (its to_PSD shift); the closed form is exact
    assert np.max(np.abs(loss - g["loss"]) / np.abs(g["loss"])) < 1e-5
    closed = [mn.loss(g["X"], g["T0"], g["V0"], g["Z0"], mn.init_spatial(g["X"].shape[0], N, g["X"].shape[1]))]
    for it in (1, 2, 5, 20):
        s = snaps[it]
        closed.append(mn.loss(g["X"], s["basis"], s["activation"], s["latent"], s["spatial"]))
    got = loss[[0, 1, 2, 5, 20]]
    assert np.max(np.abs(got - closed) / np.abs(closed)) < 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_fast_loop_matches_reference(name):
    g = load(name)
    N, K = sizes(g)
    np.random.seed(int(g["seed"]))
    model = cls()(n_basis=K, n_sources=N, normalize=bool(g["normalize"]))
    Y = model(g["X"], iteration=20)
    assert np.max(np.abs(np.asarray(model.loss) - g["loss"]) / np.abs(g["loss"])) < 1e-5
    for a in ATTRS:
        assert rel(getattr(model, a), g["%s_20" % a]) < 1e-6, a
    assert rel(Y, g["output"]) < 1e-6
    assert np.array_equal(model.estimation, Y)


def test_riccati_matches_reference():
    import torch
    from audio_source_separation_amd.ops import Engine
    eng = Engine(device="cuda:0")
    r = np.load(os.path.join(GOLDEN, "riccati.npz"))
    for M in range(2, 9):
        A = torch.from_numpy(r["A_%d" % M]).to(eng.dev)
        B = torch.from_numpy(r["B_%d" % M]).to(eng.dev)
        status = eng.new_status(A.shape[0])
        H = eng.hermitian_riccati(A, B, status=status).cpu().numpy()
        assert rel(H, r["H_%d" % M]) < 1e-10, M
        assert int(status.max()) == 0
        # the rule for an all-zero weight sum: H = 0, no singular status
        Z = torch.zeros_like(A[:2])
        st = eng.new_status(2)
        H0 = eng.hermitian_riccati(Z, B[:2].contiguous(), status=st).cpu().numpy()
        assert np.all(H0 == 0) and int(st.max()) == 0


def test_zero_bin_reproduces_reference():
    g = load("mnmf_m3_n2_k4_silent")
    N, K = sizes(g)
    np.random.seed(int(g["seed"]))
    model = cls()(n_basis=K, n_sources=N)
    model(g["X"], iteration=20)
    H = model.spatial
    assert np.allclose(H[3], np.eye(3) / 3, rtol=0, atol=1e-15)  # silent bin: I / M after the normalisation
    assert np.all(model.basis[3] == 0)
    assert rel(H, g["spatial_20"]) < 1e-6


def test_warm_start_kwargs_and_estimation():
    g = load("mnmf_m2_n2_k3")
    N, K = sizes(g)
    np.random.seed(int(g["seed"]))
    model = cls()(n_basis=K, n_sources=N)
    model(g["X"], iteration=2, target="ignored")
    assert model.target == "ignored"  # __call__ keywords become attributes
    T2 = model.basis.copy()
    # a second call keeps every attribute (warm start): two more iterations = iterations 3, 4 of one run of 4
    model(g["X"], iteration=2)
    np.random.seed(int(g["seed"]))
    ref = cls()(n_basis=K, n_sources=N)
    Y4 = ref(g["X"], iteration=4)
    assert rel(model.basis, ref.basis) < 1e-12 and not np.array_equal(model.basis, T2)
    assert rel(model.estimation, Y4) < 1e-12
    # the estimation equals separate() of the final model
    assert rel(model.separate(g["X"]), model.estimation) == 0
    # recordable_loss=False: loss is None; the caller's arrays are not written into
    Z = g["Z0"].copy()
    m2 = cls()(n_basis=K, n_sources=N, recordable_loss=False)
    m2.latent = Z
    m2(g["X"], iteration=1)
    assert m2.loss is None and np.array_equal(Z, g["Z0"])
    # update_once refreshes the estimation
    est = m2.estimation.copy()
    m2.update_once()
    assert not np.array_equal(est, m2.estimation)


def test_callbacks_see_every_step():
    g = load("mnmf_m3_n2_k4")
    N, K = sizes(g)
    seen = []
    np.random.seed(int(g["seed"]))
    model = cls()(n_basis=K, n_sources=N, callbacks=lambda m: seen.append((len(m.loss), m.estimation.copy())))
    model(g["X"], iteration=3)
    assert [n for n, _ in seen] == [1, 2, 3, 4]
    assert rel(seen[2][1], g["estimation_2"]) < 1e-9


def test_bitwise_determinism_iterate_and_batch():
    import torch
    g = load("mnmf_m4_n4_k10")
    N, K = sizes(g)

    def run(cb=None, X=None):
        np.random.seed(int(g["seed"]))
        m = cls()(n_basis=K, n_sources=N, callbacks=cb)
        Y = m(g["X"] if X is None else X, iteration=5)
        return m, Y

    m1, Y1 = run()
    m2, Y2 = run()
    assert np.array_equal(Y1, Y2) and np.array_equal(np.asarray(m1.loss), np.asarray(m2.loss))
    m3, Y3 = run(cb=lambda m: None)  # per-step loop
    assert np.array_equal(Y1, Y3) and np.array_equal(np.asarray(m1.loss), np.asarray(m3.loss))
    for a in ATTRS:
        assert np.array_equal(getattr(m1, a), getattr(m3, a)), a
    # B = 3 utterances in one launch = three single calls
    rng = np.random.default_rng(5)
    Xs = [g["X"] * s for s in (1.0, 0.5, 2.0)]
    Xs[1] = Xs[1] + 1e-3 * (rng.standard_normal(g["X"].shape) + 1j * rng.standard_normal(g["X"].shape))
    M, F, T = g["X"].shape
    state = []
    for i in range(3):
        np.random.seed(100 + i)
        state.append((np.random.rand(N, K) * 1e-2 + 1 / N, np.random.rand(F, K), np.random.rand(K, T)))
    singles = []
    for i in range(3):
        m = cls()(n_basis=K, n_sources=N)
        Z = state[i][0] / state[i][0].sum(axis=0)
        m.latent, m.basis, m.activation = Z, state[i][1], state[i][2]
        singles.append((m(Xs[i], iteration=3), np.asarray(m.loss), m.spatial))
    mb = cls()(n_basis=K, n_sources=N)
    mb.latent = np.stack([s[0] / s[0].sum(axis=0) for s in state])
    mb.basis = np.stack([s[1] for s in state])
    mb.activation = np.stack([s[2] for s in state])
    Yb = mb(torch.from_numpy(np.stack(Xs)).cuda(), iteration=3).cpu().numpy()
    lb = np.asarray(mb.loss)
    for i in range(3):
        assert np.array_equal(Yb[i], singles[i][0])
        assert np.array_equal(lb[:, i], singles[i][1])
        assert np.array_equal(mb.spatial[i], singles[i][2])


def test_overridden_step_falls_back_to_the_step_loop():
    """A subclass that overrides a step is run by the step loop (the override is called once per iteration), and ends
    in the very bits of the one-call loop.  T = 70 leaves one ragged 64-frame tile."""
    M, N, K, F, T = 3, 2, 4, 5, 70
    rng = np.random.default_rng(12)
    X = rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))
    Z0 = rng.random((N, K)) * 1e-2 + 1 / N
    Z0 /= Z0.sum(axis=0)
    T0, V0 = rng.random((F, K)), rng.random((K, T))
    calls = []

    class Counting(cls()):
        def update_latent_sawada(self):
            calls.append(len(self.loss))
            super().update_latent_sawada()

    def run(C):
        m = C(n_basis=K, n_sources=N)
        m.latent, m.basis, m.activation = Z0.copy(), T0.copy(), V0.copy()
        return m, m(X, iteration=3)

    plain, Yp = run(cls())
    assert calls == []
    model, Y = run(Counting)
    assert calls == [1, 2, 3]
    assert np.array_equal(np.asarray(model.loss), np.asarray(plain.loss)) and len(model.loss) == 4
    for a in ATTRS:
        assert np.array_equal(getattr(model, a), getattr(plain, a)), a
    assert np.array_equal(Y, Yp) and np.array_equal(model.estimation, plain.estimation)


def _fullsize(M, N, K, F, T, n_iter, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))
    X *= rng.random((1, F, 1)) + 0.1
    np.random.seed(seed)
    Z0 = np.random.rand(N, K) * 1e-2 + 1 / N
    Z0 = Z0 / Z0.sum(axis=0)
    T0, V0 = np.random.rand(F, K), np.random.rand(K, T)
    np.random.seed(seed)
    model = cls()(n_basis=K, n_sources=N)
    Y = model(X, iteration=n_iter)
    return X, (T0, V0, Z0), model, Y


def test_fullsize_m4_two_iterations():
    M, N, K, F, T = 4, 4, 10, 1025, 4096
    X, (T0, V0, Z0), model, Y = _fullsize(M, N, K, F, T, 2, 7)
    Tb, V, Z, H = T0, V0, Z0, mn.init_spatial(M, N, F)
    losses = [mn.loss(X, Tb, V, Z, H)]
    for _ in range(2):
        Tb, V, Z, H = mn.update_once(X, Tb, V, Z, H)
        losses.append(mn.loss(X, Tb, V, Z, H))
    for a, ref in zip(ATTRS, (Tb, V, Z, H)):
        assert rel(getattr(model, a), ref) < 1e-9, a
    assert np.max(np.abs(np.asarray(model.loss) - losses) / np.abs(losses)) < 1e-9
    assert rel(Y, mn.separate(X, Tb, V, Z, H)) < 1e-9


def test_m8_against_restatement():
    M, N, K, F, T = 8, 4, 10, 129, 512
    X, (T0, V0, Z0), model, Y = _fullsize(M, N, K, F, T, 1, 9)
    Tb, V, Z, H = mn.update_once(X, T0, V0, Z0, mn.init_spatial(M, N, F))
    assert rel(model.spatial, H) < 1e-9
    assert rel(Y, mn.separate(X, Tb, V, Z, H)) < 1e-9


def test_fullsize_m8_one_call():
    M, N, K, F, T = 8, 4, 10, 1025, 4096
    X, (T0, V0, Z0), model, Y = _fullsize(M, N, K, F, T, 1, 11)
    loss = np.asarray(model.loss)
    assert Y.shape == (N, F, T) and np.all(np.isfinite(Y)) and np.all(np.isfinite(loss))
    # the loss of the entry model at full size, and the output on a slice of bins (separate works bin by bin)
    assert abs(loss[0] - mn.loss(X, T0, V0, Z0, mn.init_spatial(M, N, F))) / abs(loss[0]) < 1e-9
    s = slice(500, 532)
    Tb, V, Z, H = model.basis, model.activation, model.latent, model.spatial
    assert rel(Y[:, s], mn.separate(X[:, s], Tb[s], V, Z, H[s])) < 1e-9


def test_limits_raise_before_launch():
    C = cls()
    rng = np.random.default_rng(0)

    def X(M, F=5, T=16):
        return rng.standard_normal((M, F, T)) + 0j

    for kw, x in ((dict(n_basis=3), X(1)), (dict(n_basis=3), X(9)), (dict(n_basis=3, n_sources=9), X(2)),
                  (dict(n_basis=65), X(2)), (dict(n_basis=0), X(2)), (dict(n_basis=3, reference_id=2), X(2))):
        m = C(**kw)
        with pytest.raises(ValueError):
            m(x, iteration=1)
        assert not hasattr(m, "spatial")
    with pytest.raises(ValueError):
        C(n_basis=3)(np.broadcast_to(np.zeros(1, dtype=np.complex128), (2, 1 << 14, 1 << 13)), iteration=1)
    for kw in (dict(dtype="float32"), dict(author="Ozerov"), dict(author="x"), dict(hoge=1), dict(reference_id=-1)):
        with pytest.raises(ValueError):
            C(**kw)
    m = C(n_basis=3)
    m.basis = np.ones((4, 3))  # wrong n_bins
    with pytest.raises(ValueError):
        m(X(2), iteration=1)
