"""LDPSDTF on the GPU: every entry point against the reference's recorded states (tests/golden/psdtf) and the NumPy
restatement (tests/psdtf_np.py), the class against the reference's recorded front-door runs, and the determinism of the
HIP path.

Metrics (tests/psdtf_np.py): V per basis max|a - b| / max|b|, H entry-wise, loss |a - b| / (|b| + n_bins n_frames);
tolerances come from tests/golden/psdtf/tolerances.json (tools/psdtf_tolerance_probe.py).  Every figure is printed before
it is asserted (pytest -s shows them)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import psdtf_np as pt  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [os.path.basename(f)[:-4] for f in pt.fixture_files()]
CLASS_NAMES = ["psdtf_m4_t10_k2", "psdtf_m16_t33_k3", "psdtf_m3_t257_k4", "psdtf_m33_t20_k2", "psdtf_m8_t20_k3_nonorm"]
BATCH_NAMES = ["psdtf_m4_t10_k2", "psdtf_m16_t33_k3", "psdtf_m64_t5_k3"]
TOL = pt.tolerances()
SIZES = (1, 2, 5, 16, 33, 64)


def load(name):
    return np.load(os.path.join(pt.GOLDEN, name + ".npz"))


def cls():
    from audio_source_separation_amd.algorithm.psdtf import LDPSDTF
    return LDPSDTF


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(dtype="float64")


def up(eng, *arrays):
    from audio_source_separation_amd._device import to_device, torch
    return [to_device(np.ascontiguousarray(a), torch.float64, eng.dev) for a in arrays]


def down(*tensors):
    from audio_source_separation_amd._device import to_numpy
    return [to_numpy(t) for t in tensors]


def problem(fx, it):
    """(X (T,M,M), V (K,M,M), H (K,T), eps, normalize) of a fixture at a recorded state"""
    V, H = pt.state(fx, it)
    return pt.frames_first(fx["X"]), pt.kmm(V), H, float(fx["eps"]), bool(fx["normalize"])


class Device:
    """One problem (or a batch of equal shapes) on the device."""

    def __init__(self, eng, X, V, H):
        self.eng = eng
        batched = X.ndim == 4
        self.X, self.V, self.H = up(eng, *[a if batched else a[None] for a in (X, V, H)])
        B, K, M = self.V.shape[:3]
        self.ws = eng.psdtf_workspace(B, M, self.H.shape[2], K)
        self.status = eng.new_status(B)

    def model(self):
        V, H = down(self.V, self.H)
        assert int(self.status.max().item()) == 0
        return V, H


def check(V, H, Vw, Hw, tol, what):
    figures = {"V": pt.v_metric(V, Vw), "H": pt.h_metric(H, Hw)}
    print(what, {k: "%.2e (tol %.2e)" % (v, tol[k]) for k, v in figures.items()})
    for metric, err in figures.items():
        assert err <= tol[metric], (what, metric, err, tol[metric])


# ---- entry points against the fixtures -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_update_from_every_recorded_state(eng, name):
    fx = load(name)
    for it in pt.START_ITERS:
        X, V, H, eps, norm = problem(fx, it)
        d = Device(eng, X, V, H)
        eng.psdtf_update(d.X, d.V, d.H, d.ws, eps=eps, normalize=norm, status=d.status)
        Vn, Hn = d.model()
        Vw, Hw = pt.state(fx, it + 1)
        check(Vn[0], Hn[0], pt.kmm(Vw), Hw, TOL["one_update"], "%s %d->%d" % (name, it, it + 1))


@pytest.mark.parametrize("name", NAMES)
def test_stages_against_restatement(eng, name):
    fx = load(name)
    tol = TOL["one_update"]
    for it in (0, 4):
        X, V, H, eps, _ = problem(fx, it)
        d = Device(eng, X, V, H)
        eng.psdtf_update_basis(d.X, d.V, d.H, d.ws, eps=eps, status=d.status)
        Vn, Hn = d.model()
        Vr = pt.update_basis(X, V, H, eps)
        assert np.array_equal(Hn[0], H)
        assert np.array_equal(Vn[0], np.transpose(Vn[0], (0, 2, 1)))  # to_psd leaves exactly symmetric bases
        eng.psdtf_update_activation(d.X, d.V, d.H, eps=eps, status=d.status)
        Va, Ha = d.model()
        assert np.array_equal(Va, Vn)
        Hr = pt.update_activation(X, Vn[0], H, eps)  # from the device's own basis: the stage alone
        eng.psdtf_normalize(d.V, d.H)
        Vm, Hm = d.model()
        Vq, Hq = pt.normalize(Va[0], Ha[0])
        # two orders of summing the M non-negative diagonal entries differ by at most (M - 1) 2^-52 of the trace, the
        # division or product adds a rounding on either side
        tol_norm = (X.shape[1] + 1) * 2.0 ** -52
        figures = {"basis": (pt.v_metric(Vn[0], Vr), tol["V"]), "activation": (pt.h_metric(Ha[0], Hr), tol["H"]),
                   "normalize V": (pt.v_metric(Vm[0], Vq), tol_norm), "normalize H": (pt.h_metric(Hm[0], Hq), tol_norm)}
        print(name, it, {k: "%.2e (tol %.2e)" % v for k, v in figures.items()})
        for k, (err, t) in figures.items():
            assert err <= t, (k, err, t)


@pytest.mark.parametrize("name", NAMES)
def test_loss_and_reconstruct_against_restatement(eng, name):
    fx = load(name)
    M, _, T = fx["X"].shape
    for it in (0, 20):
        X, V, H, eps, _ = problem(fx, it)
        d = Device(eng, X, V, H)
        loss, rec = down(eng.psdtf_loss(d.X, d.V, d.H, d.ws, eps=eps, status=d.status), eng.psdtf_reconstruct(d.V, d.H))
        # a sum of K products: K + 1 roundings of 2^-53 each relative to the sum of magnitudes, whatever the order
        want = pt.reconstruct(V, H)
        bound = (V.shape[0] + 1) * 2.0 ** -53 * pt.reconstruct(np.abs(V), np.abs(H))
        e_loss = pt.loss_metric(loss[0], pt.loss(X, V, H, eps), M, T)
        print(name, it, "loss %.2e (tol %.2e) reconstruct excess %.2e" % (e_loss, TOL["one_update"]["loss"],
                                                                          np.max(np.abs(rec[0] - want) - bound)))
        assert loss.shape == (1,) and rec.shape == (1, T, M, M)
        assert e_loss <= TOL["one_update"]["loss"] and np.all(np.abs(rec[0] - want) <= bound)
        if it == 20:
            e_fx = pt.loss_metric(loss[0], fx["loss"][19], M, T)
            print(name, "loss at 20 against the recorded list %.2e" % e_fx)
            assert e_fx <= TOL["one_update"]["loss"]
        Vd, Hd = d.model()
        assert np.array_equal(Vd[0], V) and np.array_equal(Hd[0], H)  # read-only calls


@pytest.mark.parametrize("name", NAMES)
def test_iterate_20_against_the_recorded_run(eng, name):
    from audio_source_separation_amd._device import torch
    fx = load(name)
    M, _, T = fx["X"].shape
    X, V, H, eps, norm = problem(fx, 0)
    d = Device(eng, X, V, H)
    block = eng.empty((20, 1), dtype=torch.float64)
    eng.psdtf_iterate(20, d.X, d.V, d.H, d.ws, eps=eps, normalize=norm, loss=block, status=d.status)
    Vn, Hn = d.model()
    Vw, Hw = pt.state(fx, 20)
    check(Vn[0], Hn[0], pt.kmm(Vw), Hw, TOL["whole_run"], name + " 20 iterations")
    e_loss = pt.loss_metric(down(block)[0][:, 0], fx["loss"], M, T)
    print(name, "loss list %.2e (tol %.2e)" % (e_loss, TOL["whole_run"]["loss"]))
    assert e_loss <= TOL["whole_run"]["loss"]


@pytest.mark.parametrize("n", SIZES)
def test_to_psd_definite_indefinite_and_diagonal(eng, n):
    eps = 1e-3
    for kind, A in pt.psd_cases(n, 40 + n):
        if kind != "diagonal":
            A = A + 0.01 / n * np.triu(np.ones((n, n)), 1)  # not symmetric: to_psd symmetrises
        want = pt.to_psd(A, eps)
        (Ad,) = up(eng, A)
        (got,) = down(eng.psdtf_to_psd(Ad, eps=eps))
        err = pt.mat_metric(got, want)
        # eigenvalues to a few ulps of the spectral radius per dimension, as for the NumPy model of the kernel
        print(n, kind, "%.2e (tol %.2e)" % (err, 64 * n * 2.0 ** -52))
        assert err <= 64 * n * 2.0 ** -52 and np.array_equal(got, np.transpose(got, (0, 2, 1)))
        # either path changes the diagonal alone: off it, the result is the symmetrised input bit for bit.  Which path ran
        # cannot be seen from outside, by design: on a definite matrix the shortcut and the eigen path give the same shift
        S = (A + np.transpose(A, (0, 2, 1))) / 2
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(got[:, off], S[:, off])
        if kind == "definite":  # delta = 0 on either path: the diagonal is s_ii + eps tr, tr summed in index order
            tr = np.zeros(len(S))
            for i in range(n):
                tr = tr + S[:, i, i]
            idx = np.arange(n)
            assert np.array_equal(got[:, idx, idx], S[:, idx, idx] + eps * tr[:, None])


# ---- determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["psdtf_m16_t33_k3", "psdtf_m3_t257_k4", "psdtf_m8_t20_k3_nonorm"])
def test_iterate_equals_repeated_update_and_loss_bit_for_bit(eng, name):
    from audio_source_separation_amd._device import torch
    fx = load(name)
    X, V, H, eps, norm = problem(fx, 0)
    runs = []
    for mode in ("iterate", "iterate", "single"):
        d = Device(eng, X, V, H)
        block = eng.empty((5, 1), dtype=torch.float64)
        if mode == "iterate":
            eng.psdtf_iterate(5, d.X, d.V, d.H, d.ws, eps=eps, normalize=norm, loss=block, status=d.status)
        else:
            for i in range(5):
                eng.psdtf_update(d.X, d.V, d.H, d.ws, eps=eps, normalize=norm, status=d.status)
                eng.psdtf_loss(d.X, d.V, d.H, d.ws, eps=eps, loss=block[i], status=d.status)
        runs.append(d.model() + tuple(down(block)))
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))


def test_batch_equals_single_calls_bit_for_bit(eng):
    from audio_source_separation_amd._device import torch
    # three different problems of one shape: the target of one fixture, its recorded states at three iterations, and the
    # targets scaled differently
    for name in BATCH_NAMES:
        fx = load(name)
        probs = [problem(fx, it) for it in (0, 2, 5)]
        scale = (1.0, 0.5, 3.0)
        Xs = np.stack([p[0] * s for p, s in zip(probs, scale)])
        Vs, Hs = np.stack([p[1] for p in probs]), np.stack([p[2] for p in probs])
        eps, norm = probs[0][3], probs[0][4]
        d = Device(eng, Xs, Vs, Hs)
        block = eng.empty((3, 3), dtype=torch.float64)
        eng.psdtf_iterate(3, d.X, d.V, d.H, d.ws, eps=eps, normalize=norm, loss=block, status=d.status)
        Vb, Hb = d.model()
        lb = down(block)[0]
        for b in range(3):
            s = Device(eng, Xs[b], Vs[b], Hs[b])
            one = eng.empty((3, 1), dtype=torch.float64)
            eng.psdtf_iterate(3, s.X, s.V, s.H, s.ws, eps=eps, normalize=norm, loss=one, status=s.status)
            V1, H1 = s.model()
            assert np.array_equal(V1[0], Vb[b]) and np.array_equal(H1[0], Hb[b]), (name, b)
            assert np.array_equal(down(one)[0][:, 0], lb[:, b]), (name, b)


# ---- the class ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASS_NAMES)
def test_class_against_the_reference_front_door(name):
    fx = load(name)
    M, _, T = fx["X"].shape
    np.random.seed(int(fx["seed"]))
    model = cls()(n_basis=fx["H0"].shape[0], normalize=bool(fx["normalize"]), eps=float(fx["eps"]))
    V, H = model(fx["X"], iteration=20)
    assert np.random.rand() == float(fx["rng_next"])  # the same draws in the same order
    assert V.shape == fx["basis_20"].shape and H.shape == fx["activation_20"].shape
    check(pt.kmm(V), H, pt.kmm(fx["basis_20"]), fx["activation_20"], TOL["whole_run"], name + " class")
    assert len(model.loss) == 20
    e_loss = pt.loss_metric(np.array(model.loss), fx["loss"], M, T)
    print(name, "loss list %.2e (tol %.2e)" % (e_loss, TOL["whole_run"]["loss"]))
    assert e_loss <= TOL["whole_run"]["loss"]
    assert np.array_equal(model.basis, V) and np.array_equal(model.activation, H)
    rec = model.reconstruct()
    assert rec.shape == fx["X"].shape
    # a sum of K signed products: K + 1 roundings of 2^-53 each relative to the sum of magnitudes, whatever the order
    bound = (H.shape[0] + 1) * 2.0 ** -53 * pt.reconstruct(np.abs(pt.kmm(V)), np.abs(H))
    assert np.all(np.abs(np.transpose(rec, (2, 0, 1)) - pt.reconstruct(pt.kmm(V), H)) <= bound)


def test_class_warm_start_second_call_and_switches():
    fx = load("psdtf_m16_t33_k3")
    X, eps = fx["X"], float(fx["eps"])
    M, _, T = X.shape
    LD = cls()
    # warm start from the recorded state at 4, one more iteration: the recorded state at 5; the RNG is left alone
    model = LD(n_basis=3, eps=eps)
    model.basis, model.activation = pt.state(fx, 4)
    state = np.random.get_state()[1].copy()
    V, H = model(X, iteration=1)
    assert np.array_equal(np.random.get_state()[1], state)
    check(pt.kmm(V), H, pt.kmm(fx["basis_5"]), fx["activation_5"], TOL["one_update"], "warm start 4->5")
    assert len(model.loss) == 1 and pt.loss_metric(model.loss[0], fx["loss"][4], M, T) <= TOL["one_update"]["loss"]
    # a second call continues from where the first one stopped and keeps appending
    np.random.seed(int(fx["seed"]))
    model = LD(n_basis=3, eps=eps)
    model(X, iteration=4)
    V, H = model(X, iteration=1)
    assert len(model.loss) == 5
    check(pt.kmm(V), H, pt.kmm(fx["basis_5"]), fx["activation_5"], TOL["whole_run"], "4 + 1 iterations")
    # five iterations in one call, the yardstick of the bit comparisons below
    np.random.seed(int(fx["seed"]))
    model = LD(n_basis=3, eps=eps)
    V, H = model(X, iteration=5)
    # keyword arguments of the call become attributes; recordable_loss=False leaves the list empty, same model
    np.random.seed(int(fx["seed"]))
    quiet = LD(n_basis=2, eps=eps, recordable_loss=False)
    Vq, Hq = quiet(X, iteration=5, n_basis=3)
    assert quiet.n_basis == 3 and quiet.loss == []
    assert np.array_equal(Vq, V) and np.array_equal(Hq, H)
    # a subclass that overrides a step takes the slow loop, with the same bits
    calls = []

    class Sub(LD):
        def update_once(self):
            calls.append(1)
            super().update_once()

    np.random.seed(int(fx["seed"]))
    sub = Sub(n_basis=3, eps=eps)
    Vs, Hs = sub(X, iteration=5)
    assert len(calls) == 5 and not sub._fast_loop_ok() and model._fast_loop_ok()
    assert np.array_equal(Vs, V) and np.array_equal(Hs, H) and list(sub.loss) == list(model.loss)
    for algorithm, exc in (("em", NotImplementedError), ("gradient", ValueError)):
        with pytest.raises(exc):
            LD(n_basis=3, algorithm=algorithm)(X, iteration=1)


def test_class_batched_target():
    fx = load("psdtf_m4_t10_k2")
    X = np.stack([fx["X"], 2.0 * fx["X"]])
    np.random.seed(3)
    model = cls()(n_basis=2)
    V, H = model(X, iteration=3)
    assert V.shape == (2, 4, 4, 2) and H.shape == (2, 2, 10) and len(model.loss) == 3 and model.loss[0].shape == (2,)
    np.random.seed(3)
    dV, dH = np.random.rand(2, 2, 4), np.random.rand(2, 2, 10)
    for b in range(2):
        single = cls()(n_basis=2)
        single.basis = pt.mmk(dV[b][:, :, None] * np.eye(4))
        single.activation = dH[b]
        V1, H1 = single(X[b], iteration=3)
        assert np.array_equal(V1, V[b]) and np.array_equal(H1, H[b])
        assert [l[b] for l in model.loss] == list(single.loss)


def test_class_refuses_what_lies_outside_the_envelope():
    LD = cls()
    X = np.tile(np.eye(5)[:, :, None], (1, 1, 6))
    skew = X.copy()
    skew[0, 1] = 1.0
    with pytest.raises(ValueError, match="float64"):
        LD(3, dtype="float32")
    for model, target, what in ((LD(0), X, "n_basis"), (LD(65), X, "n_basis"), (LD(3), np.ones((65, 65, 2)), "n_bins"),
                                (LD(3), np.ones((5, 4, 6)), "square"), (LD(3), np.ones((5, 5, 0)), "empty"),
                                (LD(3), np.ones((5, 5)), "dims"), (LD(3), X.astype(np.complex128), "real"),
                                (LD(3), skew, "symmetric")):
        with pytest.raises(ValueError, match=what):
            model(target, iteration=1)
        assert model._engine is None
    model = LD(3)
    model.basis = np.ones((5, 5, 3), dtype=np.complex128)
    with pytest.raises(ValueError, match="real"):
        model(X, iteration=1)


def test_c_abi_refuses_what_lies_outside_the_envelope(eng):
    """pt_check behind the Engine's own refusals: ASSX_E_ARG outside the envelope, ASSX_E_UNSUPPORTED for float32, before
    any pointer is looked at."""
    import ctypes
    from audio_source_separation_amd import _lib
    L, ctx, null = _lib.lib, eng.ctx, ctypes.c_void_p(0)
    E_ARG, E_UNSUPPORTED, E_NULL = -1, -2, -3

    def update(B, M, T, K, dt):
        return L.assx_psdtf_update(ctx, null, null, null, 1e-12, 1, null, null, B, M, T, K, dt, null)

    for B, M, T, K in ((0, 4, 5, 2), (1, 0, 5, 2), (1, 65, 5, 2), (1, 4, 0, 2), (1, 4, 5, 0), (1, 4, 5, 65),
                       (1 << 12, 4, 1 << 12, 2), (1 << 16, 4, 1, 2)):
        assert update(B, M, T, K, _lib.F64) == E_ARG, (B, M, T, K)
    assert update(1, 4, 5, 2, 7) == E_ARG
    assert update(1, 4, 5, 2, _lib.F32) == E_UNSUPPORTED
    assert update(1, 64, 5, 64, _lib.F64) == E_NULL and update((1 << 16) - 1, 4, 1, 2, _lib.F64) == E_NULL
    for n_mat, M in ((0, 4), (1 << 24, 4), (1, 0), (1, 65)):
        assert L.assx_psdtf_to_psd(ctx, null, n_mat, M, 1e-12, null) == E_ARG
    assert L.assx_psdtf_to_psd(ctx, null, 1, 4, 1e-12, null) == E_NULL
    assert L.assx_psdtf_iterate(ctx, -1, null, null, null, 1e-12, 1, null, null, null, 1, 4, 5, 2, _lib.F64, null) == E_ARG
    assert L.assx_psdtf_loss(ctx, null, null, null, 1e-12, null, null, null, 1, 65, 5, 2, _lib.F64, null) == E_ARG
    assert L.assx_psdtf_reconstruct(ctx, null, null, null, 1, 4, 5, 2, _lib.F32, null) == E_UNSUPPORTED
    assert L.assx_psdtf_normalize(ctx, null, null, 1, 4, 5, 65, _lib.F64, null) == E_ARG
    assert L.assx_psdtf_update_basis(ctx, null, null, null, 1e-12, null, null, 1, 0, 5, 2, _lib.F64, null) == E_ARG
    assert L.assx_psdtf_update_activation(ctx, null, null, null, 1e-12, null, 1, 4, 5, 2, _lib.F32, null) == E_UNSUPPORTED


def test_target_symmetric_to_rounding_is_symmetrised_on_upload():
    fx = load("psdtf_m4_t10_k2")
    X = fx["X"]
    ulp = X.copy()
    ulp[0, 1] = np.nextafter(ulp[0, 1], np.inf)  # what a product in another order leaves
    ulp[3, 2] = np.nextafter(ulp[3, 2], -np.inf)
    assert not np.array_equal(ulp, ulp.transpose(1, 0, 2))
    runs = []
    for target in (ulp, (ulp + ulp.transpose(1, 0, 2)) / 2):
        np.random.seed(5)
        model = cls()(n_basis=2)
        runs.append(model(target, iteration=3) + (list(model.loss),))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    far = X.copy()
    far[0, 1] *= 1 + 1e-9
    with pytest.raises(ValueError, match="symmetric"):
        cls()(n_basis=2)(far, iteration=1)


def test_reconstruct_reports_the_status_word():
    fx = load("psdtf_m4_t10_k2")
    np.random.seed(2)
    model = cls()(n_basis=2)
    model(fx["X"], iteration=1)
    model._status.fill_(1)  # as a kernel leaves it after a matrix that is not positive definite
    with pytest.raises(np.linalg.LinAlgError):
        model.reconstruct()
    assert model.reconstruct().shape == fx["X"].shape  # raised once, the word is cleared


def test_engine_refuses_arrays_of_the_wrong_shape(eng):
    fx = load("psdtf_m4_t10_k2")
    X, V, H, eps, _ = problem(fx, 0)
    d = Device(eng, X, V, H)
    (short,) = up(eng, H[None, :, :-1])
    with pytest.raises(ValueError):
        eng.psdtf_update(d.X, d.V, short, d.ws, eps=eps)
    with pytest.raises(ValueError):
        eng.psdtf_update(d.X, d.V, d.H, d.ws[:16], eps=eps)
    with pytest.raises(ValueError):
        eng.psdtf_update(d.X[:, :-1], d.V, d.H, d.ws, eps=eps)


def test_all_zero_frame_raises_linalgerror():
    fx = load("psdtf_m4_t10_k2")
    X = fx["X"].copy()
    X[:, :, 3] = 0
    np.random.seed(1)
    model = cls()(n_basis=2)
    with pytest.raises(np.linalg.LinAlgError):
        model(X, iteration=3)  # the frame's activation becomes 0, the next update inverts Y = 0: the status word, no fault
    # the kernels finished: the same object runs a sound target afterwards
    del model.basis, model.activation
    V, H = model(fx["X"], iteration=2)
    assert np.isfinite(V).all() and np.isfinite(H).all()
