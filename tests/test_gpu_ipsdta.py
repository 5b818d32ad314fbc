"""GaussIPSDTA on the GPU: every entry point against the reference's recorded states (tests/golden/ipsdta) and the NumPy
restatement (tests/ipsdta_np.py), the class against the reference's recorded front-door runs, and the determinism of the
HIP path.

Metrics (tests/ipsdta_np.py): W per bin max|a - b| / max|b|, U per (source, basis) max|a - b| / max|b| over all its blocks,
H entry-wise, loss |a - b| / (|b| + N n_bins n_frames), out per source max|a - b| / max|b|; tolerances come from
tests/golden/ipsdta/tolerances.json (tools/ipsdta_tolerance_probe.py --model gauss).  Every figure is printed before it is
asserted (pytest -s shows them)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ipsdta_np as ip  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [os.path.basename(f)[:-4] for f in ip.fixture_files()]
CLASS_NAMES = ["ipsdta_m2_f9_t64_k2_b4_s2", "ipsdta_m2_f16_t128_k2_b2_s2", "ipsdta_m3_f11_t96_k3_b3_s2",
               "ipsdta_m2_f6_t64_k2_b6_s2", "ipsdta_m2_f12_t64_k2_b3_s10", "ipsdta_m2_f12_t64_k2_b3_s2_nonorm",
               "ipsdta_m8_f6_t160_k2_b3_s2"]
TOL = ip.tolerances()


def load(name):
    return np.load(os.path.join(ip.GOLDEN, name + ".npz"))


def cls():
    from audio_source_separation_amd.bss.ipsdta import GaussIPSDTA
    return GaussIPSDTA


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(dtype="float64")


class Device:
    """One problem on the device: X (M,F,T), W (F,M,M), the packed basis (N,K,P), H (N,K,T)."""

    def __init__(self, eng, X, W, basis, H, n_blocks):
        from audio_source_separation_amd._device import to_device, torch
        self.eng, self.nblk, self.F = eng, int(n_blocks), X.shape[1]
        M, F, T = X.shape
        self.X = to_device(np.ascontiguousarray(X), torch.complex128, eng.dev)
        self.W = to_device(np.ascontiguousarray(W), torch.complex128, eng.dev)
        self.U = to_device(ip.pack(basis), torch.complex128, eng.dev)
        self.H = to_device(np.ascontiguousarray(H), torch.float64, eng.dev)
        self.ws = eng.ipsdta_workspace(M, F, T, H.shape[1], n_blocks)
        self.status = eng.new_status(1)

    def args(self):
        return self.X, self.W, self.U, self.H, self.ws, self.nblk

    def model(self, ok=True):
        from audio_source_separation_amd._device import to_numpy
        if ok:
            assert int(self.status.item()) == 0
        return to_numpy(self.W), ip.unpack(to_numpy(self.U), self.F, self.nblk), to_numpy(self.H)

    def raw(self):
        from audio_source_separation_amd._device import to_numpy
        return to_numpy(self.W), to_numpy(self.U), to_numpy(self.H)


def device(eng, fx, tag):
    W, U, H = ip.state(fx, tag)
    return Device(eng, fx["X"], W, U, H, int(fx["n_blocks"]))


def check(figures, tol, what):
    print(what, {k: "%.2e (tol %.2e)" % (v, tol[k]) for k, v in figures.items()})
    for metric, err in figures.items():
        assert err <= tol[metric], (what, metric, err, tol[metric])


def model_figures(got, want):
    return {"W": ip.w_metric(got[0], want[0]), "U": ip.basis_metric(got[1], want[1]), "H": ip.h_metric(got[2], want[2])}


# ---- entry points against the fixtures -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_iteration_from_every_recorded_state(eng, name):
    fx = load(name)
    M, F, T, K, nblk, sp = ip.dims(fx)
    eps, norm = float(fx["eps"]), bool(fx["normalize"])
    from audio_source_separation_amd._device import torch
    for it in ip.START_ITERS:
        d = device(eng, fx, it)
        loss = eng.empty((1,), dtype=torch.float64)
        eng.ipsdta_iterate(1, sp, *d.args(), eps=eps, normalize=norm, loss=loss, status=d.status)
        figures = model_figures(d.model(), ip.state(fx, it + 1))
        figures["loss"] = ip.loss_metric(loss.item(), fx["loss"][it + 1], M, F, T)
        check(figures, TOL["one_iteration"], "%s %d->%d" % (name, it, it + 1))


@pytest.mark.parametrize("name", NAMES)
def test_source_stage_and_single_sweeps_against_recorded_states(eng, name):
    """The recorded intermediate states of iteration 1: a wrong Gauss-Seidel order inside a block shows here entry by entry."""
    fx = load(name)
    M, F, T, K, nblk, sp = ip.dims(fx)
    eps, norm = float(fx["eps"]), bool(fx["normalize"])
    tol = TOL["one_stage"]
    d = device(eng, fx, 0)
    eng.ipsdta_update_source(*d.args(), eps=eps, normalize=norm, status=d.status)
    W, U, H = d.model()
    want = ip.state(fx, "src1")
    assert np.array_equal(W, want[0])
    check({"U": ip.basis_metric(U, want[1]), "H": ip.h_metric(H, want[2])}, tol, name + " source stage")
    tags = ["src1"] + ["sw1_%d" % (s + 1) for s in range(sp)]
    for a, b in zip(tags[:-1], tags[1:]):
        d = device(eng, fx, a)
        before = d.raw()
        eng.ipsdta_update_spatial(*d.args(), n_sweeps=1, eps=eps, status=d.status)
        after = d.raw()
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        check({"W": ip.w_metric(after[0], fx["W_%s" % b])}, tol, "%s %s->%s" % (name, a, b))
    # all sweeps in one call from the state after the source update
    d = device(eng, fx, "src1")
    eng.ipsdta_update_spatial(*d.args(), n_sweeps=sp, eps=eps, status=d.status)
    check({"W": ip.w_metric(d.raw()[0], fx["W_%s" % tags[-1]])}, TOL["one_iteration"], name + " all sweeps")


@pytest.mark.parametrize("name", NAMES)
def test_loss_of_every_recorded_state(eng, name):
    fx = load(name)
    M, F, T, K, nblk, sp = ip.dims(fx)
    for it in (0,) + ip.SNAP_ITERS:
        d = device(eng, fx, it)
        loss = d.eng.ipsdta_loss(*d.args(), eps=float(fx["eps"]), status=d.status)
        assert loss.shape == (1,) and int(d.status.item()) == 0
        check({"loss": ip.loss_metric(loss.item(), fx["loss"][it], M, F, T)}, TOL["one_stage"], "%s loss %d" % (name, it))


@pytest.mark.parametrize("name", NAMES)
def test_stages_against_restatement(eng, name):
    """update_basis, update_activation and normalize alone (the reference records no state between them)."""
    fx = load(name)
    M, F, T, K, nblk, sp = ip.dims(fx)
    eps, X = float(fx["eps"]), fx["X"]
    tol = TOL["one_stage"]
    for it in (0, 4):
        W, U, H = ip.state(fx, it)
        d = Device(eng, X, W, U, H, nblk)
        eng.ipsdta_update_basis(*d.args(), eps=eps, status=d.status)
        Wn, Un, Hn = d.model()
        assert np.array_equal(Wn, W) and np.array_equal(Hn, H)
        for p in ip.to_parts(Un):
            assert np.array_equal(p, ip.ct(p))  # psd leaves exactly Hermitian blocks
        e_basis = ip.basis_metric(Un, ip.update_basis(X, W, U, H, eps, nblk))
        eng.ipsdta_update_activation(*d.args(), eps=eps, status=d.status)
        Wa, Ua, Ha = d.model()
        assert np.array_equal(ip.pack(Ua), ip.pack(Un))
        e_act = ip.h_metric(Ha, ip.update_activation(X, W, Un, H, eps, nblk))  # from the device's own basis: the stage alone
        eng.ipsdta_normalize(d.U, d.H, F, nblk)
        Wm, Um, Hm = d.model()
        Uq, Hq = ip.normalize(Ua, Ha, F, nblk)
        # two orders of summing the n_bins non-negative diagonal entries differ by at most (n_bins - 1) 2^-52 of the trace,
        # the division or product adds a rounding on either side
        tol_norm = (F + 1) * 2.0 ** -52
        figures = {"basis": (e_basis, tol["U"]), "activation": (e_act, tol["H"]),
                   "normalize U": (ip.basis_metric(Um, Uq), tol_norm), "normalize H": (ip.h_metric(Hm, Hq), tol_norm)}
        print(name, it, {k: "%.2e (tol %.2e)" % v for k, v in figures.items()})
        for k, (err, t) in figures.items():
            assert err <= t, (k, err, t)


# ---- the loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_iterate_against_recorded_run_and_single_calls(eng, name):
    from audio_source_separation_amd._device import to_numpy, torch
    fx = load(name)
    M, F, T, K, nblk, sp = ip.dims(fx)
    eps, norm = float(fx["eps"]), bool(fx["normalize"])
    d = device(eng, fx, 0)
    loss = eng.empty((ip.N_ITER,), dtype=torch.float64)
    eng.ipsdta_iterate(ip.N_ITER, sp, *d.args(), eps=eps, normalize=norm, loss=loss, status=d.status)
    loss = to_numpy(loss)
    figures = model_figures(d.model(), ip.state(fx, ip.N_ITER))
    figures["loss"] = ip.loss_metric(loss, fx["loss"][1:], M, F, T)
    check(figures, TOL["whole_run"], name + " 10 iterations")

    # the single calls, bit for bit
    s = device(eng, fx, 0)
    single = []
    for _ in range(ip.N_ITER):
        eng.ipsdta_update_basis(*s.args(), eps=eps, status=s.status)
        eng.ipsdta_update_activation(*s.args(), eps=eps, status=s.status)
        if norm:
            eng.ipsdta_normalize(s.U, s.H, F, nblk)
        for _ in range(sp):
            eng.ipsdta_update_spatial(*s.args(), n_sweeps=1, eps=eps, status=s.status)
        single.append(eng.ipsdta_loss(*s.args(), eps=eps, status=s.status).item())
    assert all(np.array_equal(a, b) for a, b in zip(d.raw(), s.raw()))
    assert np.array_equal(loss, np.array(single))

    # a second run, and one without the loss, bit for bit
    r = device(eng, fx, 0)
    eng.ipsdta_iterate(ip.N_ITER, sp, *r.args(), eps=eps, normalize=norm, loss=None, status=r.status)
    assert all(np.array_equal(a, b) for a, b in zip(d.raw(), r.raw()))


# ---- sizes the fixtures do not cover -----------------------------------------------------------------------------------
# (n_channels, n_bins, n_frames, n_basis, n_blocks): every block size 1..8, with and without remains, M in {2, 3, 4, 5, 8},
# frames in {1, 63, 64, 65, 257}, K in {1, 10, 64}
SIZE_CASES = (
    (2, 3, 63, 1, 3), (2, 7, 64, 10, 4), (3, 8, 65, 1, 4), (2, 11, 64, 10, 4), (4, 9, 63, 1, 3), (2, 9, 65, 10, 2),
    (5, 8, 64, 1, 2), (2, 11, 63, 10, 2), (2, 10, 257, 1, 2), (3, 13, 65, 10, 2), (2, 12, 64, 64, 2), (2, 15, 63, 1, 2),
    (2, 14, 65, 10, 2), (8, 5, 257, 1, 2), (2, 16, 64, 1, 2), (4, 6, 64, 64, 3),
    (2, 9, 1, 10, 4), (3, 16, 1, 1, 2),
)


@pytest.mark.parametrize("case", SIZE_CASES, ids=lambda c: "m%d_f%d_t%d_k%d_b%d" % c)
def test_size_sweep_against_restatement(eng, case):
    """One iteration with two sweeps against the restatement.  The tolerance is worked out on the CPU for the very problem:
    16 x the larger of (restatement on the kernels' algorithms against restatement on numpy.linalg) and (restatement after a
    one-ulp move of everything it reads against itself), at least 16 x 2^-52 -- the recipe of the tolerance probe, with the
    restatement standing in for the reference.  With fewer frames than channels Q has rank n_frames and is inverted
    through its eps shift alone (condition above 1e12), so a single frame checks the source update and the loss only."""
    from audio_source_separation_amd._device import torch
    M, F, T, K, nblk = case
    eps, sp = 1e-12, 2 if T >= M else 0
    X, W, U, H = ip.synthetic(M, F, T, K, nblk, 7000 + sum(case))

    def run(X, W, U, H, la):
        Un, Hn = ip.update_source(X, W, U, H, eps, nblk, True, la)
        Wn = ip.update_spatial(X, W, Un, Hn, eps, nblk, sp, la) if sp else W
        return (Wn, Un, Hn), ip.loss(X, Wn, Un, Hn, eps, nblk, la)

    def figures(got, loss, want, want_loss):
        f = model_figures(got, want)
        f["loss"] = ip.loss_metric(loss, want_loss, M, F, T)
        return f

    want, want_loss = run(X, W, U, H, ip.LAPACK)
    rng = np.random.default_rng(1)
    a = figures(*run(X, W, U, H, ip.KERNEL), want, want_loss)
    b = figures(*run(ip.one_ulp(X, rng), ip.one_ulp(W, rng), ip.herm_ulp(U, rng), ip.one_ulp(H, rng), ip.LAPACK), want, want_loss)
    tol = {k: 16 * max(a[k], b[k], 2.0 ** -52) for k in a}

    d = Device(eng, X, W, U, H, nblk)
    loss = eng.empty((1,), dtype=torch.float64)
    eng.ipsdta_iterate(1, sp, *d.args(), eps=eps, normalize=True, loss=loss, status=d.status)
    check(figures(d.model(), loss.item(), want, want_loss), tol, "size %s" % (case,))


# ---- to_psd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 9))
def test_to_psd_both_paths(eng, n):
    """Positive definite matrices take the Cholesky shortcut, indefinite and rank-one ones the eigenvalue path.  Against the
    definition on numpy.linalg: the result differs from it by the error of lambda_min alone, which both eigen-solvers keep
    within a few n 2^-52 of the largest |eigenvalue| (8 n 2^-52 of max|A| n here), plus one rounding of the diagonal."""
    from audio_source_separation_amd._device import to_device, to_numpy, torch
    eps = 1e-12
    for kind, A in ip.psd_cases(n, 90 + n):
        dA = to_device(np.ascontiguousarray(A), torch.complex128, eng.dev)
        eng.ipsdta_to_psd(dA, eps=eps)
        got, want = to_numpy(dA), ip.to_psd(A, eps)
        err, tol = ip.mat_metric(got, want), (8 * n * n + 2) * 2.0 ** -52
        print("to_psd n=%d %-10s %.2e (tol %.2e)" % (n, kind, err, tol))
        assert np.array_equal(got, ip.ct(got)) and err <= tol
        if kind == "definite":  # delta is exactly 0: (A + A^H)/2 + eps tr I, to the rounding of the diagonal
            H = (A + ip.ct(A)) / 2
            assert np.max(np.abs(got - (H + eps * np.trace(H, axis1=1, axis2=2).real[:, None, None] * np.eye(n)))) \
                <= 2.0 ** -52 * np.max(np.abs(A))


# ---- the class ---------------------------------------------------------------------------------------------------------
def front_door(fx, **kwargs):
    M, F, T, K, nblk, sp = ip.dims(fx)
    np.random.seed(int(fx["seed"]))
    model = cls()(n_basis=K, normalize=bool(fx["normalize"]), eps=float(fx["eps"]), n_blocks=nblk, **kwargs)
    out = model(fx["X"], iteration=ip.N_ITER, spatial_iteration=sp)
    return model, out


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_class_front_door_against_recorded_run(name):
    fx = load(name)
    M, F, T, K, nblk, sp = ip.dims(fx)
    model, out = front_door(fx)
    assert np.random.rand() == float(fx["rng_next"])  # the draws of the reference, in its order
    want = ip.state(fx, ip.N_ITER)
    assert isinstance(model.basis, tuple) == isinstance(want[1], tuple)
    assert len(model.loss) == ip.N_ITER + 1 and out is model.estimation and out.shape == (M, F, T)
    figures = model_figures((model.demix_filter, model.basis, model.activation), want)
    figures["loss"] = ip.loss_metric(np.array(model.loss), fx["loss"], M, F, T)
    figures["out"] = ip.out_metric(out, fx["out"])
    check(figures, TOL["whole_run"], name + " front door")


def test_class_callbacks_take_the_stepwise_path_to_the_same_bits():
    fx = load(CLASS_NAMES[0])
    calls = []
    fast, out_fast = front_door(fx)
    slow, out_slow = front_door(fx, callbacks=lambda m: calls.append(len(m.loss)))
    assert calls == list(range(1, ip.N_ITER + 2))  # once before the loop, once after every iteration
    assert np.array_equal(out_fast, out_slow) and list(fast.loss) == list(slow.loss)
    assert np.array_equal(fast.demix_filter, slow.demix_filter) and np.array_equal(fast.activation, slow.activation)
    assert all(np.array_equal(a, b) for a, b in zip(fast.basis, slow.basis))


def test_class_warm_start_and_repeated_calls():
    fx = load(CLASS_NAMES[0])
    M, F, T, K, nblk, sp = ip.dims(fx)
    whole, out = front_door(fx)
    np.random.seed(int(fx["seed"]))
    model = cls()(n_basis=K, normalize=True, eps=float(fx["eps"]), n_blocks=nblk)
    model(fx["X"], iteration=4, spatial_iteration=sp)
    figures = model_figures((model.demix_filter, model.basis, model.activation), ip.state(fx, 4))
    check(figures, TOL["whole_run"], "4 iterations")
    before = np.random.get_state()
    out2 = model(fx["X"], iteration=6)  # warm start: no draw, the keyword of the first call is still an attribute
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2] and model.spatial_iteration == sp
    assert len(model.loss) == 11  # the initial entry only once, the list is never cleared
    # the second call normalises the warm-started model once more (a rounding) and goes on
    figures = model_figures((model.demix_filter, model.basis, model.activation), ip.state(fx, 10))
    figures["out"] = ip.out_metric(out2, fx["out"])
    check(figures, TOL["whole_run"], "4 + 6 iterations")
    # a basis assigned in the reference's layout is taken over
    other = cls()(n_basis=K, eps=float(fx["eps"]), n_blocks=nblk)
    other.demix_filter, other.basis, other.activation = ip.state(fx, 4)
    out3 = other(fx["X"], iteration=6, spatial_iteration=sp)
    check({"out": ip.out_metric(out3, fx["out"])}, TOL["whole_run"], "assigned state + 6 iterations")


def test_class_without_loss():
    fx = load(CLASS_NAMES[0])
    model, out = front_door(fx, recordable_loss=False)
    assert model.loss is None
    check({"out": ip.out_metric(out, fx["out"])}, TOL["whole_run"], "recordable_loss=False")


def test_class_stepwise_methods():
    fx = load(CLASS_NAMES[0])
    M, F, T, K, nblk, sp = ip.dims(fx)
    np.random.seed(int(fx["seed"]))
    model = cls()(n_basis=K, eps=float(fx["eps"]), n_blocks=nblk)
    model.input = fx["X"]
    model._reset(spatial_iteration=sp)
    check(model_figures((model.demix_filter, model.basis, model.activation), ip.state(fx, 0)), TOL["one_stage"], "reset")
    assert abs(model.compute_negative_loglikelihood() - fx["loss"][0]) <= TOL["one_stage"]["loss"] * (abs(fx["loss"][0]) + M * F * T)
    model.update_once()
    check(model_figures((model.demix_filter, model.basis, model.activation), ip.state(fx, 1)), TOL["one_iteration"], "update_once")
    Y = model.separate(fx["X"], model.demix_filter)
    assert np.max(np.abs(Y - ip.separate(fx["X"], model.demix_filter))) <= 8 * M * 2.0 ** -52 * np.max(np.abs(Y))


def test_class_zero_activation_raises_linalgerror():
    fx = load(CLASS_NAMES[0])
    M, F, T, K, nblk, sp = ip.dims(fx)
    model = cls()(n_basis=K, n_blocks=nblk)
    H = fx["H_0"].copy()
    H[1] = 0.0  # R of source 1 is the zero matrix: nothing to invert
    model.activation = H
    with pytest.raises(np.linalg.LinAlgError):
        model(fx["X"], iteration=1, spatial_iteration=sp)


def test_class_refusals():
    G = cls()
    X = load(CLASS_NAMES[0])["X"]  # (2, 9, 64)
    with pytest.raises(NotImplementedError, match="Ikeshita"):
        G(author='Ikeshita')
    with pytest.raises(ValueError):
        G(author='nobody')
    with pytest.raises(ValueError):
        G(n_neighbors=2)  # not a keyword of the reference
    with pytest.raises(ValueError, match="blocks of at most 8"):
        G(n_blocks=1)(X, iteration=1)  # one block of 9 bins
    with pytest.raises(ValueError, match="n_blocks"):
        G(n_blocks=10)(X, iteration=1)  # n_blocks > n_bins
    with pytest.raises(ValueError, match="n_blocks"):
        G()(X, iteration=1)  # the default of 1024 blocks on 9 bins
    with pytest.raises(ValueError, match="n_channels"):
        G(n_blocks=4)(X[:1], iteration=1)
    with pytest.raises(ValueError, match="n_channels"):
        G(n_blocks=4)(np.tile(X, (5, 1, 1))[:9], iteration=1)
    with pytest.raises(ValueError, match="n_basis"):
        G(n_basis=65, n_blocks=4)(X, iteration=1)
    with pytest.raises(ValueError, match="float64"):
        G(dtype='float32')
