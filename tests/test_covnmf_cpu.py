"""Covariance-domain MultichannelISNMF without a GPU: the NumPy restatement (tests/covnmf_np.py) against the
reference-recorded fixtures of tests/golden/covnmf, planted faults that the fixtures must catch, the C-ABI's symbol list,
its workspace query and NULL-context refusals, and the refusals of the class that need no device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import covnmf_np as cv  # noqa: E402
from mnmf_np import riccati  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "covnmf")
FILES = cv.fixtures(GOLDEN)
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ENTRY_POINTS = ("workspace_bytes", "update_basis", "update_activation", "update_spatial", "reconstruct", "loss",
                "iterate")
# the restatement against the reference, states relative to their largest entry and every loss relatively: the maker's
# own figures are at most 3.1e-13 up to iteration 5, 1.2e-11 at iteration 20 and 2.0e-12 for the loss
TOL = 1e-10


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def distances(g, step=cv.update_once):
    """(largest state distance over the recorded iterations, largest relative loss distance) of a run of `step`."""
    states, losses = cv.run(g["X"], g["T0"], g["V0"], cv.N_ITER, bool(g["normalize"]), float(g["eps"]), step=step)
    d = max(cv.rel(a, g["%s_%d" % (n, it)]) for it in cv.SNAP_ITERS for n, a in zip("HTV", states[it]))
    return d, float(np.max(np.abs(np.array(losses) - g["loss"]) / np.abs(g["loss"])))


def test_fixtures_are_complete():
    shapes = set()
    for name in NAMES:
        g = load(name)
        F, T, M, _ = g["X"].shape
        K = int(g["n_basis"])
        shapes.add((M, F, T, K, int(g["smooth"]), bool(g["normalize"])))
        assert g["T0"].shape == (F, K) and g["V0"].shape == (K, T) and g["loss"].shape == (cv.N_ITER,)
        assert int(g["smooth"]) >= M and float(g["eps"]) == cv.EPS
        for it in cv.SNAP_ITERS:
            assert g["H_%d" % it].shape == (F, K, M, M) and g["H_%d" % it].dtype == np.complex128
            assert g["T_%d" % it].shape == (F, K) and g["V_%d" % it].shape == (K, T)
        assert np.array_equal(g["X"], g["X"].conj().swapaxes(-1, -2))
        assert np.linalg.eigvalsh(g["X"]).min() > 0  # positive definite: the loss takes its log-determinant
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < (1 << 20)
    wanted = {(2, 5, 40, 3, 3, True), (3, 4, 33, 2, 3, True), (4, 6, 64, 4, 5, True), (5, 3, 48, 1, 6, True),
              (6, 2, 40, 3, 7, True), (7, 2, 40, 2, 8, True), (8, 3, 70, 2, 8, True), (8, 3, 70, 2, 9, False),
              (2, 3, 20, 64, 2, True), (2, 4, 257, 2, 2, True)}
    assert wanted <= shapes


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    """State by state (iterations 1, 2, 5, 20) and loss by loss."""
    g = load(name)
    states, losses = cv.run(g["X"], g["T0"], g["V0"], cv.N_ITER, bool(g["normalize"]), float(g["eps"]))
    for it in cv.SNAP_ITERS:
        for n, a in zip("HTV", states[it]):
            d = cv.rel(a, g["%s_%d" % (n, it)])
            assert d < TOL, (n, it, d)
    dl = np.abs(np.array(losses) - g["loss"]) / np.abs(g["loss"])
    assert dl.max() < TOL, dl


def test_start_state_is_the_draws_after_the_reset():
    for name in NAMES:
        g = load(name)
        np.random.seed(int(g["seed"]))
        F, T, M, _ = g["X"].shape
        K = int(g["n_basis"])
        assert np.array_equal(np.random.rand(F, K), g["T0"]) and np.array_equal(np.random.rand(K, T), g["V0"])
        assert np.random.rand() == float(g["rng_next"])
        assert np.array_equal(cv.target(M, F, T, int(g["smooth"]), int(g["seed"])), g["X"])


# ------------------------------------------------------------------------------------------------ planted faults
def _spatial(X, Tb, V, H, normalize, eps, with_tb, eps_first):
    M = X.shape[-1]
    P, Q, _, _ = cv._eval(X, Tb, V, H, eps)
    W = Tb[:, :, None] * V[None] if with_tb else np.broadcast_to(V[None], Tb.shape + V.shape[1:])
    Hn = riccati(np.einsum("fkt,ftij->fkij", W, P), H @ np.einsum("fkt,ftij->fkij", W, Q) @ H)
    if eps_first is True:
        Hn = Hn + eps * np.eye(M)
    if normalize:
        Hn = Hn / np.trace(Hn, axis1=2, axis2=3)[..., None, None]
    if eps_first is False:
        Hn = Hn + eps * np.eye(M)
    return Hn


def fault_basis_factor_and_no_eps(X, Tb, V, H, normalize, eps):
    """Tb[f,k] inside both spatial sums (it cancels in the Riccati equation) and `+ eps I` forgotten."""
    Tb = cv.update_basis(X, Tb, V, H, eps)
    V = cv.update_activation(X, Tb, V, H, eps)
    return Tb, V, _spatial(X, Tb, V, H, normalize, eps, with_tb=True, eps_first=None)


def fault_same_evaluation(X, Tb, V, H, normalize, eps):
    """basis and activation from one evaluation: the activation update sees the old basis."""
    Tn = cv.update_basis(X, Tb, V, H, eps)
    V = cv.update_activation(X, Tb, V, H, eps)
    return Tn, V, cv.update_spatial(X, Tn, V, H, normalize, eps)


def fault_normalise_before_eps(X, Tb, V, H, normalize, eps):
    """H / tr H + eps I instead of (H + eps I) / tr(H + eps I)."""
    Tb = cv.update_basis(X, Tb, V, H, eps)
    V = cv.update_activation(X, Tb, V, H, eps)
    return Tb, V, _spatial(X, Tb, V, H, normalize, eps, with_tb=False, eps_first=False)


def test_spatial_helper_of_the_faults_is_the_restatement_when_no_fault_is_planted():
    g = load(NAMES[0])
    X, Tb, V, H = g["X"], g["T_1"], g["V_1"], g["H_1"]
    for normalize in (True, False):
        assert np.array_equal(_spatial(X, Tb, V, H, normalize, cv.EPS, with_tb=False, eps_first=True),
                              cv.update_spatial(X, Tb, V, H, normalize, cv.EPS))


@pytest.mark.parametrize("fault", (fault_basis_factor_and_no_eps, fault_same_evaluation, fault_normalise_before_eps),
                         ids=lambda f: f.__name__)
def test_fixtures_catch_a_planted_fault(fault):
    """A fault is caught when some fixture sees it beyond the bound that the restatement itself is held to.  Measured:
    the two faults that differ by an eps = 1e-12 shift only move the state by 1e-12 at iteration 1 (a hundred times the
    restatement's own distance, still below the bound) and grow with the iterations: 9.9e-9 (basis factor, no eps) and
    3.3e-10 (normalisation first) on covnmf_m2_f3_t20_k64_s2 at iteration 20, 2.6e-9 and 1.5e-10 on covnmf_m8_f3_t70_k2_s8;
    the shared evaluation moves every fixture by 0.2 or more from iteration 1 on."""
    caught = []
    for name in NAMES:
        d, dl = distances(load(name), step=fault)
        print("%-36s %-32s states %.1e loss %.1e" % (fault.__name__, name, d, dl))
        if max(d, dl) >= TOL:
            caught.append(name)
    assert caught, "no fixture sees %s" % fault.__name__


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "assx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_covnmf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted("assx_covnmf_" + n for n in ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_covnmf_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    build = open(os.path.join(ROOT, "audio_source_separation_amd", "csrc", "build.sh")).read()
    assert build.count("assx_covnmf") == 2  # the SRCS list and the link line


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_covnmf_workspace_bytes
    base = q(4, 17, 65, 3, _lib.F64)
    assert base > 0
    assert q(5, 17, 65, 3, _lib.F64) > base and q(4, 18, 65, 3, _lib.F64) > base
    assert q(4, 17, 66, 3, _lib.F64) > base and q(4, 17, 65, 4, _lib.F64) > base
    for M, F, T, K, dt in ((1, 17, 65, 3, _lib.F64), (9, 17, 65, 3, _lib.F64), (4, 0, 65, 3, _lib.F64),
                           (4, 17, 0, 3, _lib.F64), (4, 17, 65, 0, _lib.F64), (4, 17, 65, 65, _lib.F64),
                           (4, 17, 65, 3, _lib.F32), (4, -1, 65, 3, _lib.F64), (4, 17, 65, 3, 7)):
        assert q(M, F, T, K, dt) == 0, (M, F, T, K, dt)
    assert q(2, 1, 1, 1, _lib.F64) > 0 and q(8, 1, 1, 64, _lib.F64) > 0
    # the target stays below 4 GiB (M M F T < 2^28); beyond that, and where a product would overflow, the answer is 0
    assert q(8, 2048, 2047, 64, _lib.F64) > 2 ** 32  # sizes in 64-bit arithmetic
    assert q(8, 2048, 2048, 64, _lib.F64) == 0
    assert q(2, 2 ** 31 - 1, 2 ** 31 - 1, 64, _lib.F64) == 0 and q(2, 2 ** 31 - 1, 1, 1, _lib.F64) == 0
    assert q(8, 2 ** 16, 2 ** 16, 64, _lib.F64) == 0


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    sizes = (4, 5, 6, 2, _lib.F64, null)
    assert L.assx_covnmf_update_basis(null, null, null, null, null, 1e-12, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_update_activation(null, null, null, null, null, 1e-12, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_update_spatial(null, null, null, null, null, 1, 1e-12, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_reconstruct(null, null, null, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_loss(null, null, null, null, null, 1e-12, null, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_iterate(null, 1, 1, null, null, null, null, 1e-12, null, null, null, *sizes) == E_NULL
    assert L.assx_covnmf_iterate(null, -1, 2, null, null, null, null, 1e-12, null, null, null, 9, 0, 0, 99, 7, null) == E_NULL


# ------------------------------------------------------------------------------------------------ the class
def test_class_refusals_touch_neither_a_device_nor_the_rng():
    from audio_source_separation_amd.algorithm.nmf import MultichannelISNMF, MultichannelNMFbase, EPS
    X = np.tile(np.eye(3, dtype=np.complex128), (5, 6, 1, 1))
    for dtype in ("float32", np.float32, "complex64"):
        with pytest.raises(ValueError, match="float64"):
            MultichannelISNMF(3, dtype=dtype)
    new = MultichannelISNMF
    refused = [(new(0), X, "n_basis"), (new(65), X, "n_basis"), (new(2.5), X, "n_basis"),
               (new(3), X.real, "complex"), (new(3), X[0], "dims"), (new(3), X[None], "dims"),
               (new(3), np.ones((5, 6, 3, 2), dtype=np.complex128), "square"),
               (new(3), np.ones((5, 6, 1, 1), dtype=np.complex128), "n_channels"),
               (new(3), np.ones((5, 6, 9, 9), dtype=np.complex128), "n_channels"),
               (new(3), np.ones((0, 6, 3, 3), dtype=np.complex128), "empty"),
               (new(3), np.ones((5, 0, 3, 3), dtype=np.complex128), "empty")]
    for model, target, what in refused:
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match=what):
            model(target, iteration=1)
        assert model._engine is None and np.array_equal(np.random.get_state()[1], state)
        assert model.loss == [] and not any(hasattr(model, a) for a in ("spatial", "basis", "activation"))
    warm = [("spatial", np.ones((5, 3, 3, 2), dtype=np.complex128), "shape"), ("basis", np.ones((5, 2)), "shape"),
            ("basis", np.ones((5, 3), dtype=np.complex128), "real"), ("activation", np.ones((3, 7)), "shape")]
    for attr, value, what in warm:
        model = new(3)
        with pytest.raises(ValueError, match=what):
            model(X, iteration=1, **{attr: value})
        assert model._engine is None
    model = new()
    assert (model.n_basis, model.normalize, model.eps, model.loss, EPS) == (10, True, 1e-12, [], 1e-12)
    assert isinstance(model.loss, list) and not hasattr(model, "criterion")
    assert new(4, False, 1e-9).normalize is False and new(4, False, 1e-9).eps == 1e-9
    assert MultichannelNMFbase().n_basis == 2 and issubclass(new, MultichannelNMFbase)
    with pytest.raises(NotImplementedError):
        MultichannelNMFbase().update_once()


def test_generator_reproduces_the_fixtures():
    if not os.path.isdir(os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")):
        pytest.skip("the reference tree is not present")
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_covnmf.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified 10 files, 0 problems" in run.stdout, run.stdout + run.stderr
