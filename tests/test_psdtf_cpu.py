"""LDPSDTF without a GPU: the NumPy restatement (tests/psdtf_np.py) against the reference's recorded states
(tests/golden/psdtf/*.npz) one update at a time and over the whole run, on numpy.linalg and on the models of the kernels'
own algorithms; to_psd against its definition; the Jacobi and Cholesky models against numpy.linalg; the C-ABI names, the
workspace query and the host-side refusals."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import psdtf_np as pt  # noqa: E402

FILES = pt.fixture_files()
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ENTRY_POINTS = ("workspace_bytes", "to_psd", "update_basis", "update_activation", "normalize", "update", "loss",
                "reconstruct", "iterate")
SIZES = (1, 2, 5, 16, 33, 64)
LAS = (pt.LAPACK, pt.KERNEL)


def load(name):
    return np.load(os.path.join(pt.GOLDEN, name + ".npz"))


def reference_src():
    src = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")  # the default of tests/golden/make_golden.py
    if not os.path.isdir(os.path.join(src, "algorithm")):
        pytest.skip("the reference tree is not on this machine")


def test_fixtures_and_tolerances_are_complete():
    tol = pt.tolerances()
    assert len(NAMES) == 10
    assert tol["factor"] == 16
    assert set(tol["one_update"]) == set(pt.METRICS) and set(tol["whole_run"]) == set(pt.METRICS)
    assert 16 * 2.0 ** -52 <= min(tol["one_update"].values()) and max(tol["one_update"].values()) <= 1e-10
    assert min(tol["whole_run"].values()) >= 16 * 2.0 ** -52
    shapes = set()
    for f in FILES:
        assert os.path.getsize(f) < 1 << 20, f  # the repository's cap per committed file, as for the MNMF fixtures
        fx = np.load(f)
        M, M2, T = fx["X"].shape
        K = fx["H0"].shape[0]
        shapes.add((M, T, K, bool(fx["normalize"])))
        assert M == M2 and np.array_equal(fx["X"], fx["X"].transpose(1, 0, 2))
        assert fx["V0"].shape == (M, M, K) and fx["H0"].shape == (K, T)
        assert fx["draw_V"].shape == (K, M) and fx["draw_H"].shape == (K, T)
        for it in pt.SNAP_ITERS:
            assert fx["basis_%d" % it].shape == (M, M, K) and fx["activation_%d" % it].shape == (K, T), (f, it)
        assert fx["loss"].shape == (20,) and fx["rng_next"].shape == () and fx["seed"].shape == () and fx["eps"] > 0
        assert all(np.isfinite(fx[k]).all() for k in fx.files if k != "versions")
        assert np.all(np.diff(fx["loss"]) <= 1e-9 * (np.abs(fx["loss"][:-1]) + M * T))  # the MM update does not go up
    assert shapes == {(4, 10, 2, True), (1, 9, 2, True), (5, 1, 2, True), (7, 70, 1, True), (16, 33, 3, True),
                      (9, 9, 64, True), (64, 5, 3, True), (3, 257, 4, True), (33, 20, 2, True), (8, 20, 3, False)}


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_one_update_at_a_time(name, la):
    fx = load(name)
    tol = pt.tolerances()["one_update"]
    X, eps, norm = pt.frames_first(fx["X"]), float(fx["eps"]), bool(fx["normalize"])
    T, M, _ = X.shape
    for it in pt.START_ITERS:
        V, H = pt.state(fx, it)
        V = pt.kmm(V)
        kept = (V.copy(), H.copy(), X.copy())
        Vn, Hn = pt.update(X, V, H, eps, norm, la)
        assert all(np.array_equal(a, b) for a, b in zip((V, H, X), kept))
        Vw, Hw = pt.state(fx, it + 1)
        assert pt.v_metric(Vn, pt.kmm(Vw)) <= tol["V"], it
        assert pt.h_metric(Hn, Hw) <= tol["H"], it
        assert pt.loss_metric(pt.loss(X, Vn, Hn, eps, la), fx["loss"][it], M, T) <= tol["loss"], it
        assert pt.loss_metric(pt.loss(X, pt.kmm(Vw), Hw, eps, la), fx["loss"][it], M, T) <= tol["loss"], it


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_over_the_whole_run(name, la):
    fx = load(name)
    tol = pt.tolerances()["whole_run"]
    X, eps, norm = pt.frames_first(fx["X"]), float(fx["eps"]), bool(fx["normalize"])
    T, M, _ = X.shape
    V, H = pt.state(fx, 0)
    states, losses = pt.run(X, pt.kmm(V), H, eps, pt.N_ITER, norm, la)
    Vw, Hw = pt.state(fx, 20)
    assert pt.v_metric(states[-1][0], pt.kmm(Vw)) <= tol["V"]
    assert pt.h_metric(states[-1][1], Hw) <= tol["H"]
    assert pt.loss_metric(np.array(losses), fx["loss"], M, T) <= tol["loss"]


def test_start_state_is_the_draws_after_the_reset():
    for name in NAMES:
        fx = load(name)
        # a transposed view of the (K, M, M) array, as in the reference: the memory order decides how NumPy sums the trace
        V = (fx["draw_V"][:, :, None] * np.eye(fx["draw_V"].shape[1])).transpose(1, 2, 0)
        H = fx["draw_H"]
        if fx["normalize"]:
            tr = np.trace(V, axis1=0, axis2=1)
            V, H = V / tr, H * tr[:, None]
        assert np.array_equal(V, fx["V0"]) and np.array_equal(H, fx["H0"]), name


@pytest.mark.parametrize("n", SIZES)
def test_to_psd_against_its_definition(n):
    eps = 1e-3  # large enough for the eps trace term to be visible in every entry of the diagonal
    for kind, A in pt.psd_cases(n, 40 + n):
        A = A + 0.01 / n * np.triu(np.ones((n, n)), 1) if kind != "diagonal" else A  # not symmetric: to_psd symmetrises
        S = (A + np.transpose(A, (0, 2, 1))) / 2
        lam = np.linalg.eigvalsh(S)
        want = (S - np.minimum(lam[:, 0], 0)[:, None, None] * np.eye(n)) \
            + eps * np.trace(S, axis1=1, axis2=2)[:, None, None] * np.eye(n)
        if kind == "indefinite":
            assert (lam[:, 0] < -0.5).all()
        if kind == "definite":
            assert (lam[:, 0] > 0.25).all()
        for la in LAS:
            got = pt.to_psd(A, eps, la)
            assert np.array_equal(got, np.transpose(got, (0, 2, 1)))
            assert pt.mat_metric(got, want) <= 64 * n * 2.0 ** -52, (kind, la.__name__)


@pytest.mark.parametrize("n", SIZES)
def test_jacobi_and_cholesky_models_against_lapack(n):
    for kind, A in pt.psd_cases(n, 70 + n):
        w, U, conv = pt.jacobi_eigh(A)
        assert conv.all()
        scale = np.max(np.abs(np.linalg.eigvalsh(A)), axis=1, keepdims=True)
        # eigenvalues to a few ulps of the spectral radius, vectors orthonormal, the decomposition reproduces A
        assert np.max(np.abs(np.sort(w, axis=1) - np.linalg.eigvalsh(A)) / scale) <= 16 * n * 2.0 ** -52, kind
        assert np.max(np.abs(np.transpose(U, (0, 2, 1)) @ U - np.eye(n))) <= 16 * n * 2.0 ** -52, kind
        assert pt.mat_metric((U * w[:, None, :]) @ np.transpose(U, (0, 2, 1)), A) <= 16 * n * 2.0 ** -52, kind
        if kind == "definite":
            L, ok = pt.chol_lower(A)
            assert ok.all() and pt.mat_metric(L, np.linalg.cholesky(A)) <= 16 * n * 2.0 ** -52
            # cond <= 3: the inverse to n ulps times the condition number
            assert pt.mat_metric(pt.chol_inverse(A), np.linalg.inv(A)) <= 64 * n * 2.0 ** -52
        if kind == "indefinite":
            assert not pt.chol_lower(A)[1].any()
            with pytest.raises(np.linalg.LinAlgError):
                pt.chol_inverse(A)
            assert np.array_equal(pt.KERNEL.min_eig(A) < -0.5, np.ones(len(A), dtype=bool))
    assert np.array_equal(pt.jacobi_pairs(6, 0)[0], [0, 1, 2]) and np.array_equal(pt.jacobi_pairs(6, 0)[1], [5, 4, 3])
    for m in (2, 4, 6, 34, 64):  # every pair exactly once per sweep
        seen = set()
        for r in range(m - 1):
            p, q = pt.jacobi_pairs(m, r)
            assert len(set(p) | set(q)) == m
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2


def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "assx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_psdtf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted("assx_psdtf_" + n for n in ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_psdtf_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    assert _lib.STATUS_NOT_CONVERGED == 4 and "ASSX_STATUS_NOT_CONVERGED = 4" in text


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_psdtf_workspace_bytes
    base = q(1, 16, 33, 3, _lib.F64)
    assert base > 0
    assert q(2, 16, 33, 3, _lib.F64) > base and q(1, 17, 33, 3, _lib.F64) > base
    assert q(1, 16, 34, 3, _lib.F64) > base and q(1, 16, 33, 4, _lib.F64) > base
    for B, M, T, K, dt in ((1, 16, 33, 0, _lib.F64), (1, 16, 33, 65, _lib.F64), (1, 0, 33, 3, _lib.F64),
                           (1, 65, 33, 3, _lib.F64), (1, 16, 33, 3, _lib.F32), (0, 16, 33, 3, _lib.F64),
                           (1, 16, 0, 3, _lib.F64)):
        assert q(B, M, T, K, dt) == 0, (B, M, T, K, dt)
    assert q(1, 64, 1, 64, _lib.F64) > 0 and q(1, 1, 1, 1, _lib.F64) > 0
    assert q(64, 64, 100000, 64, _lib.F64) > 2 ** 32  # sizes in 64-bit arithmetic


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    assert L.assx_psdtf_to_psd(null, null, 1, 4, 1e-12, null) == E_NULL
    assert L.assx_psdtf_update(null, null, null, null, 1e-12, 1, null, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL
    assert L.assx_psdtf_update_basis(null, null, null, null, 1e-12, null, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL
    assert L.assx_psdtf_update_activation(null, null, null, null, 1e-12, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL
    assert L.assx_psdtf_normalize(null, null, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL
    assert L.assx_psdtf_loss(null, null, null, null, 1e-12, null, null, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL
    assert L.assx_psdtf_reconstruct(null, null, null, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL
    assert L.assx_psdtf_iterate(null, 1, null, null, null, 1e-12, 1, null, null, null, 1, 4, 5, 2, _lib.F64, null) == E_NULL


def test_class_refusals_touch_neither_a_device_nor_the_rng():
    from audio_source_separation_amd.algorithm.psdtf import LDPSDTF, PSDTFbase, EPS
    X = np.tile(np.eye(5)[:, :, None], (1, 1, 6))
    skew = X.copy()
    skew[0, 1] = 1.0
    for dtype in ("float32", "complex128", np.float32):
        with pytest.raises(ValueError, match="float64"):
            LDPSDTF(3, dtype=dtype)
    refused = [(LDPSDTF(0), X, "n_basis"), (LDPSDTF(65), X, "n_basis"), (LDPSDTF(2.5), X, "n_basis"),
               (LDPSDTF(3), np.ones((0, 0, 6)), "n_bins"), (LDPSDTF(3), np.ones((65, 65, 2)), "n_bins"),
               (LDPSDTF(3), np.ones((5, 4, 6)), "square"), (LDPSDTF(3), np.ones((5, 5, 0)), "empty"),
               (LDPSDTF(3), np.ones((5, 5)), "dims"), (LDPSDTF(3), np.ones((2, 2, 5, 5, 6)), "dims"),
               (LDPSDTF(3), X.astype(np.complex128), "real"), (LDPSDTF(3), skew, "symmetric")]
    for model, target, what in refused:
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match=what):
            model(target, iteration=1)
        assert model._engine is None and np.array_equal(np.random.get_state()[1], state)
        assert model.loss == [] and not hasattr(model, "basis") and not hasattr(model, "activation")
    warm = [("basis", np.ones((5, 5, 3), dtype=np.complex128), "real"), ("basis", np.ones((5, 5, 2)), "shape"),
            ("basis", np.triu(np.ones((5, 5)))[:, :, None] * np.ones(3), "symmetric"),
            ("activation", np.ones((3, 7)), "shape")]
    for attr, value, what in warm:
        model = LDPSDTF(3)
        setattr(model, attr, value)
        with pytest.raises(ValueError, match=what):
            model(X, iteration=1)
        assert model._engine is None
    model = LDPSDTF(4)
    assert (model.n_basis, model.algorithm, model.normalize, model.eps, model.loss, EPS) == (4, 'mm', True, 1e-12, [], 1e-12)
    assert PSDTFbase().n_basis == 2 and LDPSDTF().n_basis == 2


def test_generator_reproduces_the_fixtures():
    reference_src()
    run = subprocess.run([sys.executable, os.path.join(pt.GOLDEN, "make_psdtf.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified 10 files, 0 problems" in run.stdout, run.stdout + run.stderr


def test_probe_reproduces_the_tolerances():
    reference_src()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psdtf_tolerance_probe.py"), "--check"],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "tolerances.json reproduced" in run.stdout, run.stdout + run.stderr
