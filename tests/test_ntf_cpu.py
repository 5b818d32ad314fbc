"""EUCNTF without a GPU: the NumPy restatement (tests/ntf_np.py) against the reference's recorded states
(tests/golden/ntf/*.npz) one update at a time and over the whole run, what the fixtures cover, the C-ABI names, the
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
import ntf_np as nt  # noqa: E402

FILES = nt.fixture_files()
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ENTRY_POINTS = ("workspace_bytes", "update", "loss", "reconstruct", "iterate")
ATTRS = ("partitioning", "basis", "activation")


def load(name):
    return np.load(os.path.join(nt.GOLDEN, name + ".npz"))


def reference_src():
    src = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")  # the default of tests/golden/make_golden.py
    if not os.path.isdir(os.path.join(src, "algorithm")):
        pytest.skip("the reference tree is not on this machine")


def test_fixtures_and_tolerances_are_complete():
    tol = nt.tolerances()
    assert len(NAMES) == 10
    assert tol["factor"] == 16
    assert set(tol["one_update"]) == set(nt.METRICS) and set(tol["whole_run"]) == set(nt.METRICS)
    assert 0 < min(tol["one_update"].values()) and max(tol["one_update"].values()) <= 1e-12
    assert min(tol["whole_run"].values()) >= 16 * 2.0 ** -52
    shapes = set()
    for f in FILES:
        assert os.path.getsize(f) <= 484699, f  # the project's cap for a golden file
        fx = np.load(f)
        N, I, J = fx["X"].shape
        K = fx["Z0"].shape[1]
        shapes.add((N, I, J, K))
        assert fx["Z0"].shape == (N, K) and fx["T0"].shape == (I, K) and fx["V0"].shape == (K, J)
        for it in nt.SNAP_ITERS:
            for a, shape in zip(ATTRS, ((N, K), (I, K), (K, J))):
                assert fx["%s_%d" % (a, it)].shape == shape, (f, a, it)
        assert fx["loss"].shape == (20,) and fx["rng_next"].shape == () and fx["seed"].shape == () and fx["eps"] > 0
    assert shapes == {(2, 17, 40, 3), (1, 9, 70, 1), (3, 33, 65, 6), (4, 5, 257, 16), (5, 129, 7, 10), (8, 8, 64, 64),
                      (32, 3, 5, 2), (2, 1, 70, 3), (2, 40, 1, 3), (6, 7, 9, 3)}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_one_update_at_a_time(name):
    fx = load(name)
    tol = nt.tolerances()["one_update"]
    X, eps = fx["X"], float(fx["eps"])
    for it in nt.START_ITERS:
        start = nt.state(fx, it)
        kept = [a.copy() for a in start]
        x_kept = X.copy()
        got = nt.update(X, *start, eps)
        assert all(np.array_equal(a, b) for a, b in zip(start, kept)) and np.array_equal(X, x_kept)
        want = nt.state(fx, it + 1)
        for metric, err in nt.compare(got, want, X).items():  # every entry of Z, T and V, and the loss
            assert err <= tol[metric], (it, metric, err)
        assert nt.rel_entry(nt.loss(X, *want), fx["loss"][it]) <= tol["loss"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_over_the_whole_run(name):
    fx = load(name)
    tol = nt.tolerances()["whole_run"]
    X, eps = fx["X"], float(fx["eps"])
    run = nt.run(X, nt.state(fx, 0), eps, nt.N_ITER)
    for metric, a, b in zip(("Z", "T", "V"), run[-1], nt.state(fx, 20)):
        assert nt.rel_entry(a, b) <= tol[metric], metric
    assert nt.rel_entry(np.array([nt.loss(X, *s) for s in run]), fx["loss"]) <= tol["loss"]


def test_recorded_cases_cover_what_they_claim():
    by = {n: load(n) for n in NAMES}
    for fx in by.values():
        for k in fx.files:
            if k not in ("versions", "X", "seed"):
                assert np.isfinite(fx[k]).all() and (fx[k] >= np.finfo(np.float64).tiny).all(), k
        assert np.isfinite(fx["X"]).all() and (fx["X"] >= 0).all()
    silent = by["ntf_n3_i33_j65_k6_silent"]
    quiet = silent["X"] == 0
    assert quiet[:, 3, :].all() and quiet[:, :, 5:7].all() and quiet[1].all() and not quiet[0].all()
    eps = float(silent["eps"])
    sums = []
    nt.update(silent["X"], *nt.state(silent, 0), eps, sums=sums)
    (tn, _), (vn, _), (zn, _) = sums  # the numerators: zero, so floored, exactly where the target is silent
    assert (tn[3] < eps).all() and (vn[:, 5:7] < eps).all() and (zn[1] < eps).all()
    assert (np.delete(tn, 3, axis=0) >= eps).all() and (zn[[0, 2]] >= eps).all()
    assert silent["partitioning_20"][1].max() < 1e-6 * silent["partitioning_20"][[0, 2]].min()  # Z[1] collapses

    floor = by["ntf_n6_i7_j9_k3_floor"]
    eps = float(floor["eps"])
    assert eps == 4.0
    both = [False] * 6
    for it in nt.START_ITERS:
        sums = []
        nt.update(floor["X"], *nt.state(floor, it), eps, sums=sums)
        for q, s in enumerate(s for pair in sums for s in pair):
            both[q] = both[q] or bool((s < eps).any() and (s >= eps).any())
    assert all(both), both  # each of the six floored sums binds somewhere and stays free somewhere


def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "assx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_ntf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted("assx_ntf_" + n for n in ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_ntf_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_ntf_workspace_bytes
    base = q(1, 2, 17, 40, 3, _lib.F64)
    assert base > 0
    assert q(2, 2, 17, 40, 3, _lib.F64) > base and q(1, 3, 17, 40, 3, _lib.F64) > base
    assert q(1, 2, 18, 40, 3, _lib.F64) > base and q(1, 2, 17, 41, 3, _lib.F64) > base
    assert q(1, 2, 17, 40, 4, _lib.F64) > base
    for B, N, I, J, K, dt in ((1, 2, 17, 40, 0, _lib.F64), (1, 2, 17, 40, 65, _lib.F64), (1, 0, 17, 40, 3, _lib.F64),
                              (1, 33, 17, 40, 3, _lib.F64), (1, 2, 17, 40, 3, _lib.F32), (0, 2, 17, 40, 3, _lib.F64),
                              (1, 2, 0, 40, 3, _lib.F64), (1, 2, 17, 0, 3, _lib.F64)):
        assert q(B, N, I, J, K, dt) == 0, (B, N, I, J, K, dt)
    assert q(1, 32, 17, 40, 64, _lib.F64) > 0
    # no reconstruction of X in the workspace: at most half of X's bytes at the large shape
    assert 0 < q(1, 4, 1025, 4096, 32, _lib.F64) <= 4 * 1025 * 4096 * 8 // 2
    assert q(64, 32, 1025, 4096, 64, _lib.F64) > 2 ** 32  # sizes in 64-bit arithmetic


def test_class_refusals_touch_neither_a_device_nor_the_rng():
    from audio_source_separation_amd.algorithm.ntf import EUCNTF, NTFbase, EPS
    X = np.ones((2, 5, 6))
    for dtype in ("float32", "complex128", np.float32):
        with pytest.raises(ValueError, match="float64"):
            EUCNTF(3, dtype=dtype)
    refused = [(EUCNTF(0), X, "n_basis"), (EUCNTF(65), X, "n_basis"), (EUCNTF(2.5), X, "n_basis"),
               (EUCNTF(3), np.ones((0, 5, 6)), "n_channels"), (EUCNTF(3), np.ones((33, 5, 6)), "n_channels"),
               (EUCNTF(3), np.ones((5, 6)), "dims"), (EUCNTF(3), np.ones((2, 2, 2, 5, 6)), "dims")]
    for model, target, what in refused:
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match=what):
            model(target, iteration=1)
        assert model._engine is None and np.array_equal(np.random.get_state()[1], state)
        assert model.loss == [] and not hasattr(model, "partitioning")
    model = EUCNTF(4)
    assert (model.n_basis, model.eps, model.loss, EPS) == (4, 1e-12, [], 1e-12)
    assert NTFbase().n_basis == 2
    with pytest.raises(TypeError):
        model(X, iteration=1, n_basis=3)  # no keyword attributes, as in the reference


def test_generator_reproduces_the_fixtures():
    reference_src()
    run = subprocess.run([sys.executable, os.path.join(nt.GOLDEN, "make_ntf.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified 10 files, 0 problems" in run.stdout, run.stdout + run.stderr


def test_probe_reproduces_the_tolerances():
    reference_src()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ntf_tolerance_probe.py"), "--check"],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "tolerances.json reproduced" in run.stdout, run.stdout + run.stderr
