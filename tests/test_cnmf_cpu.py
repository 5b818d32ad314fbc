"""ComplexEUCNMF without a GPU: the NumPy restatement (tests/cnmf_np.py) against the reference's recorded states
(tests/golden/cnmf/*.npz) one update at a time, the C-ABI names, the workspace query and the host-side refusals."""
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
import cnmf_np as cn  # noqa: E402

FILES = cn.fixture_files()
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ENTRY_POINTS = ("workspace_bytes", "update", "loss", "beta", "reconstruct", "iterate")


def test_fixtures_and_tolerances_are_complete():
    tol = cn.tolerances()
    assert len(NAMES) == 10 and sorted(tol["loss_20"]) == NAMES
    assert tol["factor"] == 16 and set(tol["one_update"]) == {"T", "V", "components", "loss"}
    assert 0 < max(tol["one_update"].values()) <= 1e-10  # above: the restatement would not be the reference's update
    for f in FILES:
        assert os.path.getsize(f) <= 484699, f  # the largest file of tests/golden/mnmf
        fx = np.load(f)
        for it in cn.SNAP_ITERS:
            assert all("%s_%d" % (a, it) in fx.files for a in ("basis", "activation", "phase")), (f, it)
        assert fx["loss"].shape == (20,) and fx["loss_reference"].shape == (20,)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_one_update_at_a_time(name):
    fx = np.load(os.path.join(cn.GOLDEN, name + ".npz"))
    tol = cn.tolerances()["one_update"]
    X, (reg, p, eps) = fx["X"], cn.params(fx)
    starts = cn.start_iters(fx)
    assert set(starts) >= {0, 1, 19}
    for it in starts:
        start = cn.state(fx, it)
        kept = [a.copy() for a in start]
        got = cn.update(X, *start, reg, p, eps)
        assert all(np.array_equal(a, b) for a, b in zip(start, kept))  # the restatement leaves its inputs alone
        want = cn.state(fx, it + 1)
        for metric, err in cn.compare(got, want, X).items():  # every entry of T, V and the components, and the loss
            assert err <= tol[metric], (it, metric, err)
        assert cn.rel(cn.loss(X, *want), fx["loss"][it]) <= tol["loss"]
        assert got[2].shape == want[2].shape and np.all(np.abs(got[2]) <= np.pi)


def test_recorded_cases_cover_what_they_claim():
    by = {n: np.load(os.path.join(cn.GOLDEN, n + ".npz")) for n in NAMES}
    silent = by["cnmf_f17_t40_k1_p1_r0p1_silent"]
    quiet = silent["X"] == 0
    assert quiet[3].all() and quiet[:, 5:7].all()
    for it in cn.SNAP_ITERS:  # Zbar is exactly 0 there, so the angle is 0
        assert np.all(silent["phase_%d" % it][:, 0, :][quiet] == 0)
    assert np.array_equal(cn.beta(silent["T0"], silent["V0"], 1e-12), np.ones_like(silent["phase_1"]))  # one basis
    neg = by["cnmf_f17_t40_k7_p1_r0p1_silent"]
    assert (neg["basis_20"] < 0).any() and (neg["activation_20"] < 0).any()
    assert (by["cnmf_f5_t257_k16_p0p7_r0p01"]["activation_20"] < 0).any()
    for fx in by.values():
        assert all(np.isfinite(fx[k]).all() for k in fx.files if k != "versions")


def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "assx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_cnmf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted("assx_cnmf_" + n for n in ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_cnmf_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_cnmf_workspace_bytes
    base = q(1, 17, 40, 3, _lib.F64)
    assert base > (3 * 17 * 40 + 17 * 3) * 8
    assert q(0, 17, 40, 3, _lib.F64) == 0
    assert q(2, 17, 40, 3, _lib.F64) > base and q(1, 18, 40, 3, _lib.F64) > base
    assert q(1, 17, 41, 3, _lib.F64) > base and q(1, 17, 40, 4, _lib.F64) > base
    assert q(1, 17, 40, 0, _lib.F64) == 0 and q(1, 17, 40, 65, _lib.F64) == 0 and q(1, 17, 40, 3, _lib.F32) == 0
    assert q(4, 1025, 4096, 64, _lib.F64) > 4 * 1025 * 4096 * 3 * 8  # sizes in 64-bit arithmetic


def test_class_refuses_float32_and_65_bases_before_touching_a_device():
    from audio_source_separation_amd.algorithm.nmf import ComplexEUCNMF
    X = np.ones((5, 6), dtype=np.complex128)
    with pytest.raises(ValueError, match="float64"):
        ComplexEUCNMF(dtype="float32")
    for K in (65, 0):
        model = ComplexEUCNMF(n_basis=K)
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match="n_basis"):
            model(X, iteration=1)
        assert model._engine is None and np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError, match="n_basis"):
        ComplexEUCNMF(n_basis=2)(X, iteration=1, n_basis=65)  # kwargs are applied before the check
    model = ComplexEUCNMF()
    assert (model.n_basis, model.regularizer, model.p, model.eps, model.loss) == (2, 0.1, 1, 1e-12, [])


def test_generator_reproduces_the_fixtures():
    src = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")  # the default of tests/golden/make_golden.py
    if not os.path.isdir(os.path.join(src, "algorithm")):
        pytest.skip("the reference tree is not on this machine")
    run = subprocess.run([sys.executable, os.path.join(cn.GOLDEN, "make_cnmf.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified 10 files, 0 problems" in run.stdout, run.stdout + run.stderr
