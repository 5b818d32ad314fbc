"""ProxLaplaceIVA without a GPU: the NumPy restatement (tests/pdsbss_np.py) against the reference-recorded cases of
tests/golden/pdsbss, planted faults that the cases must catch, the prox against its definition, the C-ABI's symbol list, its
workspace query and refusals, and what the classes refuse and print without a device.

Tolerances: the restatement and the reference are two float64 programs that sum in different orders, so a stage from a
recorded state is held to pdsbss_envelope_np.tolerance and a whole run to trajectory_tolerance (256 x the restatement's
own one-rounding sensitivity, floor 1e-13), the figures the GPU tests use.  The loss is not asserted to fall: primal-dual
splitting is no descent method on it.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import pdsbss_np as pd  # noqa: E402
import pdsbss_envelope_np as penv  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pdsbss")
NAMES = pd.cases(GOLDEN)
ENTRY_POINTS = ("assx_pdsbss_workspace_bytes", "assx_pdsbss_operator_norm", "assx_pdsbss_adjoint", "assx_pdsbss_prox_logdet",
                "assx_pdsbss_forward", "assx_pdsbss_prox_group", "assx_pdsbss_update", "assx_pdsbss_loss",
                "assx_pdsbss_iterate")
STAGE_KIND = {"G": "G", "Wt": "W", "z": "y", "yt": "y"}


def load(name):
    return pd.load_case(GOLDEN, name)


def test_fixtures_are_complete():
    shapes, params, shares = set(), [], {}
    for name in NAMES:
        g = load(name)
        M, F, T = g["X"].shape
        tag = "" if re.fullmatch(r"t\d+", name.split("_")[-1]) else name.split("_")[-1]
        shapes.add((M, F, T, tag))
        assert g["loss"].shape == (pd.N_ITER + 1,) and g["output"].shape == (M, F, T) and g["shrink"].shape == (pd.N_ITER,)
        assert abs(np.mean(np.abs(g["X"]) ** 2) - 1.0) < 1e-12
        for it in (0,) + pd.SNAP_ITERS:
            assert g["W_%d" % it].shape == (F, M, M) and g["W_%d" % it].dtype == np.complex128
            if it:
                assert g["y_%d" % it].shape == (F, M, T) and g["y_%d" % it].dtype == np.complex128
        for it in pd.STAGE_ITERS:
            assert g["G_%d" % it].shape == g["Wt_%d" % it].shape == (F, M, M)
            assert g["z_%d" % it].shape == g["yt_%d" % it].shape == (F, M, T)
        assert all(np.all(np.isfinite(v)) for k, v in g.items() if k != "versions")
        assert np.array_equal(g["W_0"], pd.identity(M, F)) == (tag != "warm")
        assert bool(g["projection_back"]) == (tag != "nopb")
        assert float(g["mu1"]) > 0 and float(g["mu2"]) > 0 and float(g["norm"]) > 0
        params.append(tuple(pd.params(g).values()))
        # the branch conditions, from the recorded arrays: no group norm next to 1 / mu2, the recorded share is the arrays'
        for it in pd.STAGE_ITERS:
            moved, gap = pd.shrinking(g["z_%d" % it], 1 / float(g["mu2"]))
            assert gap >= 1e-6 and moved.mean() == g["shrink"][it - 1]
            sv = np.linalg.svd(g["W_%d" % (it - 1)] - float(g["mu1"]) * float(g["mu2"]) * g["G_%d" % it], compute_uv=False)
            assert np.all(sv[:, -1] >= 1e-6 * sv[:, 0])
        shares[name] = g["shrink"][[it - 1 for it in pd.SNAP_ITERS]]
        parts = [name + ".npz"] + ["%s.part%d.npz" % (name, i) for i in range(1, int(g["n_parts"]))]
        assert all(os.path.getsize(os.path.join(GOLDEN, p)) < 150 * 1024 for p in parts)
    assert len([f for f in os.listdir(GOLDEN) if f.endswith(".npz")]) == sum(int(load(n)["n_parts"]) for n in NAMES)
    wanted = {(2, 5, 33, ""), (3, 4, 70, ""), (4, 6, 64, ""), (5, 3, 48, ""), (6, 2, 40, ""), (7, 2, 40, ""),
              (8, 3, 130, ""), (2, 4, 257, ""), (3, 4, 50, "warm"), (3, 5, 45, "nopb")}
    assert wanted <= shapes
    odd = [p for p in params if p != (1.0, 1.0, 1.0, 1.0)]
    assert len(odd) >= 3 and any(p[3] > 1 for p in odd) and any(p[3] < 1 for p in odd)
    assert any(p[0] != 1 for p in odd) and any(p[1] != 1 for p in odd) and any(p[2] != 1 for p in odd)
    # both branches of the shrinkage, each on >= 5 % of the cells of one recorded iteration; and a case that shrinks >= 90 %
    assert any(np.any((s >= 0.05) & (s <= 0.95)) for s in shares.values())
    assert any(np.any(s >= 0.90) for s in shares.values())


def run_distances(name, **fault):
    g = load(name)
    states, losses, stages = pd.run(g["X"], g["W_0"], pd.N_ITER, float(g["norm"]), **pd.params(g), **fault)
    d = {"W": max(penv.entrywise("W", states[it][0], g["W_%d" % it]) for it in pd.SNAP_ITERS),
         "y": max(penv.entrywise("y", states[it][1], g["y_%d" % it]) for it in pd.SNAP_ITERS),
         "loss": penv.entrywise("loss", losses, g["loss"])}
    return d, states


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    """Every recorded stage from the recorded state before it, every recorded state and loss of the whole run, the output
    and the norm."""
    g = load(name)
    par = pd.params(g)
    Xn = g["X"] / float(g["norm"])
    zero = np.zeros_like(g["z_1"])
    for it in pd.STAGE_ITERS:
        W, y = g["W_%d" % (it - 1)], (g["y_%d" % (it - 1)] if it > 1 else zero)
        Wn, yn, st = pd.update(Xn, W, y, **par)
        for k, kind in STAGE_KIND.items():
            d = penv.entrywise(kind, st[k], g["%s_%d" % (k, it)])
            assert d <= penv.tolerance({"G": "adjoint", "W": "prox_logdet", "y": "forward"}[kind]), (it, k, d)
        assert penv.entrywise("W", Wn, g["W_%d" % it]) <= penv.tolerance("update_W")
        assert penv.entrywise("y", yn, g["y_%d" % it]) <= penv.tolerance("update_y")
    d, states = run_distances(name)
    for k, v in d.items():
        assert v <= penv.trajectory_tolerance(k), (k, v)
    out = pd.separate(g["X"], states[pd.N_ITER][0], int(g["reference_id"]), bool(g["projection_back"]))
    assert penv.entrywise("output", out, g["output"]) <= penv.trajectory_tolerance("output")
    assert penv.entrywise("norm", pd.operator_norm(g["X"]), g["norm"]) <= penv.tolerance("norm")
    assert np.array_equal(g["y_1"], g["yt_1"]) == (float(g["alpha"]) == 1.0)


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", ("no_conj", "z_from_wt", "drop_c", "per_bin"))
def test_fixtures_catch_a_planted_fault(fault):
    """G without the conjugate; z from W~ in place of 2 W~ - W; C dropped from the shrinkage (seen only where C != 1); the
    shrinkage applied per bin instead of across the bins."""
    caught = []
    for name in NAMES:
        d, _ = run_distances(name, **{fault: True})
        if any(v > penv.trajectory_tolerance(k) for k, v in d.items()):
            caught.append(name)
    need = len([n for n in NAMES if float(load(n)["C"]) != 1.0]) if fault == "drop_c" else len(NAMES) // 2
    assert len(caught) >= max(need, 1), (fault, caught)


def test_prox_logdet_against_its_definition():
    """The singular values of the result are h(sigma), its singular vectors those of the argument; W = I gives h(1) I; the
    result minimises mu (-ln|det V|) + |V - W|^2 / 2 against nearby matrices."""
    rng = np.random.default_rng(5)
    for M in range(2, 9):
        W = rng.standard_normal((3, M, M)) + 1j * rng.standard_normal((3, M, M))
        for mu in (0.3, 1.0, 2.5):
            V = pd.prox_logdet(W, mu)
            s, sv = np.linalg.svd(W, compute_uv=False), np.linalg.svd(V, compute_uv=False)
            assert np.allclose(sv, pd.h(s, mu), rtol=1e-12)
            assert np.allclose(pd.prox_logdet(np.eye(M)[None] + 0j, mu)[0], pd.h(1.0, mu) * np.eye(M), atol=1e-14)

            def cost(A, f):
                return -mu * np.log(np.abs(np.linalg.det(A))) + 0.5 * np.sum(np.abs(A - W[f]) ** 2)

            for f in range(3):
                E = 1e-4 * (rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M)))
                assert cost(V[f], f) < cost(V[f] + E, f) and cost(V[f], f) < cost(V[f] - E, f)


def test_group_shrinkage_against_its_definition():
    z = np.zeros((3, 2, 4), dtype=complex)
    z[:, 0, 0] = (3.0, 4.0j, 0.0)    # den 5
    z[:, 1, 1] = (0.3, 0.0, 0.4)     # den 0.5
    p = pd.prox_group(z, 1.0, 0.5)   # frames 2, 3 and the other cells: den = 0 -> mu, factor 0
    assert np.allclose(p[:, 0, 0], 0.5 * (1 - 1 / 5) * z[:, 0, 0]) and np.all(p[:, 1, 1] == 0) and np.all(p[:, :, 2:] == 0)
    assert np.all(np.isfinite(p))


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "assx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_pdsbss_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_pdsbss_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    build = open(os.path.join(ROOT, "audio_source_separation_amd", "csrc", "build.sh")).read()
    assert build.count("assx_pdsbss") == 2  # the SRCS list and the link line
    chunk = int(re.search(r"#define ASSX_PDSBSS_FRAME_CHUNK (\d+)", raw).group(1))
    assert chunk == _lib.PDSBSS_FRAME_CHUNK == penv.FRAME_CHUNK
    assert _lib.PDSBSS_LAPLACE == 0
    for n in declared:  # the comments cite the reference lines each entry point replaces
        if n != "assx_pdsbss_workspace_bytes":
            assert re.search(r"\b%s\s+(prox|iva)\.py:\d+" % n, raw), n


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_pdsbss_workspace_bytes
    base = q(4, 17, 65)
    assert base > 0 and q(5, 17, 65) > base and q(4, 18, 65) > base and q(4, 17, 1025) > base
    for M, F, T in ((1, 17, 65), (9, 17, 65), (4, 0, 65), (4, 17, 0), (4, -1, 65), (4, 17, -1)):
        assert q(M, F, T) == 0, (M, F, T)
    assert q(2, 1, 1) > 0 and q(8, 1, 1) > 0
    assert q(8, 4096, 8191) > 0 and q(2, 64, 2 ** 21 - 1) > 2 ** 31  # sizes in 64-bit arithmetic
    assert q(8, 4096, 8192) == 0       # M F T < 2^28
    assert q(2, 2 ** 31 - 1, 2 ** 31 - 1) == 0 and q(2, 2 ** 31 - 1, 1) == 0


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes and the penalty."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    for M, F, T in ((4, 5, 6), (9, 0, -1)):
        for pen in (0, 7):
            assert L.assx_pdsbss_operator_norm(null, null, null, null, M, F, T, null, null) == E_NULL
            assert L.assx_pdsbss_adjoint(null, null, null, null, null, null, M, F, T, null) == E_NULL
            assert L.assx_pdsbss_prox_logdet(null, null, null, -1.0, M, F, null, null) == E_NULL
            assert L.assx_pdsbss_forward(null, null, null, null, null, null, M, F, T, null) == E_NULL
            assert L.assx_pdsbss_prox_group(null, pen, null, null, null, 1.0, -1.0, M, F, T, null) == E_NULL
            assert L.assx_pdsbss_update(null, pen, null, null, null, null, null, 1.0, -1.0, 1.0, 1.0, M, F, T, null,
                                        null) == E_NULL
            assert L.assx_pdsbss_loss(null, pen, null, null, null, 1.0, null, null, M, F, T, null) == E_NULL
            assert L.assx_pdsbss_iterate(null, -1, 3, pen, null, null, null, null, null, 1.0, 1.0, 0.0, 1.0, null, M, F, T,
                                         null, null) == E_NULL


# ------------------------------------------------------------------------------------------------ the classes
def new(**kw):
    from audio_source_separation_amd import bss
    return bss.ProxLaplaceIVA(**kw)


def test_class_refusals_touch_no_device():
    from audio_source_separation_amd import bss
    X = pd.mixture(3, 4, 20, 0)
    for cls in (bss.ProxLaplaceIVA, bss.PDSBSSbase):
        for dtype in ("float32", np.float32, "complex64"):
            with pytest.raises(ValueError, match="float64"):
                cls(dtype=dtype)
    refused = [(new(), X.real, "complex"), (new(), X[None], "one utterance"), (new(), X[0], "one utterance"),
               (new(), X[:1], "n_channels"), (new(), np.ones((9, 4, 20), dtype=complex), "n_channels"),
               (new(), X[:, :0], "empty"), (new(), X[:, :, :0], "empty"),
               (new(reference_id=3), X, "reference_id"), (new(reference_id=-1), X, "reference_id"),
               (new(reference_id=0.0), X, "reference_id")]
    for attr in ("regularizer", "step_prox_logdet", "step_prox_penalty", "step"):
        refused += [(new(**{attr: v}), X, attr) for v in (np.inf, np.nan, "1", 1j, True)]
    refused += [(new(step_prox_logdet=0), X, "step_prox_logdet"), (new(step_prox_logdet=-1.0), X, "step_prox_logdet"),
                (new(step_prox_penalty=0.0), X, "step_prox_penalty"), (new(step_prox_penalty=-2), X, "step_prox_penalty")]
    for model, x, what in refused:
        with pytest.raises(ValueError, match=what):
            model(x, 1)
        assert model._engine is None and model.loss == [] and not hasattr(model, "demix_filter"), what
        assert not hasattr(model, "y") and not hasattr(model, "norm")
    for W0, what in ((np.ones((4, 3, 2), dtype=complex), "shape"), (np.ones((5, 3, 3), dtype=complex), "shape")):
        model = new()
        with pytest.raises(ValueError, match=what):
            model(X, 1, demix_filter=W0)
        assert model._engine is None
    with pytest.raises(TypeError):  # `iteration` has no default (iva.py:838)
        new()(X)


def test_constructors_defaults_and_repr():
    from audio_source_separation_amd import bss
    from audio_source_separation_amd.bss.prox import PDSBSSbase
    assert bss.PDSBSSbase is PDSBSSbase and issubclass(bss.ProxLaplaceIVA, PDSBSSbase)
    assert {"PDSBSSbase", "ProxLaplaceIVA"} <= set(bss.__all__) and not hasattr(bss, "SparseProxIVA")
    m = new()
    assert (m.regularizer, m.step_prox_logdet, m.step_prox_penalty, m.step, m.reference_id, m.callbacks,
            m.apply_projection_back, m.recordable_loss, m.eps, m.loss, m.input) == \
        (1, 1.0, 1.0, 1.0, 0, None, True, True, 1e-12, [], None)
    assert repr(m) == "ProxLaplaceIVA(regularizer=1, step_prox_logdet=1.0, step_prox_penalty=1.0, step=1.0)"
    m = bss.ProxLaplaceIVA(0.5, 2.0, 0.25, 1.75, 1, print, False, False, 1e-9)
    assert (m.regularizer, m.step_prox_logdet, m.step_prox_penalty, m.step, m.reference_id, m.callbacks,
            m.apply_projection_back, m.recordable_loss, m.eps, m.loss) == (0.5, 2.0, 0.25, 1.75, 1, [print], False, False,
                                                                           1e-9, None)
    assert repr(m) == "ProxLaplaceIVA(regularizer=0.5, step_prox_logdet=2.0, step_prox_penalty=0.25, step=1.75)"
    b = PDSBSSbase(2, 3.0, 4.0, 0.5, None, True, 1e-10)
    assert (b.regularizer, b.step_prox_logdet, b.step_prox_penalty, b.step, b.eps) == (2, 3.0, 4.0, 0.5, 1e-10)
    assert not hasattr(b, "reference_id") and not hasattr(b, "apply_projection_back")
    assert not hasattr(m, "input_sparse") and not hasattr(m, "demix_filter_sparse")
    with pytest.raises(NotImplementedError, match="prox_penalty"):
        b.prox_penalty(np.zeros((1, 2, 3), dtype=complex), 1.0)
    with pytest.raises(NotImplementedError, match="compute_penalty"):
        b.compute_penalty()


def test_loop_rule():
    """A fresh model takes the one-call loop, with or without the loss; callbacks, a plain loss list or any overridden step
    keep the Python loop, and so does a PDSBSSbase subclass with a prox of its own."""
    from audio_source_separation_amd import bss
    cls = bss.ProxLaplaceIVA
    steps = ("separate", "prox_logdet", "prox_penalty", "compute_penalty", "compute_negative_logdet",
             "compute_negative_loglikelihood", "update_once", "_record_loss")
    assert "_OWN_STEPS" in vars(cls) and sorted(cls._OWN_STEPS) == sorted(steps)
    assert new()._fast_loop_ok() and new(recordable_loss=False)._fast_loop_ok()
    assert not new(callbacks=lambda m: None)._fast_loop_ok()
    for name in steps:
        sub = type("Sub_" + name, (cls,), {name: lambda self, *a, **k: getattr(cls, name)(self, *a, **k)})
        assert not sub()._fast_loop_ok(), name

    class Renamed(cls):
        pass

    assert Renamed()._fast_loop_ok()
    plain = new()
    plain.loss = []
    assert not plain._fast_loop_ok()

    class Own(bss.PDSBSSbase):
        def prox_penalty(self, z, mu=1):
            return z

        def compute_penalty(self):
            return 0.0

    assert not Own()._fast_loop_ok() and not bss.PDSBSSbase()._fast_loop_ok()


def test_generator_reproduces_the_fixtures():
    if not os.path.isdir(os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")):
        pytest.skip("the reference tree is not present")
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_pdsbss.py"), "--verify"], capture_output=True,
                         text=True)
    n_files = len([f for f in os.listdir(GOLDEN) if f.endswith(".npz")])
    assert run.returncode == 0 and "verified %d files, 0 problems" % n_files in run.stdout, run.stdout + run.stderr
