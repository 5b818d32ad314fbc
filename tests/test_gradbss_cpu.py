"""The gradient family without a GPU: the NumPy restatement (tests/gradbss_np.py) against the reference-recorded fixtures of
tests/golden/gradbss, planted faults that the fixtures must catch, the host model of the solver's rank rule, the C-ABI's
symbol list, its workspace query and refusals, and what the classes refuse and print without a device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import gradbss_np as gb  # noqa: E402
import gradbss_envelope_np as genv  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "gradbss")
FILES = gb.fixtures(GOLDEN)
NAMES = [os.path.basename(f)[:-4] for f in FILES]
FDICA = [n for n in NAMES if "FDICA" in n]
ENTRY_POINTS = ("assx_gradbss_workspace_bytes", "assx_gradbss_update", "assx_gradbss_loss", "assx_gradbss_iterate",
                "assx_fdica_solve_permutation")
# the restatement against the reference, W per bin relative to the bin's largest entry and every loss relatively: the
# maker's own figures are 0 for W and at most 2.1e-15 for the loss
TOL = 1e-12


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def cls_of(name):
    return name.split("_")[0]


def distances(name, **fault):
    g = load(name)
    model, natural = gb.CLASSES[cls_of(name)]
    states, losses = gb.run(model, natural, g["X"], g["W_0"], gb.N_ITER, float(g["lr"]), float(g["eps"]), **fault)
    dW = max(genv.entrywise("W", states[it], g["W_%d" % it]) for it in gb.SNAP_ITERS)
    return dW, genv.entrywise("loss", losses, g["loss"])


def test_fixtures_are_complete():
    shapes = {}
    for name in NAMES:
        g = load(name)
        M, F, T = g["X"].shape
        tag = name.split("_")[-1] if name.split("_")[-1] in ("warm", "nopb") else ""
        shapes.setdefault(cls_of(name), set()).add((M, F, T, tag))
        assert g["loss"].shape == (gb.N_ITER + 1,) and g["output"].shape == (M, F, T)
        assert float(g["lr"]) == 0.1 and float(g["eps"]) == gb.EPS
        assert abs(np.mean(np.abs(g["X"]) ** 2) - 1.0) < 1e-12
        for it in (0,) + gb.SNAP_ITERS:
            assert g["W_%d" % it].shape == (F, M, M) and g["W_%d" % it].dtype == np.complex128
        assert np.all(np.diff(g["loss"]) < 0)  # the losses fall monotonically
        assert np.array_equal(g["W_0"], gb.identity(M, F)) == (tag != "warm")
        if "FDICA" in name:
            assert g["order"].shape == (F,) and g["perm"].shape == (F, M) and g["gaps"].min() >= 1e-8
            assert sorted(g["order"]) == list(range(F)) and all(sorted(p) == list(range(M)) for p in g["perm"])
            assert np.array_equal(g["W_pre"], g["W_%d" % gb.N_ITER])
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 150 * 1024
    wanted = {(2, 5, 33, ""), (3, 4, 70, ""), (4, 6, 64, ""), (5, 3, 48, ""), (6, 2, 40, ""), (7, 2, 40, ""),
              (8, 3, 130, ""), (2, 4, 257, ""), (3, 4, 50, "warm")}
    assert sorted(shapes) == sorted(gb.CLASSES)
    for c, have in shapes.items():
        assert wanted <= have, c
        assert ((3, 5, 45, "nopb") in have) == ("IVA" in c)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    """W entry-wise at every recorded iteration, loss by loss, the output; for FDICA order and perm as exact integers
    and W after the solver as exact row copies."""
    g = load(name)
    dW, dl = distances(name)
    assert dW < TOL and dl < TOL, (dW, dl)
    W = g["W_post"] if "FDICA" in name else g["W_%d" % gb.N_ITER]
    out = gb.separate(g["X"], W, int(g["reference_id"]), bool(g["projection_back"]))
    assert genv.entrywise("output", out, g["output"]) < 1e-9
    if "FDICA" in name:
        Wn, order, perm, gaps = gb.solve_permutation(g["X"], g["W_pre"], float(g["eps"]))
        assert np.array_equal(order, g["order"]) and np.array_equal(perm, g["perm"])
        assert np.array_equal(Wn, g["W_post"]) and np.array_equal(np.array(gaps), g["gaps"])
        assert all(np.array_equal(Wn[f], g["W_pre"][f][perm[f]]) for f in range(len(order)))


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault,only", (("natural_with_x", "Natural"), ("floor_square", "IVA")))
def test_fixtures_catch_a_planted_update_fault(fault, only):
    """x^H in place of y^H in the natural form: against the recorded runs.  The floor applied to r^2 instead of r: that
    fault only shows where a weight is below sqrt(eps), and with the recorded eps = 1e-12 that is 1e-6, exactly the bound
    the maker keeps every denominator above -- no recorded run can see it.  It is therefore planted with eps = 0.1
    (sqrt(eps) = 0.32, inside the range of the weights) on every IVA fixture's input and first filters, the restatement
    with the fault against the restatement without."""
    caught = []
    for name in NAMES:
        if only not in name:
            continue
        if fault == "natural_with_x":
            dW, dl = distances(name, natural_with_x=True)
        else:
            g = load(name)
            model, natural = gb.CLASSES[cls_of(name)]
            good = gb.update(model, natural, g["X"], g["W_0"], eps=1e-1)
            bad = gb.update(model, natural, g["X"], g["W_0"], eps=1e-1, floor_square=True)
            dW, dl = genv.entrywise("W", bad, good), 0.0
        if max(dW, dl) >= TOL:
            caught.append(name)
    assert caught, "no fixture sees %s" % fault


@pytest.mark.parametrize("fault", ("columns", "descending"))
def test_fixtures_catch_a_planted_solver_fault(fault):
    """Columns permuted instead of rows; descending instead of ascending bin order."""
    caught = []
    for name in FDICA:
        g = load(name)
        Wn, order, perm, _ = gb.solve_permutation(g["X"], g["W_pre"], float(g["eps"]), **{fault: True})
        if not (np.array_equal(Wn, g["W_post"]) and np.array_equal(order, g["order"]) and np.array_equal(perm, g["perm"])):
            caught.append(name)
    assert len(caught) >= len(FDICA) // 2, caught


# ------------------------------------------------------------------------------------------------ the rank rule
def test_rank_rule_gives_a_permutation_for_any_input():
    nan, inf = np.nan, np.inf
    for c in ([3.0, 1.0, 2.0], [1.0, 1.0, 1.0], [nan, 1.0, nan, 0.5], [nan] * 5, [inf, -inf, nan, 0.0, 0.0, inf], [2.0]):
        order = gb.rank_order(c)
        assert sorted(order) == list(range(len(c))), (c, order)
    assert list(gb.rank_order([3.0, 1.0, 2.0])) == [1, 2, 0]
    assert list(gb.rank_order([1.0, 1.0, 1.0])) == [0, 1, 2]                 # equal values by index
    assert list(gb.rank_order([nan, 1.0, nan, 0.5])) == [3, 1, 0, 2]          # NaN last, by index
    assert list(gb.rank_order([inf, -inf, nan, 0.0, 0.0, inf])) == [1, 3, 4, 0, 5, 2]
    rng = np.random.default_rng(0)
    for N in range(2, 9):
        C = rng.random((N, N))
        p, scores = gb.best_permutation(C)
        assert sorted(p) == list(range(N)) and scores[list(map(tuple, gb._permutations(N))).index(tuple(p))] == scores.max()
        C[:] = nan
        assert list(gb.best_permutation(C)[0]) == list(range(N))              # every score NaN: the identity
        C[:] = 1.0
        assert list(gb.best_permutation(C)[0]) == list(range(N))              # all equal: the first
        C = rng.random((N, N))
        C[0, 0] = nan                                                         # the identity's score NaN: never beaten
        assert list(gb.best_permutation(C)[0]) == list(range(N))
        C = rng.random((N, N))
        C[0, 1] = nan                                                         # a NaN candidate never wins
        p, _ = gb.best_permutation(C)
        assert sorted(p) == list(range(N)) and p[0] != 1
    X, W = genv.state(3, 4, 9, 1)
    X[:, 2, :] = nan
    Wn, order, perm, _ = gb.solve_permutation(X, W)
    assert sorted(order) == list(range(4)) and order[-1] == 2 and all(sorted(p) == [0, 1, 2] for p in perm)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "assx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_(?:gradbss|fdica)_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if re.match(r"assx_(gradbss|fdica)_", n)) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    build = open(os.path.join(ROOT, "audio_source_separation_amd", "csrc", "build.sh")).read()
    assert build.count("assx_gradbss") == 2  # the SRCS list and the link line
    chunk = int(re.search(r"#define ASSX_GRADBSS_FRAME_CHUNK (\d+)", raw).group(1))
    assert chunk == _lib.GRADBSS_FRAME_CHUNK == genv.FRAME_CHUNK
    assert (_lib.GRADBSS_IVA, _lib.GRADBSS_FDICA) == (0, 1)


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_gradbss_workspace_bytes
    base = q(4, 17, 65)
    assert base > 0 and q(5, 17, 65) > base and q(4, 18, 65) > base and q(4, 17, 1025) > base
    for M, F, T in ((1, 17, 65), (9, 17, 65), (4, 0, 65), (4, 17, 0), (4, -1, 65), (4, 17, -1)):
        assert q(M, F, T) == 0, (M, F, T)
    assert q(2, 1, 1) > 0 and q(8, 1, 1) > 0
    assert q(8, 4096, 8191) > 0 and q(2, 64, 2 ** 21 - 1) > 2 ** 30  # sizes in 64-bit arithmetic
    assert q(8, 4096, 8192) == 0       # M F T < 2^28
    assert q(2, 2 ** 31 - 1, 2 ** 31 - 1) == 0 and q(2, 2 ** 31 - 1, 1) == 0


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    for M, F, T in ((4, 5, 6), (9, 0, -1)):
        assert L.assx_gradbss_update(null, 0, 0, null, null, null, 0.1, 1e-12, M, F, T, null, null) == E_NULL
        assert L.assx_gradbss_update(null, 7, 3, null, null, null, 0.1, 1e-12, M, F, T, null, null) == E_NULL
        assert L.assx_gradbss_loss(null, 1, null, null, null, null, M, F, T, null) == E_NULL
        assert L.assx_gradbss_iterate(null, 1, 0, 1, null, null, null, 0.1, 1e-12, null, M, F, T, null, null) == E_NULL
        assert L.assx_gradbss_iterate(null, -1, 0, 1, null, null, null, 0.1, 1e-12, null, M, F, T, null, null) == E_NULL
        assert L.assx_fdica_solve_permutation(null, null, null, null, null, null, 1e-12, M, F, T, null) == E_NULL


# ------------------------------------------------------------------------------------------------ the classes
def classes():
    from audio_source_separation_amd import bss
    return {n: getattr(bss, n) for n in gb.CLASSES}


def test_class_refusals_touch_no_device():
    X = gb.mixture(3, 4, 20, 0)
    for name, new in classes().items():
        for dtype in ("float32", np.float32, "complex64"):
            with pytest.raises(ValueError, match="float64"):
                new(dtype=dtype)
        refused = [(new(), X.real, "complex"), (new(), X[None], "one utterance"), (new(), X[0], "one utterance"),
                   (new(), X[:1], "n_channels"), (new(), np.ones((9, 4, 20), dtype=complex), "n_channels"),
                   (new(), X[:, :0], "empty"), (new(), X[:, :, :0], "empty"),
                   (new(lr=np.inf), X, "lr"), (new(lr=np.nan), X, "lr"), (new(lr="0.1"), X, "lr"), (new(lr=1j), X, "lr"),
                   (new(reference_id=3), X, "reference_id"), (new(reference_id=-1), X, "reference_id"),
                   (new(reference_id=0.0), X, "reference_id")]
        for model, x, what in refused:
            with pytest.raises(ValueError, match=what):
                model(x, iteration=1)
            assert model._engine is None and model.loss == [] and not hasattr(model, "demix_filter"), (name, what)
        if "FDICA" in name:  # the permutation solver ranks at most 65536 bins
            model = new()
            with pytest.raises(ValueError, match="n_bins"):
                model(np.ones((2, 65537, 1), dtype=complex), iteration=1)
            assert model._engine is None
        for W0, what in ((np.ones((4, 3, 2), dtype=complex), "shape"), (np.ones((5, 3, 3), dtype=complex), "shape")):
            model = new()
            with pytest.raises(ValueError, match=what):
                model(X, iteration=1, demix_filter=W0)
            assert model._engine is None


def test_constructors_defaults_and_repr():
    from audio_source_separation_amd import bss
    from audio_source_separation_amd.bss.iva import IVAbase
    c = classes()
    assert repr(c["GradLaplaceIVA"]()) == "NaturalGradIVA(lr=0.1)"
    assert repr(c["NaturalGradLaplaceIVA"](lr=0.5)) == "NaturalGradLaplaceIVA(lr=0.5)"
    assert repr(c["GradLaplaceFDICA"](0.2)) == "GradLaplaceFDICA(lr=0.2)"
    assert repr(c["NaturalGradLaplaceFDICA"]()) == "GradLaplaceFDICA(lr=0.1, is_holonomic=True)"
    assert repr(c["NaturalGradLaplaceFDICA"](0.1, 0, False)) == "GradLaplaceFDICA(lr=0.1, is_holonomic=False)"
    assert repr(bss.GradIVAbase()) == "GradIVA(lr=0.1)" and repr(bss.GradFDICAbase()) == "GradFDICA(lr=0.1)"
    assert repr(bss.FDICAbase()) == "FDICA()"
    m = c["GradLaplaceIVA"]()
    assert (m.lr, m.reference_id, m.callbacks, m.apply_projection_back, m.recordable_loss, m.eps, m.loss, m.input) == \
        (0.1, 0, None, True, True, 1e-12, [], None)
    m = c["NaturalGradLaplaceFDICA"](0.3, 1, True, print, False, 1e-9)
    assert (m.lr, m.reference_id, m.is_holonomic, m.callbacks, m.recordable_loss, m.eps, m.loss, m.criterion) == \
        (0.3, 1, True, [print], False, 1e-9, None, None)
    assert issubclass(c["GradLaplaceIVA"], bss.GradIVAbase) and issubclass(bss.GradIVAbase, IVAbase)
    assert issubclass(c["NaturalGradLaplaceFDICA"], bss.GradFDICAbase) and issubclass(bss.GradFDICAbase, bss.FDICAbase)
    assert not hasattr(c["GradLaplaceFDICA"](), "apply_projection_back")
    for base in (bss.GradIVAbase, bss.GradFDICAbase, bss.FDICAbase):
        with pytest.raises(NotImplementedError):
            base().update_once()
        with pytest.raises(NotImplementedError):
            base().compute_negative_loglikelihood()
    assert set(gb.CLASSES) | {"GradIVAbase", "FDICAbase", "GradFDICAbase"} <= set(bss.__all__)


def test_loop_rule():
    """A fresh model takes the one-call loop; callbacks, an overridden step or a plain loss list keep the Python loop."""
    from audio_source_separation_amd import bss
    for name, new in classes().items():
        assert "_OWN_STEPS" in vars(new) and "update_once" in new._OWN_STEPS
        assert new()._fast_loop_ok() and new(recordable_loss=False)._fast_loop_ok()
        assert not new(callbacks=lambda m: None)._fast_loop_ok()

        class Stepped(new):
            def update_once(self):
                super().update_once()

        class Lossy(new):
            def compute_negative_loglikelihood(self):
                return 0.0

        class Renamed(new):
            pass

        assert not Stepped()._fast_loop_ok() and not Lossy()._fast_loop_ok() and Renamed()._fast_loop_ok()
        plain = new()
        plain.loss = []
        assert not plain._fast_loop_ok()
    assert not classes()["NaturalGradLaplaceFDICA"](is_holonomic=False)._fast_loop_ok()
    assert not bss.GradIVAbase()._fast_loop_ok() and not bss.GradFDICAbase()._fast_loop_ok()


def test_generator_reproduces_the_fixtures():
    if not os.path.isdir(os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")):
        pytest.skip("the reference tree is not present")
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_gradbss.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified %d files, 0 problems" % len(NAMES) in run.stdout, run.stdout + run.stderr
