"""tIPSDTA without a GPU: the NumPy restatement (tests/tipsdta_np.py) against the reference's recorded states
(tests/golden/tipsdta/*.npz) stage by stage, sweep by sweep, one iteration at a time and over the whole run, on numpy.linalg
and on the models of the kernels' own algorithms; pi against its definition; nu = 1e30 against the Gauss restatement bit for
bit; three planted faults of the step order and of pi that the fixtures must see; the C-ABI names, the workspace query and
the host-side refusals."""
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
import ipsdta_np as ip  # noqa: E402
import tipsdta_np as tp  # noqa: E402

FILES = tp.fixture_files()
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ENTRY_POINTS = ("workspace_bytes", "update_basis", "update_activation", "update_source", "update_spatial", "loss", "iterate")
LAS = (ip.LAPACK, ip.KERNEL)
LEVELS = {"one_stage": {"W", "U", "H", "loss", "out"}, "one_iteration": {"W", "U", "H", "loss"},
          "whole_run": {"W", "U", "H", "loss", "out"}}
def load(name):
    return np.load(os.path.join(tp.GOLDEN, name + ".npz"))


def reference_src():
    src = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")  # the default of tests/golden/make_golden.py
    if not os.path.isdir(os.path.join(src, "bss")):
        pytest.skip("the reference tree is not on this machine")


def setup(fx):
    return fx["X"], float(fx["eps"]), bool(fx["normalize"]), float(fx["nu"]), ip.dims(fx)


def model_figures(got, want):
    return {"W": ip.w_metric(got[0], want[0]), "U": ip.basis_metric(got[1], want[1]), "H": ip.h_metric(got[2], want[2])}


def test_fixtures_and_tolerances_are_complete():
    tol = tp.tolerances()
    assert len(NAMES) == 16 and tol["factor"] == 16 and sorted(tol["measured"]) == NAMES
    for level, metrics in LEVELS.items():
        assert set(tol[level]) == metrics
        for m in metrics:  # 16 x the largest measured figure, at least 16 x 2^-52
            worst = max(tol["measured"][n][level][m] for n in NAMES)
            assert tol[level][m] == 16 * max(worst, 2.0 ** -52), (level, m)
    assert max(tol["one_stage"].values()) <= 1e-9
    shapes, seeds = set(), set()
    for f in FILES:
        assert os.path.getsize(f) < 1 << 20, f  # the repository's cap per committed file
        fx = np.load(f)
        M, F, T, K, nblk, sp = ip.dims(fx)
        nn, nlow, rem = ip.geometry(F, nblk)
        shapes.add((M, F, T, K, nblk, sp, bool(fx["normalize"]), float(fx["nu"])))
        seeds.add(int(fx["seed"]))
        tags = ["0", "src1"] + ["sw1_%d" % (s + 1) for s in range(sp)] + [str(i) for i in ip.SNAP_ITERS]
        for tag in tags:
            W, U, H = ip.state(fx, tag)
            assert W.shape == (F, M, M) and H.shape == (M, K, T), (f, tag)
            if rem:
                assert U[0].shape == (M, nlow, nn, nn, K) and U[1].shape == (M, rem, nn + 1, nn + 1, K), (f, tag)
            else:
                assert U.shape == (M, nblk, nn, nn, K), (f, tag)
        assert fx["loss"].shape == (ip.N_ITER + 1,) and fx["out"].shape == (M, F, T)
        assert fx["rng_next"].shape == () and fx["seed"].shape == () and fx["eps"] > 0 and fx["nu"] > 0
        assert all(np.isfinite(fx[k]).all() for k in fx.files if k != "versions")
        assert np.all(np.diff(fx["loss"]) <= 1e-9 * (np.abs(fx["loss"][:-1]) + M * F * T))  # MM and VCD do not go up
    # the case table lives in tests/golden/tipsdta/make_tipsdta.py; a file's name spells its row
    for M, F, T, K, nblk, sp, norm, nu in shapes:
        tail = ("" if norm else "_nonorm") + ("" if nu == 1 else "_nu%g" % nu)
        assert "tipsdta_m%d_f%d_t%d_k%d_b%d_s%d%s" % (M, F, T, K, nblk, sp, tail) in NAMES
    assert len(shapes) == 16 and {nu for *_, nu in shapes} == {0.5, 1.0, 4.0, 1000.0}
    assert seeds == set(range(2700, 2716))  # no case needed another seed


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_stage_by_stage(name, la):
    fx = load(name)
    tol = tp.tolerances()["one_stage"]
    X, eps, norm, nu, (M, F, T, K, nblk, sp) = setup(fx)
    W, U, H = ip.state(fx, 0)
    kept = (W.copy(), ip.pack(U), H.copy(), X.copy())
    Un, Hn = tp.update_source(X, W, U, H, eps, nblk, nu, norm, la)
    assert all(np.array_equal(a, b) for a, b in zip((W, ip.pack(U), H, X), kept))  # the inputs are left alone
    want = ip.state(fx, "src1")
    assert ip.basis_metric(Un, want[1]) <= tol["U"] and ip.h_metric(Hn, want[2]) <= tol["H"]
    Ws = tp.update_spatial(X, want[0], want[1], want[2], eps, nblk, nu, sp, la, each=True)
    for s in range(sp):  # each sweep from the recorded state before it, and the chain from the first
        a = "src1" if s == 0 else "sw1_%d" % s
        Wa, Ua, Ha = ip.state(fx, a)
        assert ip.w_metric(tp.update_spatial(X, Wa, Ua, Ha, eps, nblk, nu, 1, la), fx["W_sw1_%d" % (s + 1)]) <= tol["W"], s
        assert ip.w_metric(Ws[s], fx["W_sw1_%d" % (s + 1)]) <= tp.tolerances()["one_iteration"]["W"], s
    for it in (0,) + ip.SNAP_ITERS:
        assert ip.loss_metric(tp.loss(X, *ip.state(fx, it), eps, nblk, nu, la), fx["loss"][it], M, F, T) <= tol["loss"], it
    assert ip.out_metric(ip.projection_back_output(X, fx["W_10"]), fx["out"]) <= tol["out"]


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_one_iteration_at_a_time(name, la):
    fx = load(name)
    tol = tp.tolerances()["one_iteration"]
    X, eps, norm, nu, (M, F, T, K, nblk, sp) = setup(fx)
    for it in ip.START_ITERS:
        W, U, H = ip.state(fx, it)
        Wn, Un, Hn, loss = tp.iterate(X, W, U, H, eps, nblk, nu, sp, norm, la)
        figures = model_figures((Wn, Un, Hn), ip.state(fx, it + 1))
        figures["loss"] = ip.loss_metric(loss, fx["loss"][it + 1], M, F, T)
        for k, v in figures.items():
            assert v <= tol[k], (it, k, v, tol[k])


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_over_the_whole_run(name, la):
    fx = load(name)
    tol = tp.tolerances()["whole_run"]
    X, eps, norm, nu, (M, F, T, K, nblk, sp) = setup(fx)
    W, U, H = ip.state(fx, 0)
    losses = []
    for _ in range(ip.N_ITER):
        W, U, H, loss = tp.iterate(X, W, U, H, eps, nblk, nu, sp, norm, la)
        losses.append(loss)
    figures = model_figures((W, U, H), ip.state(fx, ip.N_ITER))
    figures["loss"] = ip.loss_metric(np.array(losses), fx["loss"][1:], M, F, T)
    figures["out"] = ip.out_metric(ip.projection_back_output(X, W), fx["out"])
    for k, v in figures.items():
        assert v <= tol[k], (k, v, tol[k])


@pytest.mark.parametrize("name", NAMES[:4] + NAMES[-3:])
def test_pi_against_its_definition(name):
    """pi[n,t] = (nu + 2 F) / (nu + 2 sum over ALL bins of conj(y_f) (Ri y)_f), matrix by matrix with numpy.linalg alone."""
    fx = load(name)
    X, eps, norm, nu, (M, F, T, K, nblk, sp) = setup(fx)
    W, U, H = ip.state(fx, 4)
    Y = np.einsum("fnc,cft->nft", W, X)
    total = np.zeros((M, T))
    for (f0, n, nb), Up in zip(ip.part_ranges(F, nblk), ip.to_parts(U)):
        for src in range(M):
            for t in range(T):
                for b in range(n):
                    R = sum(H[src, k, t] * Up[src, k, b] for k in range(K))
                    R = ip.to_psd(R, eps)
                    Ri = ip.to_psd(np.linalg.inv(R), eps)
                    y = Y[src, f0 + b * nb:f0 + (b + 1) * nb, t]
                    total[src, t] += (np.conj(y) @ Ri @ y).real
    want = (nu + 2 * F) / (nu + 2 * total)
    for la in LAS:
        got = tp.pi(X, W, U, H, eps, nblk, nu, la)
        assert got.shape == (M, T) and np.max(np.abs(got - want) / want) <= 1e-10, la.__name__
    assert np.all(want > 0)
    if nu <= 4:  # a weight that does vary over the frames
        assert np.std(want) > 0.01 * np.mean(want)


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", ["tipsdta_m2_f9_t64_k2_b4_s2", "tipsdta_m2_f12_t64_k2_b3_s2_nonorm",
                                  "tipsdta_m3_f11_t96_k3_b3_s2"])
def test_huge_nu_is_the_gauss_restatement_bit_for_bit(name, la):
    """nu = 1e30 swallows 2 F and 2 q: pi is exactly 1.0, and W, U, H follow the Gauss restatement bit for bit."""
    fx = load(name)
    X, eps, norm, _, (M, F, T, K, nblk, sp) = setup(fx)
    W, U, H = ip.state(fx, 1)
    assert np.array_equal(tp.pi(X, W, U, H, eps, nblk, 1e30, la), np.ones((M, T)))
    Wt, Ut, Ht, _ = tp.iterate(X, W, U, H, eps, nblk, 1e30, sp, norm, la)
    Wg, Ug, Hg, _ = ip.iterate(X, W, U, H, eps, nblk, sp, norm, la)
    assert np.array_equal(Wt, Wg) and np.array_equal(ip.pack(Ut), ip.pack(Ug)) and np.array_equal(Ht, Hg)


@pytest.mark.parametrize("fault", tp.FAULTS)
def test_planted_faults_exceed_the_one_sweep_tolerance(fault):
    """pi once per source, pi from the stepped block alone, the high group before the low one: each must move W of one
    sweep past the tolerance on at least one fixture with remains, or the fixtures cannot see what the Student-t model
    changes."""
    tol = tp.tolerances()["one_stage"]["W"]
    seen = []
    for name in NAMES:
        fx = load(name)
        X, eps, norm, nu, (M, F, T, K, nblk, sp) = setup(fx)
        if F % nblk == 0:
            continue
        W, U, H = ip.state(fx, "src1")
        good = ip.w_metric(tp.update_spatial(X, W, U, H, eps, nblk, nu, 1), fx["W_sw1_1"])
        bad = ip.w_metric(tp.update_spatial(X, W, U, H, eps, nblk, nu, 1, fault=fault), fx["W_sw1_1"])
        assert good <= tol
        seen.append((name, bad))
    print(fault, tol, seen)
    assert len(seen) >= 5 and max(b for _, b in seen) > tol, (fault, seen)


def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "assx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_tipsdta_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted("assx_tipsdta_" + n for n in ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_tipsdta_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    # each entry point has its Gauss twin's argument list plus one double
    for n in ENTRY_POINTS:
        g, t = _lib.SIGNATURES["assx_ipsdta_" + n], _lib.SIGNATURES["assx_tipsdta_" + n]
        assert t[0] is g[0] and len(t[1]) == len(g[1]) + 1
        extra = list(t[1])
        extra.remove(ctypes.c_double)
        assert extra == list(g[1]), n
    # the Engine wrappers next to the Gauss ones
    from audio_source_separation_amd.ops import Engine
    for n in ("workspace",) + ENTRY_POINTS[1:]:
        assert callable(getattr(Engine, "tipsdta_" + n)) and callable(getattr(Engine, "ipsdta_" + n))


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_tipsdta_workspace_bytes

    def documented(M, F, T, K, nblk):
        nn, nlow, rem = ip.geometry(F, nblk)
        P = nlow * nn * nn + rem * (nn + 1) ** 2
        return 16 * (2 * M * P * T + 2 * M * K * P) + 8 * (2 * M * nblk * T + M * T)

    for case in ((2, 9, 64, 2, 4), (2, 513, 256, 10, 128), (2, 513, 256, 10, 512), (8, 16, 33, 64, 2), (2, 1025, 100, 10, 1024),
                 (3, 8, 1, 1, 8), (2, 8, 5, 1, 1)):
        for nu in (1.0, 0.5, 1e30):
            assert q(*case, _lib.F64, nu) == documented(*case), case
    for M, F, T, K, nblk, dt in ((1, 16, 33, 3, 4, _lib.F64), (9, 16, 33, 3, 4, _lib.F64), (2, 16, 33, 0, 4, _lib.F64),
                                 (2, 16, 33, 65, 4, _lib.F64), (2, 16, 33, 3, 0, _lib.F64), (2, 16, 33, 3, 17, _lib.F64),
                                 (2, 16, 33, 3, 1, _lib.F64), (2, 17, 33, 3, 2, _lib.F64), (2, 16, 0, 3, 4, _lib.F64),
                                 (2, 0, 33, 3, 1, _lib.F64), (2, 16, 33, 3, 4, _lib.F32), (2, 513, 256, 10, 1024, _lib.F64)):
        assert q(M, F, T, K, nblk, dt, 1.0) == 0, (M, F, T, K, nblk, dt)
    for nu in (0.0, -1.0, float("inf"), float("nan")):  # what the entry points' argument check refuses
        assert q(2, 16, 33, 3, 4, _lib.F64, nu) == 0, nu
    assert q(8, 8192, 4000, 64, 1024, _lib.F64, 1.0) > 2 ** 32  # sizes in 64-bit arithmetic


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    dims = (2, 9, 64, 2, 4, _lib.F64, null)
    assert L.assx_tipsdta_update_basis(null, null, null, null, null, 1e-12, 1.0, null, null, *dims) == E_NULL
    assert L.assx_tipsdta_update_activation(null, null, null, null, null, 1e-12, 1.0, null, null, *dims) == E_NULL
    assert L.assx_tipsdta_update_source(null, null, null, null, null, 1e-12, 1.0, 1, null, null, *dims) == E_NULL
    assert L.assx_tipsdta_update_spatial(null, 1, null, null, null, null, 1e-12, 1.0, null, null, *dims) == E_NULL
    assert L.assx_tipsdta_loss(null, null, null, null, null, 1e-12, 1.0, null, null, null, *dims) == E_NULL
    assert L.assx_tipsdta_iterate(null, 1, 1, null, null, null, null, 1e-12, 1.0, 1, null, null, null, *dims) == E_NULL


def test_class_refusals_touch_neither_a_device_nor_the_rng():
    from audio_source_separation_amd.bss import GaussIPSDTA, IPSDTAbase, tIPSDTA
    fx = load("tipsdta_m2_f9_t64_k2_b4_s2")
    X = fx["X"]
    M, F, T = X.shape
    assert issubclass(tIPSDTA, IPSDTAbase) and not issubclass(tIPSDTA, GaussIPSDTA)
    for author in ('Ikeshita', 'nobody'):  # the reference's tIPSDTA knows Kondo alone
        with pytest.raises(ValueError, match="Not support"):
            tIPSDTA(author=author)
    with pytest.raises(ValueError, match="Invalid keywords"):
        tIPSDTA(n_neighbors=2)
    with pytest.raises(ValueError, match="float64"):
        tIPSDTA(dtype='float32')
    G = tIPSDTA
    nb = dict(n_blocks=4)
    refused = [(G(), X, "n_blocks"), (G(n_blocks=1), X, "blocks of at most 8"), (G(n_basis=65, **nb), X, "n_basis"),
               (G(**nb), np.tile(X, (5, 1, 1))[:9], "n_channels"), (G(**nb), X.real, "complex"),
               (G(nu=0, **nb), X, "nu"), (G(nu=-1.0, **nb), X, "nu"), (G(nu=float("inf"), **nb), X, "nu"),
               (G(nu=float("nan"), **nb), X, "nu"), (G(nu="1", **nb), X, "nu")]
    for model, inp, what in refused:
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match=what):
            model(inp, iteration=1)
        assert model._engine is None and np.array_equal(np.random.get_state()[1], state)
        assert model.loss == [] and not hasattr(model, "basis") and not hasattr(model, "activation")
        assert not hasattr(model, "demix_filter")
    model = G(**nb)
    model.author = 'Ikeshita'
    with pytest.raises(ValueError, match="Not support"):
        model(X, iteration=1)
    # the signature and the keyword handling of the reference
    import inspect
    sig = inspect.signature(tIPSDTA.__init__)
    assert list(sig.parameters)[1:10] == ["n_basis", "nu", "spatial_iteration", "normalize", "callbacks", "reference_id",
                                          "author", "recordable_loss", "eps"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:10]] == [10, 1, None, True, None, 0, 'Kondo', True, 1e-12]
    model = G(n_basis=4, nu=2.5, spatial_iteration=3, n_blocks=7)
    assert (model.n_basis, model.nu, model.spatial_iteration, model.n_blocks, model.normalize, model.eps, model.loss) == \
        (4, 2.5, 10, 7, True, 1e-12, [])
    assert (model.algorithm_source, model.algorithm_spatial, model.author, model.reference_id) == ('mm', 'vcd', 'Kondo', 0)
    assert repr(model) == "t-IPSDTA(n_basis=4, nu=2.5, normalize=True, algorithm(source)=mm, algorithm(spatial)=vcd, " \
                          "n_blocks=7, author=Kondo)"
    assert G(recordable_loss=False).loss is None and G().n_blocks == 1024 and G().nu == 1
    # GaussIPSDTA keeps its own name, refusals and entry points
    assert repr(GaussIPSDTA(n_blocks=7)).startswith("Gauss-IPSDTA(") and GaussIPSDTA._OPS == "ipsdta_" and G._OPS == "tipsdta_"
    with pytest.raises(NotImplementedError, match="Ikeshita"):
        GaussIPSDTA(author='Ikeshita')


def test_generator_reproduces_the_fixtures():
    reference_src()
    run = subprocess.run([sys.executable, os.path.join(tp.GOLDEN, "make_tipsdta.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified 16 files, 0 problems" in run.stdout, run.stdout + run.stderr
