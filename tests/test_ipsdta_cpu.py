"""GaussIPSDTA without a GPU: the NumPy restatement (tests/ipsdta_np.py) against the reference's recorded states
(tests/golden/ipsdta/*.npz) stage by stage, one iteration at a time and over the whole run, on numpy.linalg and on the
models of the kernels' own algorithms; psd against its definition; the Jacobi and Cholesky models against numpy.linalg;
the C-ABI names, the workspace query and the host-side refusals."""
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

FILES = ip.fixture_files()
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ENTRY_POINTS = ("workspace_bytes", "to_psd", "update_basis", "update_activation", "normalize", "update_source",
                "update_spatial", "loss", "iterate")
LAS = (ip.LAPACK, ip.KERNEL)
LEVELS = {"one_stage": {"W", "U", "H", "loss", "out"}, "one_iteration": {"W", "U", "H", "loss"},
          "whole_run": {"W", "U", "H", "loss", "out"}}
CSRC = os.path.join(ROOT, "audio_source_separation_amd", "csrc")


def load(name):
    return np.load(os.path.join(ip.GOLDEN, name + ".npz"))


def reference_src():
    src = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")  # the default of tests/golden/make_golden.py
    if not os.path.isdir(os.path.join(src, "bss")):
        pytest.skip("the reference tree is not on this machine")


def setup(fx):
    return fx["X"], float(fx["eps"]), bool(fx["normalize"]), ip.dims(fx)


def model_figures(got, want):
    return {"W": ip.w_metric(got[0], want[0]), "U": ip.basis_metric(got[1], want[1]), "H": ip.h_metric(got[2], want[2])}


def test_fixtures_and_tolerances_are_complete():
    tol = ip.tolerances()
    assert len(NAMES) == 15 and tol["factor"] == 16 and sorted(tol["measured"]) == NAMES
    for level, metrics in LEVELS.items():
        assert set(tol[level]) == metrics
        for m in metrics:  # 16 x the largest measured figure, at least 16 x 2^-52
            worst = max(tol["measured"][n][level][m] for n in NAMES)
            assert tol[level][m] == 16 * max(worst, 2.0 ** -52), (level, m)
    assert max(tol["one_stage"].values()) <= 1e-9
    shapes = set()
    for f in FILES:
        assert os.path.getsize(f) < 1 << 20, f  # the repository's cap per committed file
        fx = np.load(f)
        M, F, T, K, nblk, sp = ip.dims(fx)
        nn, nlow, rem = ip.geometry(F, nblk)
        shapes.add((M, F, T, K, nblk, sp, bool(fx["normalize"])))
        tags = ["0", "src1"] + ["sw1_%d" % (s + 1) for s in range(sp)] + [str(i) for i in ip.SNAP_ITERS]
        for tag in tags:
            W, U, H = ip.state(fx, tag)
            assert W.shape == (F, M, M) and H.shape == (M, K, T), (f, tag)
            if rem:
                assert U[0].shape == (M, nlow, nn, nn, K) and U[1].shape == (M, rem, nn + 1, nn + 1, K), (f, tag)
            else:
                assert U.shape == (M, nblk, nn, nn, K), (f, tag)
            assert ip.pack(U).shape == (M, K, nlow * nn * nn + rem * (nn + 1) ** 2)
        assert fx["loss"].shape == (ip.N_ITER + 1,) and fx["out"].shape == (M, F, T)
        assert fx["rng_next"].shape == () and fx["seed"].shape == () and fx["eps"] > 0
        assert all(np.isfinite(fx[k]).all() for k in fx.files if k != "versions")
        assert np.all(np.diff(fx["loss"]) <= 1e-9 * (np.abs(fx["loss"][:-1]) + M * F * T))  # MM and VCD do not go up
    assert shapes == {(2, 9, 64, 2, 4, 2, True), (2, 5, 64, 2, 4, 2, True), (3, 11, 96, 3, 3, 2, True),
                      (4, 13, 96, 2, 5, 2, True), (2, 16, 128, 2, 2, 2, True), (2, 15, 128, 2, 2, 2, True),
                      (2, 6, 64, 2, 1, 2, True), (2, 8, 128, 10, 2, 2, True), (2, 6, 64, 2, 6, 2, True),
                      (2, 4, 257, 2, 2, 2, True), (2, 12, 64, 2, 3, 10, True), (2, 12, 64, 2, 3, 2, False),
                      (2, 12, 64, 1, 3, 2, True), (8, 6, 160, 2, 3, 2, True), (2, 6, 48, 64, 3, 2, True)}


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_stage_by_stage(name, la):
    fx = load(name)
    tol = ip.tolerances()["one_stage"]
    X, eps, norm, (M, F, T, K, nblk, sp) = setup(fx)
    W, U, H = ip.state(fx, 0)
    kept = (W.copy(), ip.pack(U), H.copy(), X.copy())
    Un, Hn = ip.update_source(X, W, U, H, eps, nblk, norm, la)
    assert all(np.array_equal(a, b) for a, b in zip((W, ip.pack(U), H, X), kept))  # the inputs are left alone
    want = ip.state(fx, "src1")
    assert ip.basis_metric(Un, want[1]) <= tol["U"] and ip.h_metric(Hn, want[2]) <= tol["H"]
    Ws = ip.update_spatial(X, want[0], want[1], want[2], eps, nblk, sp, la, each=True)
    for s in range(sp):  # each sweep from the recorded state before it, and the chain from the first
        a = "src1" if s == 0 else "sw1_%d" % s
        Wa, Ua, Ha = ip.state(fx, a)
        assert ip.w_metric(ip.update_spatial(X, Wa, Ua, Ha, eps, nblk, 1, la), fx["W_sw1_%d" % (s + 1)]) <= tol["W"], s
        assert ip.w_metric(Ws[s], fx["W_sw1_%d" % (s + 1)]) <= ip.tolerances()["one_iteration"]["W"], s
    for it in (0,) + ip.SNAP_ITERS:
        assert ip.loss_metric(ip.loss(X, *ip.state(fx, it), eps, nblk, la), fx["loss"][it], M, F, T) <= tol["loss"], it
    assert ip.out_metric(ip.projection_back_output(X, fx["W_10"]), fx["out"]) <= tol["out"]


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_one_iteration_at_a_time(name, la):
    fx = load(name)
    tol = ip.tolerances()["one_iteration"]
    X, eps, norm, (M, F, T, K, nblk, sp) = setup(fx)
    for it in ip.START_ITERS:
        W, U, H = ip.state(fx, it)
        Wn, Un, Hn, loss = ip.iterate(X, W, U, H, eps, nblk, sp, norm, la)
        figures = model_figures((Wn, Un, Hn), ip.state(fx, it + 1))
        figures["loss"] = ip.loss_metric(loss, fx["loss"][it + 1], M, F, T)
        for k, v in figures.items():
            assert v <= tol[k], (it, k, v, tol[k])


@pytest.mark.parametrize("la", LAS, ids=lambda la: la.__name__)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_over_the_whole_run(name, la):
    fx = load(name)
    tol = ip.tolerances()["whole_run"]
    X, eps, norm, (M, F, T, K, nblk, sp) = setup(fx)
    W, U, H = ip.state(fx, 0)
    losses = []
    for _ in range(ip.N_ITER):
        W, U, H, loss = ip.iterate(X, W, U, H, eps, nblk, sp, norm, la)
        losses.append(loss)
    figures = model_figures((W, U, H), ip.state(fx, ip.N_ITER))
    figures["loss"] = ip.loss_metric(np.array(losses), fx["loss"][1:], M, F, T)
    figures["out"] = ip.out_metric(ip.projection_back_output(X, W), fx["out"])
    for k, v in figures.items():
        assert v <= tol[k], (k, v, tol[k])


def test_start_state_is_the_draws_after_the_reset():
    """The low draws, then the high draws, then the activation; real diagonals in complex storage; identity W."""
    for name in NAMES:
        fx = load(name)
        M, F, T, K, nblk, sp = ip.dims(fx)
        nn, nlow, rem = ip.geometry(F, nblk)
        np.random.seed(int(fx["seed"]))
        draws = [np.random.rand(M, K, n, nb) for _, n, nb in ip.part_ranges(F, nblk)]
        H = np.random.rand(M, K, T)
        assert np.random.rand() == float(fx["rng_next"])
        keys = ("draw_Ul", "draw_Uh") if rem else ("draw_U",)
        assert all(np.array_equal(d, fx[k]) for d, k in zip(draws, keys)) and np.array_equal(H, fx["draw_H"])
        U = ip.from_parts([(d[..., None] * np.eye(d.shape[-1])).astype(np.complex128) for d in draws], F, nblk)
        W0, U0, H0 = ip.state(fx, 0)
        assert np.array_equal(W0, np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1)))
        assert all(p.dtype == np.complex128 and not p.imag.any() for p in ip.to_parts(U0))
        if fx["normalize"]:
            U, H = ip.normalize(U, H, F, nblk)
            assert ip.basis_metric(U, U0) <= (F + 1) * 2.0 ** -52 and ip.h_metric(H, H0) <= (F + 1) * 2.0 ** -52
        else:
            assert np.array_equal(ip.pack(U), ip.pack(U0)) and np.array_equal(H, H0)


@pytest.mark.parametrize("n", range(1, 9))
def test_to_psd_against_its_definition(n):
    eps = 1e-3  # large enough for the eps trace term to be visible in every entry of the diagonal
    for kind, A in ip.psd_cases(n, 40 + n):
        A = A + 0.01 / n * np.triu(np.ones((n, n)), 1)  # not Hermitian: psd takes the Hermitian part
        S = (A + ip.ct(A)) / 2
        lam = np.linalg.eigvalsh(S)
        want = (S - np.minimum(lam[:, 0], 0)[:, None, None] * np.eye(n)) \
            + eps * np.trace(S, axis1=1, axis2=2).real[:, None, None] * np.eye(n)
        if kind == "indefinite":
            assert (lam[:, 0] < -0.5).all()
        if kind == "definite":
            assert (lam[:, 0] > 0.25).all()
        for la in LAS:
            got = ip.to_psd(A, eps, la)
            assert np.array_equal(got, ip.ct(got))
            assert ip.mat_metric(got, want) <= 64 * n * 2.0 ** -52, (kind, la.__name__)
    # a rank-one x x^H: lambda_min is rounding noise of either sign, at most n 2^-52 of the trace; taking it as 0 costs that
    kind, A = ip.psd_cases(n, 40 + n)[2]
    tr = np.trace(A, axis1=1, axis2=2).real
    assert np.all(np.abs(np.linalg.eigvalsh(A)[:, 0]) <= 8 * n * 2.0 ** -52 * tr) or n == 1
    diff = np.abs(ip.to_psd(A, eps, shift=False) - ip.to_psd(A, eps))
    assert np.all(np.max(diff, axis=(1, 2)) <= 8 * n * 2.0 ** -52 * tr)


@pytest.mark.parametrize("n", range(1, 9))
def test_jacobi_and_cholesky_models_against_lapack(n):
    for kind, A in ip.psd_cases(n, 70 + n):
        w, U = ip.jacobi_eigh(A)
        scale = np.max(np.abs(np.linalg.eigvalsh(A)), axis=1, keepdims=True)
        # eigenvalues to a few ulps of the spectral radius, vectors orthonormal, the decomposition reproduces A
        assert np.max(np.abs(np.sort(w, axis=1) - np.linalg.eigvalsh(A)) / scale) <= 16 * n * 2.0 ** -52, kind
        assert np.max(np.abs(ip.ct(U) @ U - np.eye(n))) <= 16 * n * 2.0 ** -52, kind
        assert ip.mat_metric((U * w[:, None, :]) @ ip.ct(U), A) <= 16 * n * 2.0 ** -52, kind
        if kind == "definite":
            # cond <= 3: the inverse and the root to n ulps times the condition number
            assert ip.mat_metric(ip.chol_inverse(A), np.linalg.inv(A)) <= 64 * n * 2.0 ** -52
            assert ip.mat_metric(ip.KERNEL.sqrtm(A), ip.LAPACK.sqrtm(A)) <= 64 * n * 2.0 ** -52
            assert np.array_equal(ip.KERNEL.min_eig(A), np.zeros(len(A)))  # the Cholesky shortcut
        if kind == "indefinite":
            with pytest.raises(np.linalg.LinAlgError):
                ip.chol_inverse(A)
            assert np.array_equal(ip.KERNEL.min_eig(A) < -0.5, np.ones(len(A), dtype=bool))


def test_vcd_weight_branches():
    eps = 1e-12
    eta = np.array([2.0 + 0.5j, 1e-15, 2.0 + 0.5j, 0.7 - 0.1j])
    eta_hat = np.array([0.0, 0.0, 0.3 - 0.4j, 1e-13 + 0j])
    w, ip_branch = ip.vcd_weight(eta, eta_hat, eps)
    assert ip_branch.tolist() == [True, True, False, True]
    want = [1 / np.sqrt(2.0 + 0.5j), 1 / np.sqrt(eps + 0j),
            (eta_hat[2] / (2 * eta[2])) * (1 - np.sqrt(1 + 4 * eta[2] / abs(eta_hat[2]) ** 2)), 1 / np.sqrt(0.7 - 0.1j)]
    assert np.all(np.abs(w - want) <= 4 * 2.0 ** -52 * np.abs(want))
    # the weight is the negative root of eta w^2 - eta_hat w - 1 = 0
    r, rh = 1.7, 0.6
    wr = ip.vcd_weight(np.array([r + 0j]), np.array([rh + 0j]), eps)[0][0]
    assert wr.real < 0 and abs(r * wr * wr - rh * wr - 1) <= 1e-14


def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "assx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_ipsdta_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted("assx_ipsdta_" + n for n in ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_ipsdta_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n


def test_kernels_are_part_of_the_checked_build():
    """build.sh compiles csrc/assx_ipsdta.hip for gfx950 with the other units, which puts its device assembly through
    tools/asm_wait_check.py, and links it."""
    script = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r'SRCS="\$\{ASSX_SRCS:-[^"]*\bassx_ipsdta\b', script) and "$OBJ/assx_ipsdta.o" in script


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_ipsdta_workspace_bytes

    def documented(M, F, T, K, nblk):
        nn, nlow, rem = ip.geometry(F, nblk)
        P = nlow * nn * nn + rem * (nn + 1) ** 2
        return 16 * (2 * M * P * T + 2 * M * K * P + M * F * M * M) + 8 * M * nblk * T

    for case in ((2, 9, 64, 2, 4), (2, 513, 256, 10, 128), (2, 513, 256, 10, 512), (8, 16, 33, 64, 2), (2, 1025, 100, 10, 1024),
                 (3, 8, 1, 1, 8), (2, 8, 5, 1, 1)):
        assert q(*case, _lib.F64) == documented(*case), case
    base = q(2, 16, 33, 3, 4, _lib.F64)
    assert q(3, 16, 33, 3, 4, _lib.F64) > base and q(2, 17, 33, 3, 4, _lib.F64) > base
    assert q(2, 16, 34, 3, 4, _lib.F64) > base and q(2, 16, 33, 4, 4, _lib.F64) > base
    for M, F, T, K, nblk, dt in ((1, 16, 33, 3, 4, _lib.F64), (9, 16, 33, 3, 4, _lib.F64), (2, 16, 33, 0, 4, _lib.F64),
                                 (2, 16, 33, 65, 4, _lib.F64), (2, 16, 33, 3, 0, _lib.F64), (2, 16, 33, 3, 17, _lib.F64),
                                 (2, 16, 33, 3, 1, _lib.F64), (2, 17, 33, 3, 2, _lib.F64), (2, 16, 0, 3, 4, _lib.F64),
                                 (2, 0, 33, 3, 1, _lib.F64), (2, 16, 33, 3, 4, _lib.F32), (2, 513, 256, 10, 1024, _lib.F64)):
        assert q(M, F, T, K, nblk, dt) == 0, (M, F, T, K, nblk, dt)
    assert q(8, 8192, 4000, 64, 1024, _lib.F64) > 2 ** 32  # sizes in 64-bit arithmetic


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    dims = (2, 9, 64, 2, 4, _lib.F64, null)
    assert L.assx_ipsdta_to_psd(null, null, 1, 4, 1e-12, null) == E_NULL
    assert L.assx_ipsdta_update_basis(null, null, null, null, null, 1e-12, null, null, *dims) == E_NULL
    assert L.assx_ipsdta_update_activation(null, null, null, null, null, 1e-12, null, null, *dims) == E_NULL
    assert L.assx_ipsdta_normalize(null, null, null, *dims) == E_NULL
    assert L.assx_ipsdta_update_source(null, null, null, null, null, 1e-12, 1, null, null, *dims) == E_NULL
    assert L.assx_ipsdta_update_spatial(null, 1, null, null, null, null, 1e-12, null, null, *dims) == E_NULL
    assert L.assx_ipsdta_loss(null, null, null, null, null, 1e-12, null, null, null, *dims) == E_NULL
    assert L.assx_ipsdta_iterate(null, 1, 1, null, null, null, null, 1e-12, 1, null, null, null, *dims) == E_NULL


def test_class_refusals_touch_neither_a_device_nor_the_rng():
    from audio_source_separation_amd.bss import GaussIPSDTA, IPSDTAbase
    from audio_source_separation_amd.bss.ipsdta import EPS
    fx = load("ipsdta_m2_f9_t64_k2_b4_s2")  # blocks of 2, 2, 2 and 3: the tuple layout
    X = fx["X"]
    M, F, T = X.shape
    with pytest.raises(NotImplementedError, match="Ikeshita"):
        GaussIPSDTA(author='Ikeshita')
    with pytest.raises(ValueError, match="Not support"):
        GaussIPSDTA(author='nobody')
    with pytest.raises(ValueError, match="Invalid keywords"):
        GaussIPSDTA(n_neighbors=2)
    with pytest.raises(ValueError, match="float64"):
        GaussIPSDTA(dtype='float32')
    G = GaussIPSDTA
    nb = dict(n_blocks=max(F // 4, 1))
    refused = [(G(), X, "n_blocks"), (G(n_blocks=F + 1), X, "n_blocks"), (G(n_blocks=0), X, "n_blocks"),
               (G(n_blocks=1), np.tile(X, (1, 2, 1))[:, :9], "blocks of at most 8"), (G(n_basis=0, **nb), X, "n_basis"),
               (G(n_basis=65, **nb), X, "n_basis"), (G(n_basis=2.5, **nb), X, "n_basis"), (G(**nb), X[:1], "n_channels"),
               (G(**nb), np.tile(X, (5, 1, 1))[:9], "n_channels"), (G(**nb), X.real, "complex"), (G(**nb), X[0], "dims"),
               (G(**nb), X[:, :, :0], "empty"), (G(reference_id=M, **nb), X, "reference_id")]
    for model, inp, what in refused:
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match=what):
            model(inp, iteration=1)
        assert model._engine is None and np.array_equal(np.random.get_state()[1], state)
        assert model.loss == [] and not hasattr(model, "basis") and not hasattr(model, "activation")
        assert not hasattr(model, "demix_filter")
    model = G(**nb)
    with pytest.raises(ValueError, match="spatial_iteration"):
        model(X, iteration=1, spatial_iteration=-1)
    W, U, H = ip.state(fx, 0)
    warm = [("demix_filter", W[:-1], "demix_filter"), ("activation", H[:, :, :-1], "activation"),
            ("basis", U[0], "basis"), ("basis", np.ones((M, 3, 3)), "basis")]
    for attr, value, what in warm:
        model = G(n_basis=H.shape[1], n_blocks=4)
        with pytest.raises(ValueError, match=what):
            setattr(model, attr, value)
            model(X, iteration=1)
        assert model._engine is None
    # the keyword handling of the reference: the constructor's spatial_iteration is overwritten by the default
    model = G(n_basis=4, spatial_iteration=3, n_blocks=7)
    assert (model.n_basis, model.spatial_iteration, model.n_blocks, model.normalize, model.eps, model.loss, EPS) == \
        (4, 10, 7, True, 1e-12, [], 1e-12)
    assert (model.algorithm_source, model.algorithm_spatial, model.author, model.reference_id) == ('mm', 'vcd', 'Kondo', 0)
    assert G(recordable_loss=False).loss is None and G().n_blocks == 1024 and IPSDTAbase().n_basis == 10
    assert "n_blocks=7" in repr(model) and "author=Kondo" in repr(model)
    # a basis in either layout survives the packed storage
    model.basis = U
    assert isinstance(model.basis, tuple) and all(np.array_equal(a, b) for a, b in zip(model.basis, U))
    model.basis = U[0]
    assert np.array_equal(model.basis, U[0])
    del model.basis
    assert not hasattr(model, "basis")


def test_generator_reproduces_the_fixtures():
    reference_src()
    run = subprocess.run([sys.executable, os.path.join(ip.GOLDEN, "make_ipsdta.py"), "--verify"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "verified 15 files, 0 problems" in run.stdout, run.stdout + run.stderr
