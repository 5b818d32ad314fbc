"""The beamformers, PCA and MDP without a GPU: the NumPy restatement (tests/beamform_np.py) against the reference-recorded
cases of tests/golden/beamform, planted faults that the cases must catch, the chain's insensitivity to eigenvector phases,
the C-ABI's symbol list, its workspace query and refusals, every refusal of the envelope and the three deviations of the
classes from the reference.

Tolerances: the restatement and the reference are two float64 programs that sum in different orders, so an output is held
to beamform_envelope_np.tolerance (256 x the restatement's own one-rounding sensitivity, floor 1e-13), the figures the GPU
tests use.  PCA components are compared after turning every (component, bin) row by the phase of sum_t ref conj(out);
the degenerate cases (T < M, a duplicated channel) on invariants only.
"""
import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

import beamform_np as bf  # noqa: E402
import beamform_envelope_np as benv  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "beamform")
NAMES = bf.cases(GOLDEN)
DEGENERATE = [n for n in NAMES if n.endswith(("_fewframes", "_dup"))]
REGULAR = [n for n in NAMES if n not in DEGENERATE]
ENTRY_POINTS = ("assx_bf_workspace_bytes", "assx_bf_apply", "assx_bf_ds_weights", "assx_bf_ml_weights", "assx_pca_basis",
                "assx_mdp_scale")


def load(name):
    return bf.load_case(GOLDEN, name)


def nan_distance(output, got, ref):
    """The distance of an MDP scale: NaN where the reference has NaN, and nowhere else."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    return benv.distance(output, np.where(nan, 0, got), np.where(nan, 0, ref))


def restated(g, **fault):
    """{output: distance} of the restatement from one recorded case; a fault goes to the functions that know it."""
    def pick(*names):
        return {k: v for k, v in fault.items() if k in names}

    X, A, R, Ys, ref, eps = g["X"], g["A"], g["R"], g["Ys"], int(g["reference_id"]), float(g["eps"])
    d = {"ds": benv.distance("ds", bf.delay_sum(X, A, ref, **pick("wrong_axis")), g["ds"]),
         "ml": benv.distance("ml", bf.ml(X, A, R, ref, eps, **pick("conj_filter", "wrong_axis", "floor_abs")), g["ml"]),
         "mdp": max(nan_distance("mdp", bf.mdp(Ys, X[ref], **pick("conj_wrong")), g["mdp2"]),
                    nan_distance("mdp", bf.mdp(Ys, X, **pick("conj_wrong")), g["mdp3"]))}
    if "mvdr" in g:
        d["mvdr"] = benv.distance("mvdr", bf.mvdr(X, A, ref, eps, **pick("conj_filter", "wrong_axis", "floor_abs")), g["mvdr"])
        V, w = bf.pca_basis(X, **pick("descending"))
        d["pca"] = benv.distance("pca", bf.project(X, V), g["pca"])
        d["pca_w"] = benv.distance("pca_w", w, g["pca_w"])
    return d


def test_fixtures_are_complete():
    seen = set()
    for name in NAMES:
        g = load(name)
        M, F, T = g["X"].shape
        N = g["A"].shape[2]
        tag = "" if re.fullmatch(r"t\d+", name.split("_")[-1]) else name.split("_")[-1]
        seen.add((M, N, tag))
        assert g["A"].shape == (F, M, N) and g["R"].shape == (F, M, M) and g["Ys"].shape == (N, F, T)
        assert g["ds"].shape == g["ml"].shape == (N, F, T) and g["pca"].shape == (M, F, T) and g["pca_w"].shape == (F, M)
        assert g["mdp2"].shape == (N, F) and g["mdp3"].shape == (M, N, F)
        assert not np.allclose(g["R"], g["R"].conj().transpose(0, 2, 1))  # ML gets a non-Hermitian covariance
        assert ("mvdr" in g) == (name in REGULAR)
        if name in REGULAR:  # the condition for comparing PCA component by component
            assert T >= 4 * M and bf.eigen_gap(g["X"]) >= 1e-3
        else:
            assert T < M or np.array_equal(g["X"][M - 1], g["X"][0])
        assert g["floored"].any() == (tag == "floor") and np.isnan(g["mdp2"]).any() == (tag == "silent")
        parts = [name + ".npz"] + ["%s.part%d.npz" % (name, i) for i in range(1, int(g["n_parts"]))]
        assert all(os.path.getsize(os.path.join(GOLDEN, p)) < 150 * 1024 for p in parts)
    assert len([f for f in os.listdir(GOLDEN) if f.endswith(".npz")]) == sum(int(load(n)["n_parts"]) for n in NAMES)
    plain = {(M, N) for M, N, tag in seen if not tag}
    assert {M for M, _ in plain} == set(range(2, 9))
    assert any(N < M for M, N in plain) and any(N == M for M, N in plain) and any(N > M for M, N in plain)
    assert any(int(load(n)["reference_id"]) != 0 for n in NAMES)
    assert {"floor", "silent", "fewframes", "dup", "chain"} <= {tag for _, _, tag in seen}
    assert len(DEGENERATE) == 2  # no more invariants-only cases than the two built for that purpose


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = load(name)
    for k, v in restated(g).items():
        assert v <= benv.tolerance(k), (k, v, benv.tolerance(k))
    if "chain" in g:
        assert benv.distance("chain", bf.chain(g["X"]), g["chain"]) <= benv.tolerance("chain")


def pca_invariants(X, V, w, out, tol):
    """V unitary; out is X projected on V; the component powers are the eigenvalues, ascending; the eigenvalues are those
    of the covariance.  Everything is measured against the bin's largest component: a component of a null eigenvalue is
    rounding noise and has no digits of its own."""
    M, F, T = X.shape
    eye = np.broadcast_to(np.eye(M), (F, M, M))
    assert np.abs(V.conj().transpose(0, 2, 1) @ V - eye).max() <= tol
    assert benv.entrywise("basis", out.transpose(1, 0, 2), bf.project(X, V).transpose(1, 0, 2)) <= tol
    scale = np.maximum(w[:, -1:], 1e-300)
    assert np.all(np.diff(w, axis=1) >= -tol * scale)
    assert np.abs(np.mean(np.abs(out) ** 2, axis=2).T - w).max() <= tol * scale.max()
    assert np.abs(w - np.linalg.eigvalsh(bf.covariance(X))).max() <= tol * scale.max()


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_pca_on_invariants(name):
    """T < M and a duplicated channel: eigenvalues coincide, so components are no functions of the input; the
    restatement's basis and the reference's recorded output are held to what does not depend on the choice."""
    g = load(name)
    X = g["X"]
    V, w = bf.pca_basis(X)
    tol = benv.tolerance("pca_V")
    pca_invariants(X, V, w, bf.project(X, V), tol)
    assert benv.distance("pca_w", w, g["pca_w"]) <= benv.tolerance("pca_w")
    power = np.mean(np.abs(g["pca"]) ** 2, axis=2).T
    assert np.abs(power - w).max() <= tol * w.max()


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault,outputs", [("conj_filter", ("ml", "mvdr")), ("wrong_axis", ("ds", "ml", "mvdr")),
                                           ("descending", ("pca", "pca_w")), ("conj_wrong", ("mdp",)),
                                           ("floor_abs", ("ml",))])
def test_fixtures_catch_a_planted_fault(fault, outputs):
    """The ML filter conjugated; A[f,ref,n] taken from the wrong axis; eigenvalues descending; the MDP conjugate on the
    wrong factor; the floor applied to |den| instead of NumPy's complex order (seen where a denominator is floored)."""
    caught = []
    for name in REGULAR:
        d = restated(load(name), **{fault: True})
        assert all(v <= benv.tolerance(k) for k, v in d.items() if k not in outputs), (name, d)
        if any(d[k] > 1e6 * benv.tolerance(k) for k in outputs if k in d):
            caught.append(name)
    need = [n for n in REGULAR if n.endswith("_floor")] if fault == "floor_abs" else REGULAR
    assert set(need) <= set(caught), (fault, caught)


def test_floor_follows_numpys_complex_order():
    eps = 1e-12
    den = np.array([1e-13 + 5j, 1e-12 - 1e-30j, 1e-12 + 0j, 1e-12 + 1j, -3.0 + 0j, 2e-12 - 9j, 0.5 + 0j])
    want = np.array([True, True, False, False, True, False, False])
    got, below = bf.floored(den, eps)
    assert np.array_equal(below, want) and np.array_equal(below, den < eps)
    assert np.array_equal(got, np.where(want, eps, den))


def test_chain_does_not_depend_on_eigenvector_phases():
    """pca(x)[:2] -> AuxLaplaceIVA -> projection back: a unit factor on every (component, bin) of the PCA output leaves
    the projected-back estimate where it is."""
    g = load([n for n in NAMES if n.endswith("_chain")][0])
    X = g["X"]
    rng = np.random.default_rng(3)
    for _ in range(3):
        phases = np.exp(2j * np.pi * rng.random(X.shape[:2]))
        d = benv.distance("chain", bf.chain(X, phases=phases), g["chain"])
        print("chain under random phases: %.1e" % d)
        assert d <= benv.tolerance("chain")


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "assx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_(?:bf|pca|mdp)_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith(("assx_bf_", "assx_pca_", "assx_mdp_"))) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    build = open(os.path.join(ROOT, "audio_source_separation_amd", "csrc", "build.sh")).read()
    assert build.count("assx_beamform") == 2  # the SRCS list and the link line
    chunk = int(re.search(r"#define ASSX_BF_FRAME_CHUNK (\d+)", raw).group(1))
    assert chunk == _lib.BF_FRAME_CHUNK == benv.FRAME_CHUNK
    for n in declared:  # the comments cite the reference lines each entry point replaces
        if n != "assx_bf_workspace_bytes":
            assert re.search(r"\b%s\s+(beamform|pca|minimum_distortion_principle)\.py:\d+" % n, raw), n


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_bf_workspace_bytes
    base = q(4, 3, 17, 1025)
    assert base > 0 and q(5, 3, 17, 1025) > base and q(4, 4, 17, 1025) > base and q(4, 3, 18, 1025) > base
    assert q(4, 3, 17, 2049) > base and q(1, 1, 1, 1) > 0 and q(8, 8, 1, 1) > 0
    for C, N, F, T in ((0, 3, 17, 65), (9, 3, 17, 65), (4, 0, 17, 65), (4, 9, 17, 65), (4, 3, 0, 65), (4, 3, 17, 0),
                       (4, 3, -1, 65), (4, 3, 17, -1)):
        assert q(C, N, F, T) == 0, (C, N, F, T)
    assert q(8, 2, 4096, 8191) > 0 and q(8, 2, 4096, 8192) == 0 and q(2, 8, 4096, 8192) == 0  # max(C, N) F T < 2^28
    assert q(2, 2, 2 ** 31 - 1, 2 ** 31 - 1) == 0 and q(2, 2, 2 ** 31 - 1, 1) == 0


def test_c_abi_refusals_need_no_gpu():
    """A NULL context is refused before anything else, whatever the sizes."""
    from audio_source_separation_amd import _lib
    L = _lib.lib
    null = ctypes.c_void_p(0)
    E_NULL = -3
    for M, N, F, T in ((4, 3, 5, 6), (9, 0, 0, -1)):
        assert L.assx_bf_apply(null, null, null, null, null, M, N, F, T, null) == E_NULL
        assert L.assx_bf_ds_weights(null, null, null, null, -1, M, N, F, null) == E_NULL
        assert L.assx_bf_ml_weights(null, null, null, null, null, 99, 1e-12, M, N, F, null, null) == E_NULL
        assert L.assx_pca_basis(null, null, null, null, null, M, F, null, null) == E_NULL
        assert L.assx_mdp_scale(null, null, null, null, null, M, N, F, T, null) == E_NULL


# ------------------------------------------------------------------------------------------------ the public surface
def test_every_refusal_of_the_envelope_touches_no_device():
    """ValueError before a device is touched: where no GPU is present, opening one would raise RuntimeError instead."""
    from audio_source_separation_amd.bss import beamform as B
    from audio_source_separation_amd.transform.pca import pca, pca_basis
    from audio_source_separation_amd.algorithm.minimum_distortion_principle import minimum_distortion_principle as mdp
    X, A, R = bf.mixture(3, 4, 20, 0), bf.steering(4, 3, 2, 1), np.tile(np.eye(3, dtype=complex), (4, 1, 1))
    beamformers = (lambda x, a, **kw: B.delay_sum_beamform(x, a, **kw), lambda x, a, **kw: B.ml_beamform(x, a, R, **kw),
                   lambda x, a, **kw: B.mvdr_beamform(x, a, **kw))
    for fn in beamformers:
        refused = [((X.real, A), "complex"), ((X[None], A), "one utterance"), ((X[0], A), "one utterance"),
                   ((X[:1], A[:, :1]), "n_channels"), ((np.ones((9, 4, 20), dtype=complex), np.ones((4, 9, 2))), "n_channels"),
                   ((X[:, :0], A[:0]), "empty"), ((X[:, :, :0], A), "empty"),
                   ((X, A[:3]), "steering_vector"), ((X, A[:, :2]), "steering_vector"), ((X, A[0]), "steering_vector"),
                   ((X, np.ones((4, 3, 9), dtype=complex)), "n_sources"), ((X, A[:, :, :0]), "n_sources")]
        for args, what in refused:
            with pytest.raises(ValueError, match=what):
                fn(*args)
        for ref in (3, -1, 0.0, True, "0"):
            with pytest.raises(ValueError, match="reference_id"):
                fn(X, A, reference_id=ref)
        for dtype in ("float32", np.float32, "complex64"):
            with pytest.raises(ValueError, match="float64"):
                fn(X, A, dtype=dtype)
    for bad in (R[:3], R[:, :2], R[:, :, :2], R[0]):
        with pytest.raises(ValueError, match="covariance"):
            B.ml_beamform(X, A, bad)
    for fn in (pca, pca_basis):
        for x in (X[0], X[None], X[0, 0]):
            with pytest.raises(ValueError, match="Invalid dimension."):
                fn(x)
        for x, what in ((X.real, "complex"), (X[:1], "n_channels"), (np.ones((9, 4, 20), dtype=complex), "n_channels"),
                        (X[:, :0], "empty"), (X[:, :, :0], "empty")):
            with pytest.raises(ValueError, match=what):
                fn(x)
        with pytest.raises(ValueError, match="float64"):
            fn(X, dtype="float32")
    Y = bf.mixture(2, 4, 20, 2)
    for ref in (X[0, 0], X[None]):
        with pytest.raises(ValueError, match=r"reference.ndim is expected 2 or 3, but given %d\." % ref.ndim):
            mdp(Y, ref)
    for args, what in (((Y.real, X), "complex"), ((Y, X.real), "complex"), ((Y[0], X), "one utterance"),
                       ((np.ones((9, 4, 20), dtype=complex), X), "n_channels"),
                       ((Y, np.ones((9, 4, 20), dtype=complex)), "n_channels"), ((Y[:, :, :0], X[:, :, :0]), "empty"),
                       ((Y, X[:, :3]), "reference"), ((Y, X[0, :, :5]), "reference")):
        with pytest.raises(ValueError, match=what):
            mdp(*args)
    with pytest.raises(ValueError, match="float64"):
        mdp(Y, X, dtype="float32")


def test_the_three_class_deviations(monkeypatch):
    from audio_source_separation_amd import bss
    from audio_source_separation_amd.bss import beamform as B
    assert {"DelaySumBeamformer", "MVDRBeamformer", "MaxSNRBeamformer"} <= set(bss.__all__)
    assert bss.MVDRBeamformer is B.MVDRBeamformer and B.EPS == 1e-12
    X, A, R = bf.mixture(3, 4, 20, 0), bf.steering(4, 3, 2, 1), np.tile(np.eye(3, dtype=complex), (4, 1, 1))
    calls = []
    monkeypatch.setattr(B, "delay_sum_beamform", lambda x, a, **kw: calls.append(("ds", kw)) or "ds")
    monkeypatch.setattr(B, "mvdr_beamform", lambda x, a, **kw: calls.append(("mvdr", kw)) or "mvdr")
    monkeypatch.setattr(B, "ml_beamform", lambda x, a, r, **kw: calls.append(("ml", r, kw)) or "ml")

    # the constructors, attributes and the check are the reference's
    d = B.DelaySumBeamformer()
    assert d.steering_vector is None and d.reference_id == 0
    with pytest.raises(ValueError, match=r"^Specify steering vector\.$"):
        d(X)
    assert d.input is X and not hasattr(d, "estimation")
    assert d(X, A) == "ds" and d.estimation == "ds" and d.steering_vector is A and calls[-1][1]["reference_id"] == 0
    with pytest.raises(TypeError):
        B.MVDRBeamformer()  # steering_vector has no default there
    # 1: MVDRBeamformer.__call__ works, with mvdr_beamform, or ml_beamform when a covariance is given
    m = B.MVDRBeamformer(A, 2, 1e-9)
    assert (m.reference_id, m.eps) == (2, 1e-9)
    assert m(X) == "mvdr" and calls[-1][0] == "mvdr" and calls[-1][1]["reference_id"] == 2 and calls[-1][1]["eps"] == 1e-9
    assert m(X, covariance=R) == "ml" and calls[-1][0] == "ml" and calls[-1][1] is R and m.estimation == "ml"
    with pytest.raises(ValueError, match=r"^Specify steering vector\.$"):
        B.MVDRBeamformer(None)(X)
    # 2: MaxSNRBeamformer.__call__ raises after the same check
    with pytest.raises(ValueError, match=r"^Specify steering vector\.$"):
        B.MaxSNRBeamformer(None)(X)
    s = B.MaxSNRBeamformer(None, 1)
    with pytest.raises(NotImplementedError):
        s(X, A)
    assert s.steering_vector is A and (s.reference_id, s.eps) == (1, 1e-12)
    for cls in (B.DelaySumBeamformer, B.MVDRBeamformer, B.MaxSNRBeamformer):
        with pytest.raises(ValueError, match="float64"):
            cls(A, dtype="float32")
    # 3: no "in progress" warning on import
    code = ("import warnings; warnings.simplefilter('error'); import audio_source_separation_amd.bss.beamform; "
            "from audio_source_separation_amd.bss import MVDRBeamformer")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr


# ------------------------------------------------------------------------------------------------ the envelope grid
def test_grid_covers_the_envelope():
    assert benv.FRAMES[:6] == (63, 64, 65, 255, 256, 257) and benv.FRAMES[6:] == tuple(benv.FRAME_CHUNK + k for k in (-1, 0, 1))
    sizes = {v[:4] for v in benv.GRID.values()}
    for M in range(2, 9):
        for N in {1, M - 1, M, 8}:
            for F in (1, 3, 17):
                for T in benv.FRAMES:
                    assert (M, N, F, T) in sizes
            assert (M, N, 3, 1) in {v[:4] for v in benv.TINY.values()}
    assert len(sizes) == len(benv.GRID) and all(T >= 4 * M for M, _, _, T in sizes)
    assert set(benv.OUTPUTS.values()) == set(benv.D) and all(0 < d < 1e-12 for d in benv.D.values())


@pytest.mark.parametrize("case", ["m2_n1_f1_t63", "m5_n8_f3_t257", "m8_n7_f17_t1025"])
def test_grid_states_meet_their_conditions_and_the_probe_its_table(case):
    st, ref = benv.grid_case(case)
    benv.check_state(case, st)
    assert set(ref) == set(benv.OUTPUTS)
    for k, v in benv.sensitivity(st).items():
        assert v <= benv.D[benv.kind(k)], (k, v)


def test_generator_reproduces_the_fixtures():
    if not os.path.isdir(os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")):
        pytest.skip("the reference tree is not present")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_beamform.py"), "--verify"], capture_output=True,
                             text=True)
    n_files = len([f for f in os.listdir(GOLDEN) if f.endswith(".npz")])
    assert run.returncode == 0 and "verified %d files, 0 problems" % n_files in run.stdout, run.stdout + run.stderr
