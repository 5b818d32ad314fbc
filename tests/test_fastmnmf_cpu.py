"""FastMultichannelISNMF without a GPU: the NumPy restatement (tests/fastmnmf_np.py) against the reference's own output
(tests/golden/fastmnmf/*.npz), the fixture recipe, and the C-ABI rows of the new entry points."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fastmnmf_np as fm  # noqa: E402
import envelope_np as env  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "fastmnmf")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ATTRS = ("basis", "activation", "spatial_covariance", "diagonalizer")


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_fixtures_present():
    assert len(FILES) == 12
    for f in FILES:
        assert os.path.getsize(f) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = load(name)
    normalize = str(g["normalize"]) or False
    snaps = {}

    def record(i, state):
        if i in (1, 2, 5, 20):
            snaps[i] = dict(state)

    Y, losses, _ = fm.run(g["X"], g["W0"], g["H0"], 20, normalize=normalize, record=record)
    scale = np.max(np.abs(g["loss"]))
    lerr = np.abs(np.asarray(losses) - g["loss"]) / scale
    # an ill-conditioned trajectory (envelope_np.FASTMNMF_ILL_CONDITIONED): the usual tolerances up to iteration 10,
    # 256 x the restatement's own one-ulp sensitivity after it
    late, late_loss = {}, np.zeros(21)
    if name in env.FASTMNMF_ILL_CONDITIONED:
        d, dl = env.fastmnmf_trajectory_sensitivity(g)
        late = {a: env.FACTOR * v for a, v in d.items()}
        late_loss[env.LAST_STABLE_ITERATION + 1:] = env.FACTOR * dl[env.LAST_STABLE_ITERATION + 1:]
    assert np.all(lerr < np.maximum(1e-12, late_loss)), lerr
    for i in (1, 2, 5, 20):
        # summation order alone moves the 20-iteration state by up to 4.2e-12 (diagonalizer, m4_n3_k2): 1e-11 there
        tol = 1e-12 if i <= 5 else 1e-11
        for a in ATTRS:
            assert rel(snaps[i][a], g["%s_%d" % (a, i)]) < (max(tol, late.get(a, 0)) if i == 20 else tol), (i, a)
        if i < 20:
            s = snaps[i]
            est = fm.separate(g["X"], s["basis"], s["activation"], s["spatial_covariance"], s["diagonalizer"])
            assert rel(est, g["estimation_%d" % i]) < 1e-12, i
    assert rel(Y, g["output"]) < max(1e-11, late.get("output", 0))


def test_only_ill_conditioned_fixtures_are_listed_as_such():
    """A fixture is on envelope_np.FASTMNMF_ILL_CONDITIONED exactly when the restatement ALONE, run again from a basis
    changed by one ulp, ends somewhere else after 20 iterations; up to iteration 10 all of them are stable."""
    for name in NAMES:
        g = load(name)
        d, dl = env.fastmnmf_trajectory_sensitivity(g)
        worst = max(d.values())
        print("%-28s 20 iterations: %.1e" % (name, worst))
        assert (worst > 1e-7) == (name in env.FASTMNMF_ILL_CONDITIONED), (name, d)
        assert worst < 1e-10 or worst > 1e-7, (name, d)  # nothing in between: the list is not a matter of taste
        assert np.all(dl[:env.LAST_STABLE_ITERATION + 1] < 1e-13), (name, dl)
        d10, _ = env.fastmnmf_trajectory_sensitivity(g, env.LAST_STABLE_ITERATION)
        assert max(d10.values()) < 1e-11, (name, d10)


def test_initial_draw_is_the_reference_rng_order():
    g = load(NAMES[0])
    np.random.seed(int(g["seed"]))
    assert np.array_equal(np.random.rand(*g["W0"].shape), g["W0"])
    assert np.array_equal(np.random.rand(*g["H0"].shape), g["H0"])


def test_reference_loss_is_monotone():
    for name in NAMES:
        loss = load(name)["loss"]
        assert np.all(np.diff(loss) <= 1e-9 * np.abs(loss[:-1])), name


def test_generator_verify():
    """make_fastmnmf.py --verify re-runs the reference into a temporary directory and compares every array."""
    ref = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")
    if not os.path.isdir(os.path.join(ref, "bss")):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_fastmnmf.py"), "--verify"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cabi_rows():
    from audio_source_separation_amd import _lib
    names = ("workspace_bytes", "project", "update_nmf", "update_scm", "update_diagonalizer_model", "normalize_power",
             "separate", "iterate")
    for n in names:
        assert "assx_fastmnmf_" + n in _lib.SIGNATURES
        assert hasattr(_lib.lib, "assx_fastmnmf_" + n)


def test_workspace_query_refuses_out_of_range_sizes():
    from audio_source_separation_amd import _lib
    ws = _lib.lib.assx_fastmnmf_workspace_bytes
    assert ws(1, 4, 4, 1025, 4096, 4, _lib.F64) > 2 * 4 * 1025 * 4096 * 8
    for B, M, N, K in ((1, 1, 1, 4), (1, 9, 4, 4), (1, 4, 0, 4), (1, 4, 9, 4), (1, 4, 4, 0), (1, 4, 4, 65)):
        assert ws(B, M, N, 17, 64, K, _lib.F64) == 0, (M, N, K)
