"""MultichannelISNMF without a GPU: the NumPy restatement (tests/mnmf_np.py) against the reference's own output
(tests/golden/mnmf/*.npz), the closed-form loss, and the host-side argument checks of the class."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mnmf_np as mn  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "mnmf")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "mnmf_*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FILES]
ATTRS = ("basis", "activation", "latent", "spatial")


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_fixtures_present():
    assert len(FILES) == 13
    for f in FILES + [os.path.join(GOLDEN, "riccati.npz")]:
        assert os.path.getsize(f) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = load(name)
    snaps = {}

    def record(i, state):
        if i in (1, 2, 5, 20):
            snaps[i] = dict(state)

    Y, losses, _ = mn.run(g["X"], g["T0"], g["V0"], g["Z0"], 20, normalize=bool(g["normalize"]), record=record,
                          with_loss=False)
    for i in (1, 2, 5, 20):
        for a in ATTRS:
            tol = 1e-12 if i <= 5 else 1e-10
            if a == "spatial" and not g["normalize"] and i == 5:
                tol = 3e-12  # without the trace normalisation H carries the scale freedom: 1.4e-12 measured
            assert rel(snaps[i][a], g["%s_%d" % (a, i)]) < tol, (i, a)
        if i < 20:
            s = snaps[i]
            est = mn.separate(g["X"], s["basis"], s["activation"], s["latent"], s["spatial"])
            assert rel(est, g["estimation_%d" % i]) < 1e-11, i
    assert rel(Y, g["output"]) < 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_loss_on_reference_snapshots(name):
    g = load(name)
    M, F, _ = g["X"].shape
    N = g["Z0"].shape[0]
    got = [mn.loss(g["X"], g["T0"], g["V0"], g["Z0"], mn.init_spatial(M, N, F))]
    for i in (1, 2, 5, 20):
        got.append(mn.loss(g["X"], g["basis_%d" % i], g["activation_%d" % i], g["latent_%d" % i], g["spatial_%d" % i]))
    want = g["loss"][[0, 1, 2, 5, 20]]
    assert np.max(np.abs(np.asarray(got) - want) / np.abs(want)) < 1e-5


def test_riccati_restatement():
    r = np.load(os.path.join(GOLDEN, "riccati.npz"))
    for M in range(2, 9):
        H = mn.riccati(r["A_%d" % M], r["B_%d" % M])
        assert rel(H, r["H_%d" % M]) < 1e-11, M
        assert rel(H @ r["A_%d" % M] @ H, r["B_%d" % M]) < 1e-10, M
    assert np.all(mn.riccati(np.zeros((1, 3, 3)), np.eye(3)[None]) == 0)


def cls():
    from audio_source_separation_amd.bss.mnmf import MultichannelISNMF
    return MultichannelISNMF


def test_repr_and_defaults():
    m = cls()(n_basis=20, n_sources=2, normalize=False)
    assert repr(m) == "IS-MNMF(n_basis=20, n_sources=2, normalize=False, author=Sawada)"
    assert m.reference_id == 0 and m.eps == 1e-12 and m.loss == [] and m.callbacks is None
    assert not hasattr(m, "basis") and not hasattr(m, "spatial")
    m2 = cls()(callbacks=print, recordable_loss=False)
    assert m2.callbacks == [print] and m2.loss is None and m2.n_basis == 10 and m2.normalize is True


@pytest.mark.parametrize("kw", [dict(hoge=1), dict(target=None), dict(author="Ozerov"), dict(author="foo"),
                                dict(dtype="float32"), dict(reference_id=-1)])
def test_invalid_arguments(kw):
    with pytest.raises(ValueError):
        cls()(**kw)


def test_invalid_keywords_message():
    with pytest.raises(ValueError, match="Invalid keywords."):
        cls()(n_basis=2, hoge=1)
