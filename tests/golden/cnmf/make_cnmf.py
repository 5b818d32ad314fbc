"""Golden vectors of ComplexEUCNMF (Kameoka's complex NMF), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  Each
case file holds a seeded target (a rank-3 magnitude with uniform random phase), the seed of the global NumPy RNG the
reference draws basis, activation and phase from (in that order), the basis and activation it drew (T0, V0; its phase
draw is overwritten by the target's phase at once), `rng_next` = the next np.random.rand() after its `_reset`, the state
(basis, activation, phase) after iterations 1, 2, 5, 19 and 20 -- and 4 where the file stays small, so that 4 -> 5 is
one more recorded step --, `regularizer`, `p`, `eps`, and two loss lists:

    loss            sum |sum_k T V exp(i Phi) - X|^2 of the reference's model after every iteration
    loss_reference  the list the reference itself records: it multiplies by the angle Phi, not by exp(i Phi)

No reference source is copied.

    python tests/golden/cnmf/make_cnmf.py            # write the files next to this script
    python tests/golden/cnmf/make_cnmf.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path
from algorithm.nmf import ComplexEUCNMF  # noqa: E402

OUT_DIR = HERE
SNAP_ITERS = (1, 2, 5, 19, 20)
EXTRA_ITER, EXTRA_MAX_PHASE = 4, 13000  # iteration 4 too while the phase has at most this many entries
N_ITER = 20
ATTRS = ("basis", "activation", "phase")

# (F, T, K, p, regularizer, silent): `silent` zeroes one bin and frames 5-6 of the target
CASES = (
    (17, 40, 1, 1, 0.1, True),      # Beta = 1; silent entries give Zbar exactly 0, so the angle is 0
    (17, 40, 2, 1, 0.1, False),
    (33, 65, 6, 1.2, 1e-3, False),  # general power
    (9, 130, 3, 2, 0.1, False),
    (17, 40, 7, 1, 0.1, True),      # basis and activation go negative
    (5, 257, 16, 0.7, 1e-2, False),  # frames cross a tile; negative activation
    (8, 64, 64, 1, 0.1, False),     # n_basis at the cap
    (1, 70, 3, 1, 0.1, False),      # one bin
    (40, 1, 3, 1.2, 0.1, False),    # one frame
    (13, 63, 5, 1, 0.0, False),     # no regulariser
)


def case_name(F, T, K, p, regularizer, silent):
    tag = lambda v: ("%g" % v).replace(".", "p").replace("-", "m")  # noqa: E731
    return "cnmf_f%d_t%d_k%d_p%s_r%s%s" % (F, T, K, tag(p), tag(regularizer), "_silent" if silent else "")


def target(F, T, silent, seed):
    rng = np.random.default_rng(seed)
    X = (rng.random((F, 3)) @ rng.random((3, T))) * np.exp(2j * np.pi * rng.random((F, T)))
    if silent:
        X[3, :] = 0
        X[:, 5:7] = 0
    return X


def model_loss(model, X):
    Y = np.sum(model.basis[:, :, None] * model.activation[None] * np.exp(1j * model.phase), axis=1) - X
    return np.sum(Y.real ** 2 + Y.imag ** 2)


def gen_case(F, T, K, p, regularizer, silent, idx):
    seed = 1400 + idx
    X = target(F, T, silent, seed)
    np.random.seed(seed)
    T0 = np.random.rand(F, K)
    V0 = np.random.rand(K, T)

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        np.random.seed(seed)
        model = ComplexEUCNMF(n_basis=K, regularizer=regularizer, p=p)
        model.target = X
        model._reset()
        rng_next = np.random.rand()
        assert np.array_equal(model.basis, T0) and np.array_equal(model.activation, V0)
        assert np.array_equal(model.phase[:, 0, :], np.angle(X))
        snaps, loss = {}, []
        for it in range(1, N_ITER + 1):
            model.update(iteration=1)  # update_once + the reference's own loss entry
            loss.append(model_loss(model, X))
            if it in SNAP_ITERS or (it == EXTRA_ITER and F * K * T <= EXTRA_MAX_PHASE):
                for a in ATTRS:
                    snaps["%s_%d" % (a, it)] = np.array(getattr(model, a))

        # the same through the reference's front door
        np.random.seed(seed)
        whole = ComplexEUCNMF(n_basis=K, regularizer=regularizer, p=p)
        Tb, V, Phi = whole(X, iteration=N_ITER)
    assert np.array_equal(Tb, snaps["basis_20"]) and np.array_equal(V, snaps["activation_20"])
    assert np.array_equal(Phi, snaps["phase_20"]) and whole.loss == model.loss
    assert all(np.all(np.isfinite(v)) for v in snaps.values())
    return dict(X=X, seed=np.int64(seed), T0=T0, V0=V0, rng_next=np.float64(rng_next), loss=np.array(loss),
                loss_reference=np.array(model.loss), regularizer=np.float64(regularizer), p=np.float64(p),
                eps=np.float64(model.eps), silent=np.array(bool(silent)), **snaps)


def save(name, arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, versions=make_golden.VERSIONS, **arrays)
    print("wrote %-44s %8.1f KiB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def generate():
    for idx, case in enumerate(CASES):
        save(case_name(*case), gen_case(*case, idx))


def verify():
    import tempfile
    global OUT_DIR
    bad = []
    with tempfile.TemporaryDirectory() as tmp:
        OUT_DIR = tmp
        generate()
        OUT_DIR = HERE
        fresh = sorted(f for f in os.listdir(tmp) if f.endswith(".npz"))
        for f in fresh:
            path = os.path.join(HERE, f)
            if not os.path.exists(path):
                bad.append("%s: not committed" % f)
                continue
            a, b = np.load(os.path.join(tmp, f)), np.load(path)
            if sorted(a.files) != sorted(b.files):
                bad.append("%s: keys differ" % f)
                continue
            for k in a.files:
                if k != "versions" and (a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
                                        or a[k].tobytes() != b[k].tobytes()):
                    bad.append("%s[%s] differs" % (f, k))
        for f in sorted(set(x for x in os.listdir(HERE) if x.endswith(".npz")) - set(fresh)):
            bad.append("%s: committed but not generated" % f)
    print("verified %d files, %d problems" % (len(fresh), len(bad)))
    for line in bad:
        print("  MISMATCH", line)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--verify"]:
        sys.exit(verify())
    generate()
