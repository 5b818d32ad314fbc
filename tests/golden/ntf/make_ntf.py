"""Golden vectors of EUCNTF (non-negative tensor factorisation), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  Each
case file holds a seeded target X (N, I, J) (a rank-3 tensor with 1 % noise), the seed of the global NumPy RNG the
reference draws partitioning, basis and activation from (in that order), the draws themselves (Z0, T0, V0), `rng_next` =
the next np.random.rand() after them, `eps`, the state (partitioning, basis, activation) after iterations 1, 2, 4, 5, 19
and 20, and `loss` (20,), the reference's compute_loss() after every iteration.

The maker asserts that every recorded entry is a normal positive double, that the reference's front door reproduces the
stepwise run bit for bit, and, for the floor case, that each of the six sums an update floors has, at some recorded start
state, an entry below eps and an entry at or above it.  No reference source is copied.

    python tests/golden/ntf/make_ntf.py            # write the files next to this script
    python tests/golden/ntf/make_ntf.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path
import ntf_np as nt  # noqa: E402
from algorithm.ntf import EUCNTF  # noqa: E402

OUT_DIR = HERE
ATTRS = ("partitioning", "basis", "activation")
TINY = np.finfo(np.float64).tiny

# (N, I, J, K, eps, tag).  "silent": bin 3, frames 5-6 and channel 1 of the target are zero, so the numerator floors bind
# in all three updates and Z[1] collapses.  "floor": eps so large that every floored sum both binds and stays free.
CASES = (
    (2, 17, 40, 3, 1e-12, ""),
    (1, 9, 70, 1, 1e-12, ""),          # one channel, one basis
    (3, 33, 65, 6, 1e-12, "silent"),
    (4, 5, 257, 16, 1e-12, ""),        # frames cross a 256 tile
    (5, 129, 7, 10, 1e-12, ""),        # bins cross a tile; K no multiple of 4; J < 64
    (8, 8, 64, 64, 1e-12, ""),         # K at the cap
    (32, 3, 5, 2, 1e-12, ""),          # N at the cap
    (2, 1, 70, 3, 1e-12, ""),          # one bin
    (2, 40, 1, 3, 1e-12, ""),          # one frame
    (6, 7, 9, 3, 4.0, "floor"),
)


def case_name(N, I, J, K, eps, tag):
    return "ntf_n%d_i%d_j%d_k%d%s" % (N, I, J, K, "_" + tag if tag else "")


def target(N, I, J, tag, seed):
    rng = np.random.default_rng(seed)
    X = np.einsum("nk,ik,kj->nij", rng.random((N, 3)), rng.random((I, 3)), rng.random((3, J)))
    X = X * (1 + 0.01 * rng.random((N, I, J)))
    if tag == "silent":
        X[:, 3, :] = 0
        X[:, :, 5:7] = 0
        X[1] = 0
    return X


def floors_bind_and_stay_free(fx):
    """For each of the six floored sums: is there a recorded start state with an entry below eps and one at or above?"""
    eps = float(fx["eps"])
    both = [False] * 6
    for it in nt.START_ITERS:
        sums = []
        nt.update(fx["X"], *nt.state(fx, it), eps, sums=sums)
        flat = [s for pair in sums for s in pair]
        for q, s in enumerate(flat):
            both[q] = both[q] or bool((s < eps).any() and (s >= eps).any())
    return both


def gen_case(N, I, J, K, eps, tag, idx):
    seed = 2200 + idx
    X = target(N, I, J, tag, seed)
    np.random.seed(seed)
    Z0 = np.random.rand(N, K)
    T0 = np.random.rand(I, K)
    V0 = np.random.rand(K, J)
    rng_next = np.random.rand()

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        model = EUCNTF(K, eps=eps)
        model.target = X
        model.partitioning, model.basis, model.activation = Z0.copy(), T0.copy(), V0.copy()
        snaps, loss = {}, []
        for it in range(1, nt.N_ITER + 1):
            model.update_once()
            loss.append(model.compute_loss().sum())
            if it in nt.SNAP_ITERS:
                for a in ATTRS:
                    snaps["%s_%d" % (a, it)] = np.array(getattr(model, a))

        # the same through the reference's front door
        np.random.seed(seed)
        whole = EUCNTF(K, eps=eps)
        Z, T, V = whole(X, iteration=nt.N_ITER)
        assert np.random.rand() == rng_next
    assert np.array_equal(Z, snaps["partitioning_20"]) and np.array_equal(T, snaps["basis_20"])
    assert np.array_equal(V, snaps["activation_20"]) and whole.loss == loss
    assert np.array_equal(whole.target, X)
    arrays = dict(X=X, seed=np.int64(seed), eps=np.float64(eps), Z0=Z0, T0=T0, V0=V0, rng_next=np.float64(rng_next),
                  loss=np.array(loss), **snaps)
    for k, v in arrays.items():
        if k not in ("X", "seed"):
            assert np.all(np.isfinite(v)) and np.all(v >= TINY), (k, "not a normal positive double")
    assert np.all(np.isfinite(X)) and np.all(X >= 0)
    if tag == "floor":
        assert all(floors_bind_and_stay_free(arrays)), floors_bind_and_stay_free(arrays)
    return arrays


def save(name, arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, versions=make_golden.VERSIONS, **arrays)
    print("wrote %-32s %8.1f KiB" % (os.path.basename(path), os.path.getsize(path) / 1024))


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
