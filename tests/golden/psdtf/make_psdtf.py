"""Golden vectors of LDPSDTF (log-det positive semidefinite tensor factorisation), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  Each
case file holds a seeded target X (n_bins, n_bins, n_frames) (two random PSD bases times random activations plus
0.05 x x^T with x (n_bins, 2) per frame), the seed of the global NumPy RNG the reference draws from, the draws themselves
(`draw_V` (n_basis, n_bins): the diagonals of the bases, then `draw_H` (n_basis, n_frames)), `rng_next` = the next
np.random.rand() after them, `eps`, `normalize`, the state the first update starts from (V0, H0: the draws after the
reference's reset), the state (basis, activation) after iterations 1, 2, 4, 5, 19 and 20, and `loss` (20,).

The maker asserts that no NumPy warning is raised, that every recorded value is finite, that every activation entry is at
least 1e-8 of its row maximum, that cond(Y) <= 1e4 at every recorded state, and that the reference's front door reproduces
the stepwise run bit for bit.  No reference source is copied.

    python tests/golden/psdtf/make_psdtf.py            # write the files next to this script
    python tests/golden/psdtf/make_psdtf.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path
import psdtf_np as pt  # noqa: E402
from algorithm.psdtf import LDPSDTF  # noqa: E402

OUT_DIR = HERE

# (n_bins, n_frames, n_basis, normalize)
CASES = (
    (4, 10, 2, True),
    (1, 9, 2, True),       # one bin
    (5, 1, 2, True),       # one frame
    (7, 70, 1, True),      # one basis
    (16, 33, 3, True),
    (9, 9, 64, True),      # n_basis at the cap
    (64, 5, 3, True),      # n_bins at the cap
    (3, 257, 4, True),     # frames cross 256
    (33, 20, 2, True),     # n_bins crosses 32
    (8, 20, 3, False),     # no normalisation
)


def case_name(M, T, K, norm):
    return "psdtf_m%d_t%d_k%d%s" % (M, T, K, "" if norm else "_nonorm")


def target(M, T, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((2, M, M))
    W = A @ np.transpose(A, (0, 2, 1)) / M
    x = rng.standard_normal((T, M, 2))
    X = np.einsum("kt,kij->tij", rng.random((2, T)) + 0.1, W) + 0.05 * x @ np.transpose(x, (0, 2, 1))
    X = (X + np.transpose(X, (0, 2, 1))) / 2
    return np.ascontiguousarray(np.transpose(X, (1, 2, 0)))


def check_state(V, H, eps, what):
    assert np.all(np.isfinite(V)) and np.all(np.isfinite(H)), (what, "not finite")
    assert np.all(H >= 1e-8 * np.max(H, axis=1, keepdims=True)), (what, "an activation entry below 1e-8 of its row")
    Y = pt.to_psd(pt.reconstruct(pt.kmm(V), H), eps)
    assert np.max(np.linalg.cond(Y)) <= 1e4, (what, "cond(Y) = %g" % np.max(np.linalg.cond(Y)))


def gen_case(M, T, K, norm, idx):
    seed = 2300 + idx
    eps = 1e-12
    X = target(M, T, seed)
    np.random.seed(seed)
    draw_V = np.random.rand(K, M)
    draw_H = np.random.rand(K, T)
    rng_next = np.random.rand()

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        np.random.seed(seed)
        model = LDPSDTF(n_basis=K, normalize=norm, eps=eps)
        model.target = X
        model._reset()
        V0, H0 = np.array(model.basis), np.array(model.activation)
        check_state(V0, H0, eps, "start")
        snaps, loss = {}, []
        for it in range(1, pt.N_ITER + 1):
            model.loss = []
            model.update(iteration=1)
            loss.append(model.loss[0])
            if it in pt.SNAP_ITERS:
                snaps["basis_%d" % it] = np.array(model.basis)
                snaps["activation_%d" % it] = np.array(model.activation)
                check_state(snaps["basis_%d" % it], snaps["activation_%d" % it], eps, it)

        # the same through the reference's front door
        np.random.seed(seed)
        whole = LDPSDTF(n_basis=K, normalize=norm, eps=eps)
        V, H = whole(X, iteration=pt.N_ITER)
        assert np.random.rand() == rng_next
    assert np.array_equal(V, snaps["basis_20"]) and np.array_equal(H, snaps["activation_20"]) and whole.loss == loss
    arrays = dict(X=X, seed=np.int64(seed), eps=np.float64(eps), normalize=np.bool_(norm), draw_V=draw_V, draw_H=draw_H,
                  V0=V0, H0=H0, rng_next=np.float64(rng_next), loss=np.array(loss), **snaps)
    for k, v in arrays.items():
        assert np.all(np.isfinite(v)), (k, "not finite")
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
