"""Golden vectors of the covariance-domain MultichannelISNMF (algorithm/nmf.py), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  Each
case file holds a positive-definite target X (n_bins, n_frames, n_channels, n_channels) -- the mean of `smooth` >=
n_channels consecutive outer products of a seeded convolutive mixture (`covnmf_np.target`) --, the seed of the global
NumPy RNG the reference draws from, the draws themselves (`T0` first, then `V0`), `rng_next` = the next
np.random.rand() after them, `eps`, `normalize`, `n_basis`, `smooth`, the state after iterations 1, 2, 5 and 20
(`H_<it>`, `T_<it>`, `V_<it>`) and `loss` (20,: one entry after every iteration, none before the loop).

The maker asserts that no NumPy warning is raised, that every recorded value is finite, that at every recorded state
cond(X^ + eps I) <= 1e8, no denominator of the basis or activation update is within six orders of magnitude of its eps
floor and every activation entry is at least 1e-8 of its row maximum, and that the reference's front door reproduces
the stepwise run bit for bit.  A case that fails a condition gets another seed (SEEDS), not a wider condition.  It
prints, per case, the largest distance of the restatement tests/covnmf_np.py from the reference (states relative to
their largest entry, loss relative).  No reference source is copied.

    python tests/golden/covnmf/make_covnmf.py            # write the files next to this script
    python tests/golden/covnmf/make_covnmf.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path
import covnmf_np as cv  # noqa: E402
from algorithm.nmf import MultichannelISNMF  # noqa: E402

OUT_DIR = HERE

# (n_channels, n_bins, n_frames, n_basis, smooth, normalize)
CASES = (
    (2, 5, 40, 3, 3, True),
    (3, 4, 33, 2, 3, True),
    (4, 6, 64, 4, 5, True),
    (5, 3, 48, 1, 6, True),     # one basis
    (6, 2, 40, 3, 7, True),
    (7, 2, 40, 2, 8, True),
    (8, 3, 70, 2, 8, True),
    (8, 3, 70, 2, 9, False),    # no normalisation
    (2, 3, 20, 64, 2, True),    # n_basis at the cap
    (2, 4, 257, 2, 2, True),    # frames cross 256
)

# a case that fails one of the maker's conditions gets another seed
SEEDS = {}

COND_MAX = 1e8
MIN_DENOMINATOR = 1e-6
MIN_ACTIVATION = 1e-8


def case_name(M, F, T, K, smooth, norm):
    return "covnmf_m%d_f%d_t%d_k%d_s%d%s" % (M, F, T, K, smooth, "" if norm else "_nonorm")


def snapshot(model, tag, out):
    out["H_%s" % tag] = np.array(model.spatial, dtype=np.complex128)
    out["T_%s" % tag] = np.array(model.basis)
    out["V_%s" % tag] = np.array(model.activation)


def check_state(X, H, Tb, V, tag, eps):
    what = "state %s" % tag
    assert np.all(V >= MIN_ACTIVATION * np.max(V, axis=1, keepdims=True)), (what, "an activation entry below 1e-8 of its row")
    cond = float(np.max(np.linalg.cond(cv.reconstruct(Tb, V, H) + eps * np.eye(X.shape[-1]))))
    assert cond <= COND_MAX, (what, "cond(X^ + eps I) = %g" % cond)
    low = cv.denominators(X, Tb, V, H, eps)
    assert low > MIN_DENOMINATOR, (what, "a denominator of %g" % low)


def gen_case(M, F, T, K, smooth, norm, idx):
    seed = SEEDS.get(idx, 2700 + idx)
    eps = 1e-12
    X = cv.target(M, F, T, smooth, seed)
    np.random.seed(seed)
    T0 = np.random.rand(F, K)
    V0 = np.random.rand(K, T)
    rng_next = np.random.rand()

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        np.random.seed(seed)
        model = MultichannelISNMF(n_basis=K, normalize=norm, eps=eps)
        model.target = X
        model._reset()
        assert np.array_equal(model.basis, T0) and np.array_equal(model.activation, V0)
        snaps, loss = {}, []
        for it in range(1, cv.N_ITER + 1):
            model.update_once()
            loss.append(model.criterion(model.reconstruct(), X).sum())
            if it in cv.SNAP_ITERS:
                snapshot(model, str(it), snaps)

        # the same through the reference's front door
        np.random.seed(seed)
        whole = MultichannelISNMF(n_basis=K, normalize=norm, eps=eps)
        out = whole(X, iteration=cv.N_ITER)
        assert np.random.rand() == rng_next
        final = {}
        snapshot(whole, str(cv.N_ITER), final)
        assert all(np.array_equal(final[k], snaps[k]) for k in final) and whole.loss == loss
        assert all(np.array_equal(a, b) for a, b in zip(out, (whole.spatial, whole.basis, whole.activation)))

        arrays = dict(X=X, seed=np.int64(seed), eps=np.float64(eps), normalize=np.bool_(norm), n_basis=np.int64(K),
                      smooth=np.int64(smooth), rng_next=np.float64(rng_next), T0=T0, V0=V0, loss=np.array(loss), **snaps)
        for k, v in arrays.items():
            assert np.all(np.isfinite(v)), (k, "not finite")
        check_state(X, cv.init_spatial(M, F, K), T0, V0, "0", eps)
        for it in cv.SNAP_ITERS:
            check_state(X, snaps["H_%d" % it], snaps["T_%d" % it], snaps["V_%d" % it], str(it), eps)

        # the restatement against the reference
        states, rloss = cv.run(X, T0, V0, cv.N_ITER, normalize=norm, eps=eps)
        early = max(cv.rel(a, snaps["%s_%d" % (n, it)]) for it in cv.SNAP_ITERS[:-1] for n, a in zip("HTV", states[it]))
        late = max(cv.rel(a, snaps["%s_%d" % (n, cv.N_ITER)]) for n, a in zip("HTV", states[cv.N_ITER]))
        dl = float(np.max(np.abs(np.array(rloss) - np.array(loss)) / np.abs(loss)))
        print("  %-32s restatement: states <= it 5 %.1e, it 20 %.1e, loss %.1e" % (case_name(M, F, T, K, smooth, norm),
                                                                                    early, late, dl))
    return arrays


def save(name, arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, versions=make_golden.VERSIONS, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print("wrote %-40s %8.1f KiB" % (os.path.basename(path), size / 1024))


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
