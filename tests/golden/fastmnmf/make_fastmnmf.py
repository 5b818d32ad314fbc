"""Golden vectors of FastMultichannelISNMF, made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  The
files hold a seeded mixture, the seed of the global NumPy RNG the reference draws basis and activation from, the
state after iterations 1, 2, 5 and 20 (basis, activation, spatial_covariance, diagonalizer, estimation), the loss list
and the output.  No reference source is copied.

    python tests/golden/fastmnmf/make_fastmnmf.py            # write the files next to this script
    python tests/golden/fastmnmf/make_fastmnmf.py --verify   # regenerate into a temporary directory and compare

The files live in this subdirectory: `make_golden.py --verify` flags every top-level file its own groups do not write.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  NumPy-2 `solve` shim, reference on sys.path, convolutive_mixture
from bss.mnmf import FastMultichannelISNMF  # noqa: E402

OUT_DIR = HERE
SNAP_ITERS = (1, 2, 5, 20)
N_ITER = 20

# (M, N, K, normalize, F, T)
CASES = (
    (2, 2, 3, "power", 17, 128),
    (3, 2, 4, "power", 17, 128),
    (4, 4, 10, "power", 17, 96),
    (4, 3, 2, "power", 17, 128),
    (3, 5, 2, "power", 17, 96),
    (6, 4, 3, "power", 17, 96),
    (8, 8, 2, "power", 11, 96),
    (3, 2, 4, False, 17, 128),
    # the corners of the size envelope (appended: the seeds and bytes of the files above do not change); T shrinks
    # with N * K so that five copies of the (N, K, T) activation stay under the 1 MiB a committed file may have
    (5, 6, 17, "power", 9, 80),
    (7, 7, 33, "power", 7, 48),
    (8, 8, 64, "power", 5, 32),
    (3, 1, 4, "power", 9, 100),
)


def case_name(M, N, K, normalize):
    return "fastmnmf_m%d_n%d_k%d%s" % (M, N, K, "" if normalize == "power" else "_nonorm")


def gen_case(M, N, K, normalize, F, T, idx):
    seed = 1200 + idx
    X = make_golden.convolutive_mixture(M, F, T, seed=seed)
    snaps = {}
    names = ("basis", "activation", "spatial_covariance", "diagonalizer", "estimation")

    def record(model):
        it = len(model.loss) - 1
        if it in SNAP_ITERS:
            for a in names:
                snaps["%s_%d" % (a, it)] = np.array(getattr(model, a))

    np.random.seed(seed)
    W0 = np.random.rand(N, F, K)
    H0 = np.random.rand(N, K, T)
    np.random.seed(seed)
    model = FastMultichannelISNMF(n_basis=K, n_sources=N, normalize=normalize, callbacks=[record])
    Y = model(X, iteration=N_ITER)
    assert np.array_equal(model.basis.shape, W0.shape)
    arrays = dict(X=X, seed=np.int64(seed), W0=W0, H0=H0, loss=np.array(model.loss), output=Y,
                  normalize=np.array(normalize if normalize else ""), **snaps)
    assert np.array_equal(Y, snaps["estimation_20"])  # the output is the estimation of the last iteration
    del arrays["estimation_20"]
    return arrays


def save(name, arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, versions=make_golden.VERSIONS, **arrays)
    print("wrote %-40s %8.1f KiB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def generate():
    for idx, (M, N, K, normalize, F, T) in enumerate(CASES):
        save(case_name(M, N, K, normalize), gen_case(M, N, K, normalize, F, T, idx))


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
