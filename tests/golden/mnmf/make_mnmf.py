"""Golden vectors of MultichannelISNMF (Sawada's full-rank MNMF), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  Each
case file holds a seeded mixture, the seed of the global NumPy RNG the reference draws latent, basis and activation
from (in that order), the initial latent, basis and activation, the state after iterations 1, 2, 5 and 20 (basis, activation, latent,
spatial, estimation), the loss list and the output.  `riccati.npz` holds a batch of random `solve_Riccati` inputs and
outputs per channel count.  No reference source is copied.

    python tests/golden/mnmf/make_mnmf.py            # write the files next to this script
    python tests/golden/mnmf/make_mnmf.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  NumPy-2 `solve` shim, reference on sys.path, convolutive_mixture
from bss.mnmf import MultichannelISNMF  # noqa: E402
from algorithm.linalg import solve_Riccati  # noqa: E402

OUT_DIR = HERE
SNAP_ITERS = (1, 2, 5, 20)
N_ITER = 20
ATTRS = ("basis", "activation", "latent", "spatial", "estimation")

# (M, N, K, normalize, F, T, silent): `silent` zeroes one bin and four frames of the mixture
CASES = (
    (2, 2, 3, True, 17, 128, False),
    (3, 2, 4, True, 17, 128, False),
    (3, 3, 20, True, 17, 96, False),
    (4, 3, 5, False, 17, 96, False),
    (4, 4, 10, True, 13, 96, False),
    (2, 3, 4, True, 17, 96, False),
    (8, 4, 2, True, 9, 64, False),
    (3, 2, 4, True, 17, 96, True),
    # the corners of the size envelope (appended: the seeds and bytes of the files above do not change).  F and T of
    # the last one were picked by the restatement's own sensitivity: at T = 96 a one-ulp change of the initial basis
    # moves the spatial model by 4e-11 after 5 iterations (restatement against itself), at T = 100 by 1e-14.
    (5, 5, 17, True, 9, 100, False),
    (6, 7, 33, True, 7, 80, False),
    (7, 8, 64, True, 5, 65, False),
    (3, 1, 4, True, 9, 100, False),
    (8, 2, 20, True, 9, 100, False),
)
RICCATI_M = (2, 3, 4, 5, 6, 7, 8)
RICCATI_BATCH = 16


def case_name(M, N, K, normalize, silent):
    return "mnmf_m%d_n%d_k%d%s%s" % (M, N, K, "" if normalize else "_nonorm", "_silent" if silent else "")


def gen_case(M, N, K, normalize, F, T, silent, idx):
    seed = 1300 + idx
    X = make_golden.convolutive_mixture(M, F, T, seed=seed)
    if silent:
        X[:, 3, :] = 0
        X[:, :, 10:14] = 0
    snaps = {}

    def record(model):
        it = len(model.loss) - 1
        if it in SNAP_ITERS:
            for a in ATTRS:
                snaps["%s_%d" % (a, it)] = np.array(getattr(model, a))

    np.random.seed(seed)
    Z0 = np.random.rand(N, K) * 1e-2 + 1 / N  # the reference's latent before its normalisation over sources
    Z0 = Z0 / np.maximum(Z0.sum(axis=0), 1e-12)
    T0 = np.random.rand(F, K)
    V0 = np.random.rand(K, T)
    np.random.seed(seed)
    model = MultichannelISNMF(n_basis=K, n_sources=N, normalize=normalize, callbacks=[record])
    Y = model(X, iteration=N_ITER)
    assert model.basis.shape == T0.shape
    arrays = dict(X=X, seed=np.int64(seed), Z0=Z0, T0=T0, V0=V0, loss=np.array(model.loss), output=Y,
                  normalize=np.array(bool(normalize)), **snaps)
    assert np.array_equal(Y, snaps["estimation_20"])  # the output is the estimation of the last iteration
    del arrays["estimation_20"]
    return arrays


def gen_riccati():
    rng = np.random.default_rng(1399)
    arrays = {}
    for M in RICCATI_M:
        G = rng.standard_normal((RICCATI_BATCH, M, M)) + 1j * rng.standard_normal((RICCATI_BATCH, M, M))
        A = G @ G.conj().swapaxes(-1, -2) + 1e-3 * np.eye(M)
        G = rng.standard_normal((RICCATI_BATCH, M, M)) + 1j * rng.standard_normal((RICCATI_BATCH, M, M))
        B = G @ G.conj().swapaxes(-1, -2)
        arrays["A_%d" % M], arrays["B_%d" % M] = A, B
        arrays["H_%d" % M] = solve_Riccati(A[None], B[None])[0]  # the reference sorts along axis 2
    return arrays


def save(name, arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, versions=make_golden.VERSIONS, **arrays)
    print("wrote %-40s %8.1f KiB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def generate():
    for idx, (M, N, K, normalize, F, T, silent) in enumerate(CASES):
        save(case_name(M, N, K, normalize, silent), gen_case(M, N, K, normalize, F, T, silent, idx))
    save("riccati", gen_riccati())


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
