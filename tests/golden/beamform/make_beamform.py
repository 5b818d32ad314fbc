"""Golden vectors of the closed-form spatial filters (bss/beamform.py, transform/pca.py,
algorithm/minimum_distortion_principle.py), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/` through make_golden, which also holds the NumPy-1
`solve` shim the reference's AuxIVA needs; `ASSX_REFERENCE_SRC` overrides the path).  Per case: the inputs `X`
(`beamform_np.mixture`), steering vectors `A`, a non-Hermitian `R`, sources `Ys`, `reference_id`, `eps`, and what the
reference returned: `ds`, `ml`, `mvdr`, `pca`, `mdp2` (2-D reference X[reference_id]) and `mdp3` (3-D reference X);
`pca_w`, the eigenvalues of the covariance the reference's pca forms (numpy.linalg.eigvalsh of its own expression), and
`floored` (F,N), where the ML denominator was replaced.  The tagged cases: "floor" holds a bin whose R makes every
denominator negative, so that it is floored; "silent" holds a source bin of zeros, whose MDP scale is NaN; "fewframes"
(T < M) and "dup" (a duplicated channel) are the degenerate PCA inputs that are compared on invariants only; "chain" is
pca(x)[:2] -> AuxLaplaceIVA(apply_projection_back=False), 5 iterations -> projection_back against x[0].  A case is
spread over numbered parts below 150 KiB; `beamform_np.load_case` puts them together.

The maker asserts: every value finite except the silent bin's scales; outside the degenerate cases every bin's smallest
eigenvalue gap is at least 1e-3 of its largest eigenvalue and T >= 4 M; the floored bin is floored and no other is.  It
prints, per case, the largest entry-wise distance of the restatement tests/beamform_np.py from the reference.  No
reference source is copied.

    python tests/golden/beamform/make_beamform.py            # write the files next to this script
    python tests/golden/beamform/make_beamform.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path, the NumPy-1 solve shim
import beamform_np as bf  # noqa: E402
from bss.beamform import delay_sum_beamform, ml_beamform, mvdr_beamform  # noqa: E402
from bss.iva import AuxLaplaceIVA  # noqa: E402
from transform.pca import pca  # noqa: E402
from algorithm.minimum_distortion_principle import minimum_distortion_principle  # noqa: E402
from algorithm.projection_back import projection_back  # noqa: E402

OUT_DIR = HERE
PART_BYTES = 150 * 1024
MIN_GAP = 1e-3
DEGENERATE = ("fewframes", "dup")

# (n_channels, n_sources, n_bins, n_frames, reference_id, tag): every M in 2..8; N < M, N == M and N > M
CASES = (
    (2, 3, 5, 33, 1, ""),
    (3, 2, 4, 70, 2, ""),
    (4, 4, 6, 64, 0, ""),
    (5, 1, 3, 48, 4, ""),
    (6, 8, 2, 40, 3, ""),
    (7, 7, 2, 40, 6, ""),
    (8, 2, 3, 130, 5, ""),
    (3, 2, 4, 50, 0, "floor"),
    (4, 3, 5, 45, 1, "silent"),
    (4, 2, 3, 2, 0, "fewframes"),
    (5, 2, 3, 40, 0, "dup"),
    (3, 2, 5, 70, 0, "chain"),
)


def case_name(M, N, F, T, tag):
    return "beamform_m%d_n%d_f%d_t%d%s" % (M, N, F, T, "_" + tag if tag else "")


def elem(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.nanmax(np.abs(a - b)) / max(np.nanmax(np.abs(b)), 1e-300))


def gen_case(M, N, F, T, ref, tag, idx):
    seed = 7100 + 10 * idx
    rng = np.random.default_rng(seed + 5000)
    X = bf.mixture(M, F, T, seed)
    if tag == "dup":
        X[M - 1] = X[0]
    A = bf.steering(F, M, N, seed + 1)
    G = bf.cgauss(rng, (F, M, M))
    R = G @ G.conj().transpose(0, 2, 1) / M + 0.5 * np.eye(M) + 0.2 * bf.cgauss(rng, (F, M, M))  # not Hermitian
    if tag == "floor":
        R[1] = -(G[1] @ G[1].conj().T / M + 0.5 * np.eye(M))  # every denominator of bin 1 is negative
    Ys = bf.cgauss(rng, (N, F, T)) * (0.5 + rng.random((N, F, 1)))
    if tag == "silent":
        Ys[1, 2] = 0.0
    eps = 1e-12

    if tag not in DEGENERATE:
        assert T >= 4 * M and bf.eigen_gap(X) >= MIN_GAP, (case_name(M, N, F, T, tag), bf.eigen_gap(X))
    arrays = dict(X=X, A=A, R=R, Ys=Ys, reference_id=np.int64(ref), eps=np.float64(eps), seed=np.int64(seed))
    arrays["ds"] = delay_sum_beamform(X, A, reference_id=ref)
    arrays["ml"] = ml_beamform(X, A, R.copy(), reference_id=ref, eps=eps)
    arrays["pca"] = pca(X)
    Xt = X.transpose(1, 2, 0)
    arrays["pca_w"] = np.linalg.eigvalsh(np.mean(Xt[:, :, :, None] * Xt[:, :, None, :].conj(), axis=1))
    if tag not in DEGENERATE:  # their covariance is singular: the reference's inverse is noise or a LinAlgError
        arrays["mvdr"] = mvdr_beamform(X, A, reference_id=ref, eps=eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        arrays["mdp2"] = minimum_distortion_principle(Ys, X[ref])
        arrays["mdp3"] = minimum_distortion_principle(Ys, X)
    _, below = bf.floored(np.sum(A.conj() * (np.linalg.inv(R) @ A), axis=1), eps)
    arrays["floored"] = below
    assert below[1].all() and not np.delete(below, 1, axis=0).any() if tag == "floor" else not below.any()
    if tag == "chain":
        est = AuxLaplaceIVA(algorithm_spatial="IP", apply_projection_back=False)(pca(X)[:2], iteration=5)
        arrays["chain"] = est * projection_back(est, X[0])[..., None]
    for k, v in arrays.items():
        if k in ("mdp2", "mdp3") and tag == "silent":
            nan = np.isnan(v)
            assert nan.any() and nan.sum() == (1 if k == "mdp2" else M), k
            assert np.all(np.isfinite(v[~nan]))
        else:
            assert np.all(np.isfinite(v)), (k, "not finite")

    # the restatement against the reference
    d = {"ds": elem(bf.delay_sum(X, A, ref), arrays["ds"]), "ml": elem(bf.ml(X, A, R, ref, eps), arrays["ml"]),
         "pca": elem(bf.align_phase(bf.pca(X), arrays["pca"]), arrays["pca"]) if tag not in DEGENERATE else float("nan"),
         "w": elem(bf.pca_basis(X)[1], arrays["pca_w"]),
         "mdp": max(elem(bf.mdp(Ys, X[ref]), arrays["mdp2"]), elem(bf.mdp(Ys, X), arrays["mdp3"]))}
    if "mvdr" in arrays:
        d["mvdr"] = elem(bf.mvdr(X, A, ref, eps), arrays["mvdr"])
    if tag == "chain":
        d["chain"] = elem(bf.chain(X), arrays["chain"])
    print("  %-34s restatement: %s" % (case_name(M, N, F, T, tag), ", ".join("%s %.1e" % kv for kv in d.items())))
    return arrays


def save(name, arrays):
    """Numbered parts, each below PART_BYTES: the arrays in insertion order, a new part when the next one would not fit."""
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        nb = np.asarray(v).nbytes + 256
        if cur and size + nb > PART_BYTES - 8192:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += nb
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(OUT_DIR, name + (".part%d" % i if i else "") + ".npz")
        extra = dict(versions=make_golden.VERSIONS, n_parts=np.int64(len(parts))) if i == 0 else {}
        np.savez_compressed(path, **extra, **part)
        size = os.path.getsize(path)
        assert size < PART_BYTES, (path, size)
        print("wrote %-52s %8.1f KiB" % (os.path.basename(path), size / 1024))


def generate():
    for idx, (M, N, F, T, ref, tag) in enumerate(CASES):
        save(case_name(M, N, F, T, tag), gen_case(M, N, F, T, ref, tag, idx))
    assert {c[0] for c in CASES if not c[5]} == set(range(2, 9))
    assert any(c[1] < c[0] for c in CASES) and any(c[1] == c[0] for c in CASES) and any(c[1] > c[0] for c in CASES)
    assert any(c[4] != 0 for c in CASES)


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
