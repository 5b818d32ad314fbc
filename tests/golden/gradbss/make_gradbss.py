"""Golden vectors of the gradient family (bss/iva.py, bss/fdica.py), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/` through make_golden; `ASSX_REFERENCE_SRC` overrides
the path).  One file per class and case: `X` (a seeded convolutive Laplacian mixture of unit mean power,
`gradbss_np.mixture`), `W_0` (identity, or the recorded warm start), `W_<it>` after iterations 1, 2, 5 and 10, `loss` (11
entries: before the loop and after every iteration), `output`, `lr`, `eps`, `reference_id`, `projection_back`, `seed`;
for FDICA also `W_pre` (= W_10, before the solver), `order`, `perm`, `W_post` and `gaps` (the smallest relative gap
between neighbouring sorted correlations, the smallest relative gap between the best and the second-best permutation
score of a bin).

The maker asserts: no NumPy warning; every value finite; every |det W_f| at least 1e-6 of its largest; every floored
denominator at least 1e6 eps; the reference's front door reproduces its stepwise run bit for bit; for FDICA both gaps at
least 1e-8.  A case that fails a condition gets another seed (SEEDS), not a wider condition.  It prints, per file, the
largest entry-wise distance of the restatement tests/gradbss_np.py from the reference.  No reference source is copied.

    python tests/golden/gradbss/make_gradbss.py            # write the files next to this script
    python tests/golden/gradbss/make_gradbss.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path
import gradbss_np as gb  # noqa: E402
from bss.iva import GradLaplaceIVA, NaturalGradLaplaceIVA  # noqa: E402
from bss.fdica import GradLaplaceFDICA, NaturalGradLaplaceFDICA  # noqa: E402

OUT_DIR = HERE
REFERENCE = {"GradLaplaceIVA": GradLaplaceIVA, "NaturalGradLaplaceIVA": NaturalGradLaplaceIVA,
             "GradLaplaceFDICA": GradLaplaceFDICA, "NaturalGradLaplaceFDICA": NaturalGradLaplaceFDICA}

# (n_channels, n_bins, n_frames, tag); tag "warm": a recorded non-identity demix_filter, "nopb": IVA only, without
# projection back
CASES = (
    (2, 5, 33, ""), (3, 4, 70, ""), (4, 6, 64, ""), (5, 3, 48, ""), (6, 2, 40, ""), (7, 2, 40, ""), (8, 3, 130, ""),
    (2, 4, 257, ""),     # frames cross 256
    (3, 4, 50, "warm"),
    (3, 5, 45, "nopb"),
)

# (class, case index) -> seed: a case that fails one of the maker's conditions gets another seed
SEEDS = {}

MIN_DET_RATIO = 1e-6
MIN_DENOMINATOR = 1e6 * gb.EPS
MIN_GAP = 1e-8


def case_name(cls, M, F, T, tag):
    return "%s_m%d_f%d_t%d%s" % (cls, M, F, T, "_" + tag if tag else "")


def elem(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)))


def check_state(model, X, W, tag):
    det = np.abs(np.linalg.det(W))
    assert det.min() >= MIN_DET_RATIO * det.max(), (tag, "|det W| spans %g" % (det.min() / det.max()))
    low = gb.smallest_denominator(model, X, W)
    assert low >= MIN_DENOMINATOR, (tag, "a denominator of %g" % low)


def gen_case(cls, M, F, T, tag, idx):
    model, natural = gb.CLASSES[cls]
    if tag == "nopb" and model != "iva":
        return None
    seed = SEEDS.get((cls, idx), 3100 + 10 * idx + sorted(gb.CLASSES).index(cls))
    X = gb.mixture(M, F, T, seed)
    rng = np.random.default_rng(seed + 5000)
    W0 = gb.identity(M, F)
    if tag == "warm":
        W0 = W0 + 0.2 * (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M)))
    kw = dict(lr=gb.LR, reference_id=min(1, M - 1), eps=gb.EPS)
    if model == "iva":
        kw["apply_projection_back"] = tag != "nopb"

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        # stepwise, as the reference's __call__ does it
        step = REFERENCE[cls](**kw)
        step.input = X
        step._reset(demix_filter=W0.copy())
        snaps, loss = {"W_0": W0.copy()}, [step.compute_negative_loglikelihood()]
        for it in range(1, gb.N_ITER + 1):
            step.update_once()
            loss.append(step.compute_negative_loglikelihood())
            if it in gb.SNAP_ITERS:
                snaps["W_%d" % it] = np.array(step.demix_filter)

        # the same through the reference's front door
        whole = REFERENCE[cls](**kw)
        output = whole(X, iteration=gb.N_ITER, demix_filter=W0.copy())
        assert whole.loss == loss, "front door and stepwise losses differ"

        arrays = dict(X=X, seed=np.int64(seed), lr=np.float64(gb.LR), eps=np.float64(gb.EPS),
                      reference_id=np.int64(kw["reference_id"]), projection_back=np.bool_(tag != "nopb"),
                      loss=np.array(loss), output=np.array(output), **snaps)
        if model == "fdica":
            step.solve_permutation()
            arrays["W_pre"] = snaps["W_%d" % gb.N_ITER]
            arrays["W_post"] = np.array(step.demix_filter)
            assert np.array_equal(arrays["W_post"], whole.demix_filter), "front door and stepwise solver differ"
            Wn, order, perm, gaps = gb.solve_permutation(X, arrays["W_pre"], gb.EPS)
            arrays["order"], arrays["perm"], arrays["gaps"] = order, perm, np.array(gaps)
            assert min(gaps) >= MIN_GAP, ("gaps", gaps)
            # the recorded integers are the reference's: its permuted rows are exact copies of the rows they name
            assert np.array_equal(Wn, arrays["W_post"]), "the restatement's solver and the reference's differ"
            assert all(np.array_equal(arrays["W_post"][f], arrays["W_pre"][f][perm[f]]) for f in range(F))
        else:
            assert np.array_equal(snaps["W_%d" % gb.N_ITER], whole.demix_filter), "front door and stepwise W differ"

        for k, v in arrays.items():
            assert np.all(np.isfinite(v)), (k, "not finite")
        for it in (0,) + gb.SNAP_ITERS:
            check_state(model, X, snaps["W_%d" % it], "%s W_%d" % (cls, it))

        # the restatement against the reference
        states, rloss = gb.run(model, natural, X, W0, gb.N_ITER, gb.LR, gb.EPS)
        d = max(elem(states[it], snaps["W_%d" % it]) for it in gb.SNAP_ITERS)
        dl = elem(rloss, loss)
        Wf = arrays["W_post"] if model == "fdica" else states[gb.N_ITER]
        do = elem(gb.separate(X, Wf, kw["reference_id"], tag != "nopb"), output)
        print("  %-40s restatement: W %.1e, loss %.1e, output %.1e%s" % (
            case_name(cls, M, F, T, tag), d, dl, do,
            "  gaps %.1e %.1e" % tuple(arrays["gaps"]) if model == "fdica" else ""))
    return arrays


def save(name, arrays):
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, versions=make_golden.VERSIONS, **arrays)
    size = os.path.getsize(path)
    assert size < 150 * 1024, (name, size)
    print("wrote %-44s %8.1f KiB" % (os.path.basename(path), size / 1024))


def generate():
    for cls in sorted(gb.CLASSES):
        for idx, case in enumerate(CASES):
            arrays = gen_case(cls, *case, idx)
            if arrays is not None:
                save(case_name(cls, *case), arrays)


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
