"""Golden vectors of ProxLaplaceIVA (bss/iva.py on bss/prox.py), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/` through make_golden; `ASSX_REFERENCE_SRC` overrides
the path).  Per case: `X` (`gradbss_np.mixture`), `W_0` (identity, or the recorded warm start), `norm` as the reference's
svds call returned it, the parameters `C`, `mu1`, `mu2`, `alpha`, `W_<it>` and `y_<it>` after iterations 1, 2, 5 and 10, for
iterations 1 and 2 the stages `G_<it>`, `Wt_<it>`, `z_<it>`, `yt_<it>`, `loss` (11 entries), `output`, `reference_id`,
`projection_back`, `seed`, and `shrink` (10 entries: the share of (n,t) cells that the group shrinkage moves, per
iteration).  The dual is as large as X and ten arrays of that size are recorded, so a case is spread over numbered parts
`<case>.npz`, `<case>.part1.npz`, ..., each below 150 KiB; `pdsbss_np.load_case` puts them together.

The maker asserts: no NumPy warning; every value finite; the reference's front door reproduces its stepwise run bit for
bit (svds starts from a random vector, so the global generator is seeded before either); every prox argument has
sigma_min >= 1e-6 sigma_max; no group norm lies within 1e-6 relative of 1 / mu2; one rounding of X, W0 and the norm moves W and y after the ten
iterations by at most 1e-11 (the restatement's own figure); over the suite at least one case holds
each branch of the shrinkage on >= 5 % of the cells in one recorded iteration and at least one case shrinks >= 90 %.  A
case that fails a condition gets another seed or another mu2, not a weaker condition.  It prints, per case, the largest
entry-wise distance of the restatement tests/pdsbss_np.py from the reference.  No reference source is copied.

    python tests/golden/pdsbss/make_pdsbss.py            # write the files next to this script
    python tests/golden/pdsbss/make_pdsbss.py --verify   # regenerate into a temporary directory and compare
"""
import contextlib
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "gradbss"))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path
import pdsbss_np as pd  # noqa: E402
import pdsbss_envelope_np as penv  # noqa: E402
from make_gradbss import CASES as GRAD_CASES  # noqa: E402
from bss.iva import ProxLaplaceIVA  # noqa: E402

OUT_DIR = HERE
PART_BYTES = 150 * 1024

# (n_channels, n_bins, n_frames, tag, parameters): the ten shapes of the gradient family with the default parameters, then
# the cases with parameters of their own ("tight": mu2 = 4 puts nearly every cell on the shrinking branch; "over": a
# relaxation step above 1; "damped": below 1)
CASES = tuple((M, F, T, tag, {}) for M, F, T, tag in GRAD_CASES) + (
    (5, 6, 40, "tight", dict(regularizer=1.0, step_prox_logdet=1.0, step_prox_penalty=4.0, step=1.0)),
    (3, 6, 50, "over", dict(regularizer=0.7, step_prox_logdet=0.5, step_prox_penalty=2.0, step=1.75)),
    (4, 5, 40, "damped", dict(regularizer=1.3, step_prox_logdet=2.0, step_prox_penalty=0.5, step=0.6)),
)

# case index -> seed: a case that fails one of the maker's conditions gets another seed
SEEDS = {6: 4162}  # (8, 3, 130): the default seed's run moves by 1e-8 under one rounding of its input

MIN_SIGMA_RATIO = 1e-6
MIN_DEN_GAP = 1e-6
MAX_RUN_SENSITIVITY = 1e-11


def case_name(M, F, T, tag):
    return "proxlaplaceiva_m%d_f%d_t%d%s" % (M, F, T, "_" + tag if tag else "")


def elem(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def dense(v, shape):
    return np.asarray(v.toarray()).reshape(shape)


@contextlib.contextmanager
def norm_spy():
    """The singular values that scipy's svds returns while the block runs: the reference's `norm` as it computed it."""
    import scipy.sparse.linalg as sla
    seen, svds = [], sla.svds

    def spy(*args, **kwargs):
        out = svds(*args, **kwargs)
        seen.append(float(out[1][0]))
        return out

    sla.svds = spy
    try:
        yield seen
    finally:
        sla.svds = svds


def spy_on_prox(model):
    """Wraps the model's two prox methods on the instance; the returned dict holds the argument and the result of the
    latest call of each."""
    seen = {}

    def wrap(name, method):
        def spy(arg, *args, **kwargs):
            out = method(arg, *args, **kwargs)
            seen[name + "_in"], seen[name + "_out"] = arg, out
            return out
        return spy

    model.prox_logdet = wrap("logdet", model.prox_logdet)
    model.prox_penalty = wrap("penalty", model.prox_penalty)
    return seen


def gen_case(M, F, T, tag, par, idx):
    seed = SEEDS.get(idx, 4100 + 10 * idx)
    X = pd.mixture(M, F, T, seed)
    rng = np.random.default_rng(seed + 5000)
    W0 = pd.identity(M, F)
    if tag == "warm":
        W0 = W0 + 0.2 * (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M)))
    kw = dict(reference_id=min(1, M - 1), apply_projection_back=tag != "nopb", **par)

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        # stepwise, as the reference's __call__ does it; the stages are what its update hands to its own prox methods
        np.random.seed(seed)
        step = ProxLaplaceIVA(**kw)
        step.input = X
        with norm_spy() as seen:
            step._reset(demix_filter=W0.copy())
        norm = seen[0]
        C, mu1, mu2, alpha = (float(v) for v in (step.regularizer, step.step_prox_logdet, step.step_prox_penalty, step.step))
        seen_prox = spy_on_prox(step)
        snaps, loss, shrink = {"W_0": W0.copy()}, [step.compute_negative_loglikelihood()], []
        for it in range(1, pd.N_ITER + 1):
            y_before = step.y
            adjoint = dense(step.input_sparse.conj().T @ y_before, (F, M, M))  # the operator's adjoint on the dual
            step.update_once()
            loss.append(step.compute_negative_loglikelihood())
            # what the update handed to its two prox steps and got back
            arg, wt = (dense(seen_prox[k], (F, M, M)) for k in ("logdet_in", "logdet_out"))
            z, yt = dense(seen_prox["penalty_in"], (F, M, T)), dense(seen_prox["penalty_in"] - seen_prox["penalty_out"], (F, M, T))
            sv = np.linalg.svd(arg, compute_uv=False)
            assert sv.min(axis=1).min() >= MIN_SIGMA_RATIO * sv.max(), (it, "a prox argument is close to rank-deficient")
            moved, gap = pd.shrinking(z, 1 / mu2)
            assert gap >= MIN_DEN_GAP, (it, "a group norm within %g of 1 / mu2" % gap)
            shrink.append(moved.mean())
            # the stages belong together: the adjoint read off the operator is the one inside the prox argument, and the
            # new dual is the relaxed shrunk z
            assert np.allclose(arg, snaps.get("W_prev", W0) - mu1 * mu2 * adjoint, rtol=0, atol=1e-13 * np.abs(arg).max())
            assert np.array_equal(dense(step.y, (F, M, T)), alpha * yt + (1 - alpha) * dense(y_before, (F, M, T)))
            snaps["W_prev"] = np.array(step.demix_filter)
            if it in pd.STAGE_ITERS:
                snaps["G_%d" % it], snaps["Wt_%d" % it], snaps["z_%d" % it], snaps["yt_%d" % it] = adjoint, wt, z, yt
            if it in pd.SNAP_ITERS:
                snaps["W_%d" % it] = np.array(step.demix_filter)
                snaps["y_%d" % it] = dense(step.y, (F, M, T))

        # the same through the reference's front door
        np.random.seed(seed)
        whole = ProxLaplaceIVA(**kw)
        with norm_spy() as seen:
            output = whole(X, pd.N_ITER, demix_filter=W0.copy())
        assert seen == [norm], "front door and stepwise norms differ"
        assert whole.loss == loss, "front door and stepwise losses differ"
        assert np.array_equal(snaps["W_%d" % pd.N_ITER], whole.demix_filter), "front door and stepwise W differ"
        assert np.array_equal(snaps["y_%d" % pd.N_ITER], dense(whole.y, (F, M, T))), "front door and stepwise y differ"

        del snaps["W_prev"]
        arrays = dict(X=X, seed=np.int64(seed), norm=np.float64(norm), C=np.float64(C), mu1=np.float64(mu1),
                      mu2=np.float64(mu2), alpha=np.float64(alpha), reference_id=np.int64(kw["reference_id"]),
                      projection_back=np.bool_(tag != "nopb"), loss=np.array(loss), shrink=np.array(shrink),
                      output=np.array(output), **snaps)
        for k, v in arrays.items():
            assert np.all(np.isfinite(v)), (k, "not finite")

        # a run that one rounding of its input moves by more than MAX_RUN_SENSITIVITY pins nothing down: h(0) > 0, so the
        # prox turns the two smallest singular directions of its argument with a condition of 2 h / (s1 + s2), per iteration
        moved = penv.trajectory_sensitivity(arrays)
        assert max(moved["W"], moved["y"]) <= MAX_RUN_SENSITIVITY, ("the run is ill-conditioned", moved)

        # the restatement against the reference
        states, rloss, stages = pd.run(X, W0, pd.N_ITER, norm, C, mu1, mu2, alpha)
        dW = max(elem(states[it][0], snaps["W_%d" % it]) for it in pd.SNAP_ITERS)
        dy = max(elem(states[it][1], snaps["y_%d" % it]) for it in pd.SNAP_ITERS)
        ds = max(elem(stages[it][k], snaps["%s_%d" % (k, it)]) for it in pd.STAGE_ITERS for k in pd.STAGES)
        dl = float(np.max(np.abs(np.array(rloss) - loss) / np.abs(loss)))
        do = elem(pd.separate(X, states[pd.N_ITER][0], kw["reference_id"], tag != "nopb"), output)
        dn = abs(pd.operator_norm(X) - norm) / norm
        print("  %-36s restatement: W %.1e, y %.1e, stages %.1e, loss %.1e, output %.1e, norm %.1e; shrink %.2f..%.2f" % (
            case_name(M, F, T, tag), dW, dy, ds, dl, do, dn, min(shrink), max(shrink)))
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
    shares = {}
    for idx, (M, F, T, tag, par) in enumerate(CASES):
        arrays = gen_case(M, F, T, tag, par, idx)
        shares[case_name(M, F, T, tag)] = arrays["shrink"][[it - 1 for it in pd.SNAP_ITERS]]
        save(case_name(M, F, T, tag), arrays)
    # both branches of the shrinkage are taken, and seen: each on >= 5 % of the cells somewhere, shrinking >= 90 % somewhere
    assert any(np.any((s >= 0.05) & (s <= 0.95)) for s in shares.values()), "no case holds both branches on 5 % of the cells"
    assert any(np.any(s >= 0.90) for s in shares.values()), "no case shrinks 90 % of the cells"
    params = [tuple(float(CASES[i][4].get(k, 1.0)) for k in ("regularizer", "step_prox_logdet", "step_prox_penalty", "step"))
              for i in range(len(CASES))]
    assert sum(1 for p in params if p != (1.0, 1.0, 1.0, 1.0)) >= 3 and any(p[3] > 1 for p in params)


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
