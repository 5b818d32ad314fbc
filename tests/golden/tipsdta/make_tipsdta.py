"""Golden vectors of tIPSDTA (author='Kondo'), made by running the *reference* itself.

Runs only where the reference tree is present (it imports its `src/`; `ASSX_REFERENCE_SRC` overrides the path).  Each
case file holds a seeded convolutive mixture X (n_channels, n_bins, n_frames), the seed of the global NumPy RNG the
reference draws from, the draws themselves (`draw_Ul`, `draw_Uh`, or `draw_U` without remains, then `draw_H`), `rng_next` =
the next np.random.rand() after them, `eps`, `nu`, `normalize`, `n_basis`, `n_blocks`, `spatial_iteration`, and the state
(`W_<tag>`, the basis as `Ul_<tag>` and `Uh_<tag>` or as `U_<tag>`, `H_<tag>`) at the tags `0` (the start, after the
reference's reset), `src1` (after the source update of iteration 1), `sw1_<s>` (after sweep s of iteration 1) and `1`, `2`,
`4`, `5`, `9`, `10` (after these iterations), `loss` (11,: the entry before the loop and one per iteration) and `out`, the
output of the front-door call.

The maker asserts that no NumPy warning is raised, that every recorded value is finite, that cond(R) <= 1e4 for every
(source, frame, block) at every recorded state, that every activation entry is at least 1e-8 of its row maximum, that at
every VCD step recomputed by the restatement (tests/tipsdta_np.py) at the recorded states |eta_hat| of a block of more than
one bin is at least 1e-6 or exactly 0 (a diagonal model, as at the start: gamma is exactly 0 there) and that no numerator
or denominator of the activation update is floored there, that the loss does not increase, and that the reference's front
door reproduces the stepwise run bit for bit.  No reference source is copied.

    python tests/golden/tipsdta/make_tipsdta.py            # write the files next to this script
    python tests/golden/tipsdta/make_tipsdta.py --verify   # regenerate into a temporary directory and compare
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  reference on sys.path, the NumPy 2 `solve` shim
import ipsdta_np as ip  # noqa: E402
import tipsdta_np as tp  # noqa: E402
from bss.ipsdta import tIPSDTA  # noqa: E402

OUT_DIR = HERE

# (n_channels, n_bins, n_frames, n_basis, n_blocks, spatial_iteration, normalize, nu)
CASES = (
    (2, 9, 64, 2, 4, 2, True, 1),       # sizes 2 and 3
    (2, 5, 64, 2, 4, 2, True, 1),       # sizes 1 and 2, the default's shape
    (3, 11, 96, 3, 3, 2, True, 1),      # sizes 3 and 4
    (4, 13, 96, 2, 5, 2, True, 1),      # sizes 2 and 3, three high blocks
    (2, 16, 128, 2, 2, 2, True, 1),     # size 8, the cap
    (2, 15, 128, 2, 2, 2, True, 1),     # sizes 7 and 8
    (2, 6, 64, 2, 1, 2, True, 1),       # one block
    (2, 8, 128, 10, 2, 2, True, 1),     # the default n_basis
    (2, 6, 64, 2, 6, 2, True, 1),       # all blocks of one bin
    (2, 4, 257, 2, 2, 2, True, 1),      # frames cross 256
    (2, 12, 64, 2, 3, 10, True, 1),     # the default spatial_iteration
    (2, 12, 64, 2, 3, 2, False, 1),     # no normalisation
    (2, 12, 64, 2, 3, 2, True, 1000),   # nearly Gaussian
    (2, 12, 64, 2, 3, 2, True, 0.5),    # a heavier tail than the default
    (8, 6, 160, 2, 3, 2, True, 4),      # n_channels at the cap
    (2, 6, 48, 64, 3, 2, True, 1),      # n_basis at the cap
)

# a case that fails one of the maker's conditions gets another seed, the reason next to it (at most three)
SEEDS = {}


def case_name(M, F, T, K, nblk, sp, norm, nu):
    tail = ("" if norm else "_nonorm") + ("" if nu == 1 else "_nu%g" % nu)
    return "tipsdta_m%d_f%d_t%d_k%d_b%d_s%d%s" % (M, F, T, K, nblk, sp, tail)


def snapshot(model, tag, out):
    out["W_%s" % tag] = np.array(model.demix_filter)
    if isinstance(model.basis, tuple):
        out["Ul_%s" % tag], out["Uh_%s" % tag] = np.array(model.basis[0]), np.array(model.basis[1])
    else:
        out["U_%s" % tag] = np.array(model.basis)
    out["H_%s" % tag] = np.array(model.activation)


def check_state(X, fx, tag, eps, nblk, nu):
    W, basis, H = ip.state(fx, tag)
    what = "state %s" % tag
    assert np.all(H >= 1e-8 * np.max(H, axis=2, keepdims=True)), (what, "an activation entry below 1e-8 of its row")
    cond = ip.max_cond(basis, H, eps)
    assert cond <= 1e4, (what, "cond(R) = %g" % cond)
    diag = {}
    tp.update_activation(X, W, basis, H, eps, nblk, nu, diag=diag)
    assert not diag["num_floored"] and not diag["den_floored"], (what, diag)
    tp.update_spatial(X, W, basis, H, eps, nblk, nu, 1, diag=diag)
    assert diag.get("eta_hat_min", np.inf) >= 1e-6, (what, "|eta_hat| = %g" % diag["eta_hat_min"])


def gen_case(M, F, T, K, nblk, sp, norm, nu, idx):
    seed = SEEDS.get(idx, 2700 + idx)
    eps = 1e-12
    X = ip.mixture(M, F, T, seed)
    nn, nlow, rem = ip.geometry(F, nblk)
    np.random.seed(seed)
    draws = {}
    if rem > 0:
        draws["draw_Ul"] = np.random.rand(M, K, nlow, nn)
        draws["draw_Uh"] = np.random.rand(M, K, rem, nn + 1)
    else:
        draws["draw_U"] = np.random.rand(M, K, nblk, nn)
    draws["draw_H"] = np.random.rand(M, K, T)
    rng_next = np.random.rand()

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a NumPy warning means the case left the region the tests describe
        np.random.seed(seed)
        # the reference's constructor overwrites its `spatial_iteration` argument with the default of 10 (ipsdta.py:1104-1105):
        # the number of sweeps is given at the call, whose keywords become attributes
        model = tIPSDTA(n_basis=K, nu=nu, normalize=norm, eps=eps, n_blocks=nblk)
        model.input = X
        model._reset(spatial_iteration=sp)
        snaps, loss = {}, [model.compute_negative_loglikelihood()]
        snapshot(model, "0", snaps)
        for it in range(1, ip.N_ITER + 1):
            model.update_source_model()
            if it == 1:
                snapshot(model, "src1", snaps)
            for s in range(sp):
                model.update_spatial_model()
                if it == 1:
                    snapshot(model, "sw1_%d" % (s + 1), snaps)
            loss.append(model.compute_negative_loglikelihood())
            if it in ip.SNAP_ITERS:
                snapshot(model, str(it), snaps)

        # the same through the reference's front door
        np.random.seed(seed)
        whole = tIPSDTA(n_basis=K, nu=nu, normalize=norm, eps=eps, n_blocks=nblk)
        out = whole(X, iteration=ip.N_ITER, spatial_iteration=sp)
        assert np.random.rand() == rng_next
        final = {}
        snapshot(whole, "10", final)
        assert all(np.array_equal(final[k], snaps[k]) for k in final) and whole.loss == loss

        arrays = dict(X=X, seed=np.int64(seed), eps=np.float64(eps), nu=np.float64(nu), normalize=np.bool_(norm), n_basis=np.int64(K),
                      n_blocks=np.int64(nblk), spatial_iteration=np.int64(sp), rng_next=np.float64(rng_next),
                      loss=np.array(loss), out=np.array(out), **draws, **snaps)
        for k, v in arrays.items():
            assert np.all(np.isfinite(v)), (k, "not finite")
        for tag in ["0", "src1"] + ["sw1_%d" % (s + 1) for s in range(sp)] + [str(i) for i in ip.SNAP_ITERS]:
            check_state(X, arrays, tag, eps, nblk, nu)
        loss = np.array(loss)
        assert np.all(np.diff(loss) <= 1e-9 * (np.abs(loss[:-1]) + M * F * T)), "the loss went up"
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
