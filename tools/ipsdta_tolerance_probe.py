#!/usr/bin/env python3
"""Measure the tolerances of the GaussIPSDTA tests (--model gauss) or the tIPSDTA tests (--model t) and write
tests/golden/ipsdta/tolerances.json or tests/golden/tipsdta/tolerances.json (CPU, NumPy only).

Runs where the reference tree is present, like tests/golden/ipsdta/make_ipsdta.py.  Metrics (tests/ipsdta_np.py): W, per bin
max|a - b| / max|b|; U, per (source, basis) max|a - b| / max|b| over all its blocks; H, entry-wise |a - b| / |b|; loss,
|a - b| / (|b| + N n_bins n_frames); out, per source max|a - b| / max|b|.  For every fixture three things are measured
against the reference:

  restatement   tests/ipsdta_np.py (the t model: tests/tipsdta_np.py) on numpy.linalg, every psd() by its definition
  kernel model  the same module on the NumPy models of what the kernels do differently (Cholesky inverse, cyclic Jacobi,
                the Cholesky shortcut of psd, min(lambda_min, 0) = 0 in the psd of x x^H and of y y^H + eps I, log|det W|
                from an LU): the difference between the two rows is what these choices cost
  sensitivity   the reference against itself after every real and imaginary part of what the step reads (X, W, the bases --
                kept Hermitian -- and H) moved to a neighbouring double (the largest of N_DRAWS draws of the directions)

`one_stage`: the source update from the start, every sweep of iteration 1 from the recorded state before it, the loss of a
recorded state and the projected output of the final W.  `one_iteration`: from every recorded state whose successor is
recorded.  `whole_run`: 10 iterations from the start, compared at iteration 10 (the loss: the largest figure over the whole
list).  Each is the largest figure over all fixtures, per metric.  A tolerance is FACTOR x the largest of the three
figures, and at least FACTOR x 2^-52.  A one-stage tolerance above LIMIT means the restatement is not the reference's
update: nothing is written then.

    python tools/ipsdta_tolerance_probe.py --model gauss|t            # writes tolerances.json
    python tools/ipsdta_tolerance_probe.py --model gauss|t --check    # measures and compares with the committed file
    python tools/ipsdta_tolerance_probe.py --envelope                 # the d tables of tests/ipsdta_envelope_np.py

`--envelope` needs neither the reference tree nor a fixture: over the grid of tests/ipsdta_envelope_np.py and for both
models it measures, per entry point, the LAPACK restatement against the restatement on the kernels' algorithms and against
itself after a one-ulp move of everything it reads (ipsdta_envelope_np.measure), prints the figures per case and the
tables D and D_BASIS_SINGLE_FRAME as that module commits them, and compares them with the committed ones.

Below, nu is None for the Gauss model and the fixture's degree of freedom for the t model; the restatements take it after
n_blocks.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402

import ipsdta_np as ip  # noqa: E402
import tipsdta_np as tp  # noqa: E402

GaussIPSDTA = tIPSDTA = projection_back = None  # the reference's, bound by load_reference()

FACTOR = 16
LIMIT = 1e-9
RESOLUTION = 2.0 ** -52
N_DRAWS = 3


def load_reference():
    global GaussIPSDTA, tIPSDTA, projection_back
    import make_golden  # noqa: F401  reference on sys.path
    from bss.ipsdta import GaussIPSDTA, tIPSDTA
    from algorithm.projection_back import projection_back


def restatement(nu):
    """The NumPy module of the model and what its functions take after n_blocks."""
    return (ip, ()) if nu is None else (tp, (nu,))


def reference_model(X, W, basis, H, eps, norm, nblk, sp, nu):
    """The reference at a given state, without its reset (which would draw, copy and normalise)."""
    M, F, T = X.shape
    if nu is None:
        m = GaussIPSDTA(n_basis=H.shape[1], normalize=norm, eps=eps, n_blocks=nblk)
    else:
        m = tIPSDTA(n_basis=H.shape[1], nu=nu, normalize=norm, eps=eps, n_blocks=nblk)
    m.spatial_iteration = sp
    m.input = X
    m.n_sources = m.n_channels = M
    m.n_bins, m.n_frames = F, T
    m.n_neighbors, m.n_remains = F // nblk, F % nblk
    m.demix_filter = W.copy()
    # the reference keeps a basis as a transposed view of a (N, K, n, nb, nb) array; the memory order decides how NumPy sums
    parts = [p.transpose(0, 2, 3, 4, 1) for p in ip.to_parts(basis)]
    m.basis = parts[0] if m.n_remains == 0 else tuple(parts)
    m.activation = H.copy()
    return m


def model_state(m):
    b = m.basis
    return m.demix_filter.copy(), (tuple(np.array(p) for p in b) if isinstance(b, tuple) else np.array(b)), \
        m.activation.copy()


def reference_output(X, W, reference_id=0):
    Y = GaussIPSDTA.separate(None, X, demix_filter=W)  # the t model inherits it
    return Y * projection_back(Y, reference=X[reference_id])[..., np.newaxis]


def perturbed(X, W, basis, H, seed):
    rng = np.random.default_rng(seed)
    return ip.one_ulp(X, rng), ip.one_ulp(W, rng), ip.herm_ulp(basis, rng), ip.one_ulp(H, rng)


def raise_to(total, figures):
    for k, v in figures.items():
        total[k] = max(total.get(k, 0.0), float(v))


def model_figures(got, want):
    return {"W": ip.w_metric(got[0], want[0]), "U": ip.basis_metric(got[1], want[1]), "H": ip.h_metric(got[2], want[2])}


def reference_iterations(X, W, basis, H, eps, norm, nblk, sp, nu, n):
    m = reference_model(X, W, basis, H, eps, norm, nblk, sp, nu)
    losses = []
    for _ in range(n):
        m.update_once()
        losses.append(float(m.compute_negative_loglikelihood()))
    return model_state(m), losses


def restated_iterations(X, W, basis, H, eps, norm, nblk, sp, nu, n, la):
    rs, ex = restatement(nu)
    losses = []
    for _ in range(n):
        W, basis, H, loss = rs.iterate(X, W, basis, H, eps, nblk, *ex, sp, norm, la)
        losses.append(loss)
    return (W, basis, H), losses


def probe_fixture(fx, name):
    X, eps, norm = fx["X"], float(fx["eps"]), bool(fx["normalize"])
    M, F, T, K, nblk, sp = ip.dims(fx)
    nu = float(fx["nu"]) if "nu" in fx else None
    rs, ex = restatement(nu)
    own = {"one_stage": {}, "one_iteration": {}, "whole_run": {}}
    stage = own["one_stage"]

    # ---- the source update from the start
    W, U, H = ip.state(fx, 0)
    m = reference_model(X, W, U, H, eps, norm, nblk, sp, nu)
    m.update_source_model()
    ref = model_state(m)
    want = ip.state(fx, "src1")
    assert all(np.array_equal(a, b) for a, b in zip(ip.to_parts(ref[1]), ip.to_parts(want[1]))), (name, "src1 U")
    assert np.array_equal(ref[2], want[2]), (name, "src1 H")
    for la in (ip.LAPACK, ip.KERNEL):
        Un, Hn = rs.update_source(X, W, U, H, eps, nblk, *ex, norm, la)
        raise_to(stage, {"U": ip.basis_metric(Un, ref[1]), "H": ip.h_metric(Hn, ref[2])})
    for d in range(N_DRAWS):
        Xp, Wp, Up, Hp = perturbed(X, W, U, H, d)
        m = reference_model(Xp, Wp, Up, Hp, eps, norm, nblk, sp, nu)
        m.update_source_model()
        got = model_state(m)
        raise_to(stage, {"U": ip.basis_metric(got[1], ref[1]), "H": ip.h_metric(got[2], ref[2])})

    # ---- every sweep of iteration 1
    tags = ["src1"] + ["sw1_%d" % (s + 1) for s in range(sp)]
    for a, b in zip(tags[:-1], tags[1:]):
        W, U, H = ip.state(fx, a)
        m = reference_model(X, W, U, H, eps, norm, nblk, sp, nu)
        m.update_spatial_model()
        assert np.array_equal(m.demix_filter, fx["W_%s" % b]), (name, b)
        for la in (ip.LAPACK, ip.KERNEL):
            raise_to(stage, {"W": ip.w_metric(rs.update_spatial(X, W, U, H, eps, nblk, *ex, 1, la), m.demix_filter)})
        for d in range(N_DRAWS):
            mp = reference_model(*perturbed(X, W, U, H, 10 + d), eps, norm, nblk, sp, nu)
            mp.update_spatial_model()
            raise_to(stage, {"W": ip.w_metric(mp.demix_filter, m.demix_filter)})

    # ---- the loss and the output
    for it in (0, 1, 10):
        W, U, H = ip.state(fx, it)
        m = reference_model(X, W, U, H, eps, norm, nblk, sp, nu)
        ref_loss = float(m.compute_negative_loglikelihood())
        assert ref_loss == fx["loss"][it], (name, "loss", it)
        for la in (ip.LAPACK, ip.KERNEL):
            raise_to(stage, {"loss": ip.loss_metric(rs.loss(X, W, U, H, eps, nblk, *ex, la), ref_loss, M, F, T)})
        for d in range(N_DRAWS):
            mp = reference_model(*perturbed(X, W, U, H, 20 + d), eps, norm, nblk, sp, nu)
            raise_to(stage, {"loss": ip.loss_metric(float(mp.compute_negative_loglikelihood()), ref_loss, M, F, T)})
    W = fx["W_10"]
    ref_out = reference_output(X, W)
    assert np.array_equal(ref_out, fx["out"]), (name, "out")
    raise_to(stage, {"out": ip.out_metric(ip.projection_back_output(X, W), ref_out)})
    for d in range(N_DRAWS):
        rng = np.random.default_rng(30 + d)
        raise_to(stage, {"out": ip.out_metric(reference_output(ip.one_ulp(X, rng), ip.one_ulp(W, rng)), ref_out)})

    # ---- one iteration from every recorded state whose successor is recorded
    for it in ip.START_ITERS:
        W, U, H = ip.state(fx, it)
        ref, ref_loss = reference_iterations(X, W, U, H, eps, norm, nblk, sp, nu, 1)
        want = ip.state(fx, it + 1)
        assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[2], want[2]), (name, it)
        assert ref_loss[0] == fx["loss"][it + 1], (name, it)
        for la in (ip.LAPACK, ip.KERNEL):
            got, losses = restated_iterations(X, W, U, H, eps, norm, nblk, sp, nu, 1, la)
            raise_to(own["one_iteration"], dict(model_figures(got, ref),
                                                loss=ip.loss_metric(np.array(losses), np.array(ref_loss), M, F, T)))
        for d in range(N_DRAWS):
            got, losses = reference_iterations(*perturbed(X, W, U, H, 100 * it + d), eps, norm, nblk, sp, nu, 1)
            raise_to(own["one_iteration"], dict(model_figures(got, ref),
                                                loss=ip.loss_metric(np.array(losses), np.array(ref_loss), M, F, T)))

    # ---- the whole run
    W, U, H = ip.state(fx, 0)
    ref, ref_loss = reference_iterations(X, W, U, H, eps, norm, nblk, sp, nu, ip.N_ITER)
    assert np.array_equal(ref_loss, fx["loss"][1:]), name
    ref_out = reference_output(X, ref[0])
    for la in (ip.LAPACK, ip.KERNEL):
        got, losses = restated_iterations(X, W, U, H, eps, norm, nblk, sp, nu, ip.N_ITER, la)
        raise_to(own["whole_run"], dict(model_figures(got, ref), out=ip.out_metric(ip.projection_back_output(X, got[0]), ref_out),
                                        loss=ip.loss_metric(np.array(losses), np.array(ref_loss), M, F, T)))
    for d in range(N_DRAWS):
        Xp, Wp, Up, Hp = perturbed(X, W, U, H, 1000 + d)
        got, losses = reference_iterations(Xp, Wp, Up, Hp, eps, norm, nblk, sp, nu, ip.N_ITER)
        raise_to(own["whole_run"], dict(model_figures(got, ref), out=ip.out_metric(reference_output(Xp, got[0]), ref_out),
                                        loss=ip.loss_metric(np.array(losses), np.array(ref_loss), M, F, T)))
    return own


def probe(rs):
    levels = ("one_stage", "one_iteration", "whole_run")
    worst, measured = {k: {} for k in levels}, {}
    for path in rs.fixture_files():
        name = os.path.splitext(os.path.basename(path))[0]
        own = probe_fixture(np.load(path), name)
        measured[name] = own
        for k in levels:
            raise_to(worst[k], own[k])
        print("%-40s %s" % (name, {k: {m: "%.1e" % v for m, v in own[k].items()} for k in levels}), file=sys.stderr)
    doc = {"factor": FACTOR, "measured": measured}
    for k in levels:
        doc[k] = {m: FACTOR * max(v, RESOLUTION) for m, v in worst[k].items()}
    top = max(doc["one_stage"].values())
    if top > LIMIT:
        sys.exit("one-stage tolerance %.1e > %.0e: the restatement is not the reference's update" % (top, LIMIT))
    return doc


def envelope():
    """Measure the d tables of tests/ipsdta_envelope_np.py; exit status 1 where they differ from the committed ones."""
    import ipsdta_envelope_np as ev
    outputs = ("basis", "activation", "normalize_U", "normalize_H", "spatial_1", "spatial_2", "loss")
    print("%-20s %-5s " % ("case", "model") + " ".join("%-11s" % o for o in outputs))

    def report(name, model, d):
        print("%-20s %-5s " % (name, model) + " ".join("%-11s" % ("%.1e" % d[o] if o in d else "-") for o in outputs),
              flush=True)

    worst, own = ev.measure_grid(report=report)
    D = {m: {k: ev.round_up(v) for k, v in worst[m].items()} for m in worst}
    S = {m: {c: ev.round_up(v) for c, v in own[m].items()} for m in own}
    for m in D:
        print("D[%r] = %r" % (m, D[m]))
    for m in S:
        print("D_BASIS_SINGLE_FRAME[%r] = %r" % (m, S[m]))
    same = D == ev.D and S == ev.D_BASIS_SINGLE_FRAME
    print("the committed tables are %s" % ("reproduced" if same else "DIFFERENT"))
    sys.exit(0 if same else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("gauss", "t"))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--envelope", action="store_true")
    a = ap.parse_args()
    if a.envelope:
        envelope()
    if a.model is None:
        ap.error("--model or --envelope is required")
    load_reference()
    rs = ip if a.model == "gauss" else tp
    out = os.path.join(rs.GOLDEN, "tolerances.json")
    doc = probe(rs)
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if a.check:
        same = os.path.exists(out) and open(out).read() == text
        print("tolerances.json %s" % ("reproduced" if same else "DIFFERS"))
        sys.exit(0 if same else 1)
    with open(out, "w") as fh:
        fh.write(text)
    print("wrote %s" % out)


if __name__ == "__main__":
    main()
