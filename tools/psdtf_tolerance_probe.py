#!/usr/bin/env python3
"""Measure the tolerances of the LDPSDTF tests and write tests/golden/psdtf/tolerances.json (CPU, NumPy only).

Runs where the reference tree is present, like tests/golden/psdtf/make_psdtf.py.  Metrics (tests/psdtf_np.py): V, per
basis max|a - b| / max|b| over the matrix (off-diagonal entries pass through zero); H, entry-wise |a - b| / |b|; loss,
|a - b| / (|b| + n_bins n_frames).  For every fixture three things are measured against the reference:

  restatement   tests/psdtf_np.py on numpy.linalg
  kernel model  tests/psdtf_np.py on the NumPy models of the kernels' algorithms (Cholesky inverse, Jacobi in the kernels'
                rotation order, the Cholesky shortcut of to_psd)
  sensitivity   the reference against itself after every entry of V (symmetrically) and H moved to a neighbouring double
                (the largest of N_DRAWS independent draws of the directions)

`one_update`: from every recorded state whose successor is recorded.  `whole_run`: 20 updates from the initial state,
compared at iteration 20 (the loss: the largest figure over all 20 entries of the list).  Both are the largest figure over
all fixtures, per metric.  A tolerance is FACTOR x the largest of the three figures, and at least FACTOR x 2^-52.  A
one-update tolerance above LIMIT means the restatement is not the reference's update: nothing is written then.

    python tools/psdtf_tolerance_probe.py            # writes tolerances.json
    python tools/psdtf_tolerance_probe.py --check    # measures and compares with the committed file
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402

import psdtf_np as pt  # noqa: E402
import make_golden  # noqa: E402,F401  reference on sys.path
from algorithm.psdtf import LDPSDTF  # noqa: E402

FACTOR = 16
LIMIT = 1e-10
RESOLUTION = 2.0 ** -52
N_DRAWS = 3
OUT = os.path.join(pt.GOLDEN, "tolerances.json")


def reference_run(X, V, H, eps, norm, n):
    """The reference's states ((K, M, M), (K, T)) and losses after 1..n updates from basis V (M, M, K) and H."""
    m = LDPSDTF(n_basis=H.shape[0], normalize=norm, eps=eps)
    m.target = X
    # the reference keeps the basis as a transposed view of a (K, M, M) array; the memory order decides how NumPy sums
    m.basis, m.activation = pt.kmm(V).transpose(1, 2, 0), H.copy()
    states = []
    for _ in range(n):
        m.update(iteration=1)
        states.append((pt.kmm(m.basis), m.activation.copy()))
    return states, [float(v) for v in m.loss]


def perturbed(V, H, seed):
    rng = np.random.default_rng(seed)
    return pt.mmk(pt.sym_ulp(pt.kmm(V), rng)), pt.one_ulp(H, rng)


def raise_to(total, figures):
    for k, v in figures.items():
        total[k] = max(total.get(k, 0.0), v)


def against(states, losses, ref_states, ref_losses, M, T):
    """Model metrics at the last state, loss metric over the whole list."""
    return {"V": pt.v_metric(states[-1][0], ref_states[-1][0]), "H": pt.h_metric(states[-1][1], ref_states[-1][1]),
            "loss": pt.loss_metric(np.array(losses), np.array(ref_losses), M, T)}


def probe():
    one, whole, measured = {}, {}, {}
    for path in pt.fixture_files():
        name = os.path.splitext(os.path.basename(path))[0]
        fx = np.load(path)
        X, eps, norm = fx["X"], float(fx["eps"]), bool(fx["normalize"])
        Xf = pt.frames_first(X)
        M, _, T = X.shape
        own = {"one_update": {}, "whole_run": {}}
        for it in pt.START_ITERS:
            V, H = pt.state(fx, it)
            want = pt.state(fx, it + 1)
            ref, ref_loss = reference_run(X, V, H, eps, norm, 1)
            assert np.array_equal(pt.mmk(ref[0][0]), want[0]) and np.array_equal(ref[0][1], want[1]), (name, it)
            assert ref_loss[0] == fx["loss"][it], (name, it)
            for la in (pt.LAPACK, pt.KERNEL):
                raise_to(own["one_update"], against(*pt.run(Xf, pt.kmm(V), H, eps, 1, norm, la), ref, ref_loss, M, T))
            for d in range(N_DRAWS):
                raise_to(own["one_update"], against(*reference_run(X, *perturbed(V, H, 100 * it + d), eps, norm, 1), ref,
                                                    ref_loss, M, T))
        V, H = pt.state(fx, 0)
        ref, ref_loss = reference_run(X, V, H, eps, norm, pt.N_ITER)
        assert np.array_equal(ref_loss, fx["loss"]), name
        for la in (pt.LAPACK, pt.KERNEL):
            raise_to(own["whole_run"], against(*pt.run(Xf, pt.kmm(V), H, eps, pt.N_ITER, norm, la), ref, ref_loss, M, T))
        for d in range(N_DRAWS):
            raise_to(own["whole_run"], against(*reference_run(X, *perturbed(V, H, 1000 + d), eps, norm, pt.N_ITER), ref,
                                               ref_loss, M, T))
        measured[name] = own
        raise_to(one, own["one_update"])
        raise_to(whole, own["whole_run"])
        print("%-30s one update %s  whole run %s" % (name, {k: "%.1e" % v for k, v in own["one_update"].items()},
                                                     {k: "%.1e" % v for k, v in own["whole_run"].items()}),
              file=sys.stderr)
    doc = {"factor": FACTOR,
           "one_update": {k: FACTOR * max(one[k], RESOLUTION) for k in pt.METRICS},
           "whole_run": {k: FACTOR * max(whole[k], RESOLUTION) for k in pt.METRICS},
           "measured": measured}
    worst = max(doc["one_update"].values())
    if worst > LIMIT:
        sys.exit("one-update tolerance %.1e > %.0e: the restatement is not the reference's update" % (worst, LIMIT))
    return doc


def main():
    doc = probe()
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if sys.argv[1:] == ["--check"]:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("tolerances.json %s" % ("reproduced" if same else "DIFFERS"))
        sys.exit(0 if same else 1)
    with open(OUT, "w") as fh:
        fh.write(text)
    print("wrote %s" % OUT)


if __name__ == "__main__":
    main()
