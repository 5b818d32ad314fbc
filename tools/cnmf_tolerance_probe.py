#!/usr/bin/env python3
"""Measure the tolerances of the ComplexEUCNMF tests and write tests/golden/cnmf/tolerances.json (CPU, NumPy only).

Runs where the reference tree is present, like tests/golden/cnmf/make_cnmf.py.  Every figure is a max-abs difference
over the max-abs of what it is compared with.  Metrics: T (basis), V (activation), components (T V exp(i Phi); the
phase is never compared as a raw angle, it wraps at +-pi) and loss.  For every fixture two things are measured:

  restatement   tests/cnmf_np.py against the reference's recorded next state
  sensitivity   the reference against itself after every entry of T, V and Phi moved to a neighbouring double (the
                largest of N_DRAWS independent draws of the directions)

`one_update`: from every recorded state whose successor is recorded.  `whole_run`: from the initial state, metrics at
iterations 1 and 2 and the loss at 5.  Both are the largest figure over all fixtures, per metric.  `loss_20`: the
sensitivity of loss[20] alone, per fixture (whole runs diverge entry by entry: a one-ulp change grows by about x50 per
iteration in the components).  loss[20] turns out to be far better conditioned than the model: in several fixtures all
draws return the very same double.  A measured 0 says "less than one ulp", not "exact" -- a relative difference of two
float64 values cannot be resolved below RESOLUTION = 2^-52 -- so that is the least sensitivity recorded for it; a sum
of F T terms in another order does not reproduce every bit.  A tolerance is FACTOR x the larger of the two figures:
the factor covers the device's sincos, atan2 and pow being a few ulp from NumPy's, and another order of summation.  A
one-update tolerance above LIMIT means the restatement is not the reference's update: nothing is written then.

    python tools/cnmf_tolerance_probe.py            # writes tolerances.json
    python tools/cnmf_tolerance_probe.py --check    # measures and compares with the committed file
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402

import cnmf_np as cn  # noqa: E402
import make_golden  # noqa: E402,F401  reference on sys.path
from algorithm.nmf import ComplexEUCNMF  # noqa: E402

FACTOR = 16
LIMIT = 1e-10
RESOLUTION = 2.0 ** -52
N_DRAWS = 3
METRICS = ("T", "V", "components", "loss")
OUT = os.path.join(cn.GOLDEN, "tolerances.json")


def reference_run(X, model, regularizer, p, eps, n):
    """The reference's states after 1..n update_once calls from `model` = (T, V, Phi)."""
    m = ComplexEUCNMF(n_basis=model[0].shape[1], regularizer=regularizer, p=p, eps=eps)
    m.target = X
    m.basis, m.activation, m.phase = (a.copy() for a in model)
    m.update_beta()
    out = []
    for _ in range(n):
        m.update_once()
        out.append((m.basis.copy(), m.activation.copy(), m.phase.copy()))
    return out


def restatement_run(X, model, regularizer, p, eps, n):
    out = []
    for _ in range(n):
        model = cn.update(X, *model, regularizer, p, eps)
        out.append(model)
    return out


def perturbed(model, seed):
    rng = np.random.default_rng(seed)
    return tuple(cn.one_ulp(a, rng) for a in model)


def raise_to(total, figures):
    for k, v in figures.items():
        total[k] = max(total.get(k, 0.0), v)


def probe():
    one, whole, loss20, measured = {}, {"1": {}, "2": {}, "5": {}}, {}, {}
    for path in cn.fixture_files():
        name = os.path.splitext(os.path.basename(path))[0]
        fx = np.load(path)
        X, (reg, p, eps) = fx["X"], cn.params(fx)
        own = {"one_update": {}, "whole_run": {"1": {}, "2": {}, "5": {}}}
        for it in cn.start_iters(fx):
            start, want = cn.state(fx, it), cn.state(fx, it + 1)
            ref = reference_run(X, start, reg, p, eps, 1)[0]
            assert all(np.array_equal(a, b) for a, b in zip(ref, want)), (name, it)  # the recipe reproduces the record
            raise_to(own["one_update"], cn.compare(restatement_run(X, start, reg, p, eps, 1)[0], want, X))
            for d in range(N_DRAWS):
                moved = reference_run(X, perturbed(start, 100 * it + d), reg, p, eps, 1)[0]
                raise_to(own["one_update"], cn.compare(moved, want, X))
        start = cn.state(fx, 0)
        ref = reference_run(X, start, reg, p, eps, 20)
        ref_loss = [cn.loss(X, *s) for s in ref]
        assert np.array_equal(ref_loss, fx["loss"]), name
        runs = [restatement_run(X, start, reg, p, eps, 5)]
        runs += [reference_run(X, perturbed(start, 1000 + d), reg, p, eps, 20) for d in range(N_DRAWS)]
        l20 = 0.0
        for r, run in enumerate(runs):
            for it in (1, 2):
                raise_to(own["whole_run"][str(it)], cn.compare(run[it - 1], ref[it - 1], X))
            raise_to(own["whole_run"]["5"], {"loss": cn.rel(cn.loss(X, *run[4]), ref_loss[4])})
            if r > 0:
                l20 = max(l20, cn.rel(cn.loss(X, *run[19]), ref_loss[19]))
        own["loss_20"] = l20
        measured[name] = own
        raise_to(one, own["one_update"])
        for it in whole:
            raise_to(whole[it], own["whole_run"][it])
        loss20[name] = FACTOR * max(l20, RESOLUTION)
        print("%-40s one update %s  loss[20] %.1e" % (name, {k: "%.1e" % v for k, v in own["one_update"].items()}, l20),
              file=sys.stderr)
    doc = {"factor": FACTOR,
           "one_update": {k: FACTOR * one[k] for k in METRICS},
           "whole_run": {it: {k: FACTOR * v for k, v in whole[it].items()} for it in whole},
           "loss_20": loss20,
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
