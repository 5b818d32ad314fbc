#!/usr/bin/env python3
"""Measure the tolerances of the EUCNTF tests and write tests/golden/ntf/tolerances.json (CPU, NumPy only).

Runs where the reference tree is present, like tests/golden/ntf/make_ntf.py.  Every entry of the model is positive, so
every figure is the largest |a - b| / |b| over the entries.  Metrics: Z (partitioning), T (basis), V (activation) and
loss.  For every fixture two things are measured:

  restatement   tests/ntf_np.py against the reference
  sensitivity   the reference against itself after every entry of Z, T and V moved to a neighbouring double (the
                largest of N_DRAWS independent draws of the directions)

`one_update`: from every recorded state whose successor is recorded.  `whole_run`: 20 updates from the initial state,
compared at iteration 20 (the loss: the largest figure over all 20 entries of the list).  Both are the largest figure
over all fixtures, per metric.  A tolerance is FACTOR x the larger of the two figures, and at least FACTOR x RESOLUTION
= 2^-52: a relative difference of two float64 values cannot be resolved below that, and a sum in another order does not
reproduce every bit.  A one-update tolerance above LIMIT means the restatement is not the reference's update: nothing is
written then.

    python tools/ntf_tolerance_probe.py            # writes tolerances.json
    python tools/ntf_tolerance_probe.py --check    # measures and compares with the committed file
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402

import ntf_np as nt  # noqa: E402
import make_golden  # noqa: E402,F401  reference on sys.path
from algorithm.ntf import EUCNTF  # noqa: E402

FACTOR = 16
LIMIT = 1e-12
RESOLUTION = 2.0 ** -52
N_DRAWS = 3
OUT = os.path.join(nt.GOLDEN, "tolerances.json")


def reference_run(X, model, eps, n):
    """The reference's states and losses after 1..n update_once calls from `model` = (Z, T, V)."""
    m = EUCNTF(model[0].shape[1], eps=eps)
    m.target = X
    m.partitioning, m.basis, m.activation = (a.copy() for a in model)
    states, losses = [], []
    for _ in range(n):
        m.update_once()
        states.append((m.partitioning.copy(), m.basis.copy(), m.activation.copy()))
        losses.append(float(m.compute_loss()))
    return states, losses


def perturbed(model, seed):
    rng = np.random.default_rng(seed)
    return tuple(nt.one_ulp(a, rng) for a in model)


def raise_to(total, figures):
    for k, v in figures.items():
        total[k] = max(total.get(k, 0.0), v)


def against(states, losses, ref_states, ref_losses):
    """Model metrics at the last state, loss metric over the whole list."""
    out = {k: nt.rel_entry(a, b) for k, a, b in zip(("Z", "T", "V"), states[-1], ref_states[-1])}
    out["loss"] = nt.rel_entry(np.array(losses), np.array(ref_losses))
    return out


def probe():
    one, whole, measured = {}, {}, {}
    for path in nt.fixture_files():
        name = os.path.splitext(os.path.basename(path))[0]
        fx = np.load(path)
        X, eps = fx["X"], float(fx["eps"])
        own = {"one_update": {}, "whole_run": {}}
        for it in nt.START_ITERS:
            start, want = nt.state(fx, it), nt.state(fx, it + 1)
            ref, ref_loss = reference_run(X, start, eps, 1)
            assert all(np.array_equal(a, b) for a, b in zip(ref[0], want)), (name, it)  # the recipe reproduces the record
            assert ref_loss[0] == fx["loss"][it], (name, it)
            got = nt.update(X, *start, eps)
            raise_to(own["one_update"], against([got], [nt.loss(X, *got)], ref, ref_loss))
            for d in range(N_DRAWS):
                raise_to(own["one_update"], against(*reference_run(X, perturbed(start, 100 * it + d), eps, 1), ref,
                                                    ref_loss))
        start = nt.state(fx, 0)
        ref, ref_loss = reference_run(X, start, eps, nt.N_ITER)
        assert np.array_equal(ref_loss, fx["loss"]), name
        run = nt.run(X, start, eps, nt.N_ITER)
        raise_to(own["whole_run"], against(run, [nt.loss(X, *s) for s in run], ref, ref_loss))
        for d in range(N_DRAWS):
            raise_to(own["whole_run"], against(*reference_run(X, perturbed(start, 1000 + d), eps, nt.N_ITER), ref,
                                               ref_loss))
        measured[name] = own
        raise_to(one, own["one_update"])
        raise_to(whole, own["whole_run"])
        print("%-30s one update %s  whole run %s" % (name, {k: "%.1e" % v for k, v in own["one_update"].items()},
                                                     {k: "%.1e" % v for k, v in own["whole_run"].items()}),
              file=sys.stderr)
    doc = {"factor": FACTOR,
           "one_update": {k: FACTOR * max(one[k], RESOLUTION) for k in nt.METRICS},
           "whole_run": {k: FACTOR * max(whole[k], RESOLUTION) for k in nt.METRICS},
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
