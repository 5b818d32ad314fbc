#!/usr/bin/env python3
"""Measure d, the one-rounding sensitivity of every gradient IVA / FDICA output, over the envelope grid (CPU, NumPy only).

For every case of tests/gradbss_envelope_np.py's grid the NumPy restatement is evaluated on the state and on three copies
whose real and imaginary parts are multiplied by 1 + s * u, s in {-1, 0, 1}, u = 2^-52.  d is the largest entry-wise
difference per output over the grid; the tests' tolerance is 256 * d with a floor of 1e-13 (tests/envelope_np.py).  The
trajectory figures are the same for whole 10-iteration runs from the fixtures' inputs (tests/golden/gradbss), W0 moved by
one rounding.  tests/gradbss_envelope_np.py holds the numbers this prints.

    python tools/gradbss_tolerance_probe.py            # the whole grid and the fixtures, one JSON document
    python tools/gradbss_tolerance_probe.py --cases m2_f1_t1 m8_f17_t1025
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import envelope_np as env  # noqa: E402
import gradbss_np as gb  # noqa: E402
import gradbss_envelope_np as genv  # noqa: E402


def probe(cases, verbose):
    total, worst = {}, {}
    for case in cases:
        d = genv.sensitivity(genv.state(*genv.GRID[case]))
        for k, v in d.items():
            if v > total.get(genv.kind(k), -1.0):
                total[genv.kind(k)], worst[genv.kind(k)] = v, "%s %s" % (case, k)
        if verbose:
            print("gradbss %-16s %s" % (case, {k: "%.1e" % v for k, v in d.items()}), file=sys.stderr)
    return total, worst


def probe_trajectories(verbose):
    total = {}
    for path in gb.fixtures(os.path.join(ROOT, "tests", "golden", "gradbss")):
        g = np.load(path)
        cls = os.path.basename(path).split("_")[0]
        d = genv.trajectory_sensitivity(cls, g["X"], g["W_0"], reference_id=int(g["reference_id"]))
        for k, v in d.items():
            total[k] = max(total.get(k, 0.0), v)
        if verbose:
            print("gradbss %-44s %s" % (os.path.basename(path), {k: "%.1e" % v for k, v in d.items()}), file=sys.stderr)
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="*", help="grid cases by name (default: the whole grid)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    d, worst = probe(a.cases or list(genv.GRID), not a.quiet)
    traj = probe_trajectories(not a.quiet)
    out = {"D": d, "worst": worst, "D_TRAJECTORY": traj,
           "tolerances": {"grid": {k: env.tolerance(v) for k, v in d.items()},
                          "trajectory": {k: env.tolerance(v) for k, v in traj.items()}}}
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
