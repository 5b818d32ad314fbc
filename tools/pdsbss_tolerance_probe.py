#!/usr/bin/env python3
"""Measure d, the one-rounding sensitivity of every ProxLaplaceIVA output, over the envelope grid (CPU, NumPy only).

For every case of tests/pdsbss_envelope_np.py's grid the NumPy restatement is evaluated on the state and on three copies
whose real and imaginary parts (X, W, y and the norm) are multiplied by 1 + s * u, s in {-1, 0, 1}, u = 2^-52.  d is the
largest entry-wise difference per kind of output over the grid; the tests' tolerance is 256 * d with a floor of 1e-13
(tests/envelope_np.py).  The trajectory figures are the same for whole 10-iteration runs from the recorded cases
(tests/golden/pdsbss).  tests/pdsbss_envelope_np.py holds the numbers this prints.

    python tools/pdsbss_tolerance_probe.py            # the whole grid and the fixtures, one JSON document
    python tools/pdsbss_tolerance_probe.py --cases m2_f1_t63 m8_f17_t1025
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import envelope_np as env  # noqa: E402
import pdsbss_np as pd  # noqa: E402
import pdsbss_envelope_np as penv  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pdsbss")


def probe(cases, verbose):
    total, worst = {}, {}
    for case in cases:
        st, _, share = penv.grid_case(case)
        d = penv.sensitivity(st)
        for k, v in d.items():
            if v > total.get(penv.kind(k), -1.0):
                total[penv.kind(k)], worst[penv.kind(k)] = v, "%s %s" % (case, k)
        if verbose:
            print("pdsbss %-16s shrinking %.2f %s" % (case, share, {k: "%.1e" % v for k, v in d.items()}), file=sys.stderr)
    return total, worst


def probe_trajectories(verbose):
    total, worst = {}, {}
    for name in pd.cases(GOLDEN):
        d = penv.trajectory_sensitivity(pd.load_case(GOLDEN, name))
        for k, v in d.items():
            if v > total.get(k, -1.0):
                total[k], worst[k] = v, name
        if verbose:
            print("pdsbss %-40s %s" % (name, {k: "%.1e" % v for k, v in d.items()}), file=sys.stderr)
    return total, worst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="*", help="grid cases by name (default: the whole grid)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    d, worst = probe(a.cases or list(penv.GRID), not a.quiet)
    traj, traj_worst = probe_trajectories(not a.quiet)
    out = {"D": d, "worst": worst, "D_TRAJECTORY": traj, "worst_trajectory": traj_worst,
           "tolerances": {"grid": {k: env.tolerance(v) for k, v in d.items()},
                          "trajectory": {k: env.tolerance(v) for k, v in traj.items()}}}
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
