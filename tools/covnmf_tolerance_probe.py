#!/usr/bin/env python3
"""Measure d, the one-rounding sensitivity of every covariance-domain MNMF output, over the envelope grid (CPU, NumPy only).

For every case of tests/covnmf_envelope_np.py's grid the NumPy restatement is evaluated on the state and on three copies
whose real and imaginary parts are multiplied by 1 + s * u, s in {-1, 0, 1}, u = 2^-52 (target and spatial
re-symmetrised).  d is the largest entry-wise difference per output over the grid; the tests' tolerance is 256 * d with a
floor of 1e-13 (tests/envelope_np.py).  tests/covnmf_envelope_np.py holds the numbers this prints.

    python tools/covnmf_tolerance_probe.py            # the whole grid, one JSON document
    python tools/covnmf_tolerance_probe.py --cases m2_k1_f3_t1 m8_k64_f17_t130
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import envelope_np as env  # noqa: E402
import covnmf_envelope_np as cenv  # noqa: E402


def probe(cases, verbose):
    total, few = {}, {}
    for case in cases:
        t0 = time.time()
        d = cenv.sensitivity(cenv.case_state(case))
        own = {}
        for k, v in d.items():
            if cenv.kind(k) == "spatial" and cenv.few_frames(case):  # stays out of the grid's (the T < 2 M exception)
                few[case] = max(few.get(case, 0.0), v)
            else:
                own[cenv.kind(k)] = max(own.get(cenv.kind(k), 0.0), v)
        for k, v in own.items():
            total[k] = max(total.get(k, 0.0), v)
        if verbose:
            print("covnmf %-20s %5.1f s  %s%s" % (case, time.time() - t0, {k: "%.1e" % v for k, v in own.items()},
                                                  "  few-frames spatial %.1e" % few[case] if case in few else ""),
                  file=sys.stderr)
    return total, few


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="*", help="grid cases by name (default: the whole grid)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    d, few = probe(a.cases or list(cenv.GRID), not a.quiet)
    out = {"D": d, "D_SPATIAL_FEW_FRAMES": few,
           "tolerances": {"grid": {k: env.tolerance(v) for k, v in d.items()},
                          "spatial_few_frames": {k: env.tolerance(v) for k, v in few.items()}}}
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
