#!/usr/bin/env python3
"""Measure d, the one-rounding sensitivity of every beamformer / PCA / MDP output, over the envelope grid (CPU, NumPy only).

For every case of tests/beamform_envelope_np.py's grid the NumPy restatement is evaluated on the state and on three copies
whose real and imaginary parts (X, A, R and the sources) are multiplied by 1 + s * u, s in {-1, 0, 1}, u = 2^-52.  d is
the largest entry-wise difference per kind of output over the grid; the tests' tolerance is 256 * d with a floor of 1e-13
(tests/envelope_np.py).  The chain figure is the same for the recorded PCA -> AuxLaplaceIVA -> projection back case
(tests/golden/beamform).  tests/beamform_envelope_np.py holds the numbers this prints.

    python tools/beamform_tolerance_probe.py            # the whole grid and the chain, one JSON document
    python tools/beamform_tolerance_probe.py --cases m2_n1_f1_t63 m8_n8_f17_t1025
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import envelope_np as env  # noqa: E402
import beamform_np as bf  # noqa: E402
import beamform_envelope_np as benv  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "beamform")


def probe(cases, verbose):
    total, worst = {}, {}
    for case in cases:
        st, _ = benv.grid_case(case)
        d = benv.sensitivity(st)
        for k, v in d.items():
            if v > total.get(benv.kind(k), -1.0):
                total[benv.kind(k)], worst[benv.kind(k)] = v, "%s %s" % (case, k)
        if verbose:
            print("beamform %-18s %s" % (case, {k: "%.1e" % v for k, v in d.items()}), file=sys.stderr)
    return total, worst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="*", help="grid cases by name (default: the whole grid)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    d, worst = probe(a.cases or list(benv.GRID), not a.quiet)
    chain = max(benv.chain_sensitivity(bf.load_case(GOLDEN, n)["X"]) for n in bf.cases(GOLDEN) if n.endswith("_chain"))
    out = {"D": d, "worst": worst, "D_CHAIN": chain,
           "tolerances": {"grid": {k: env.tolerance(v) for k, v in d.items()}, "chain": env.tolerance(chain)}}
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
