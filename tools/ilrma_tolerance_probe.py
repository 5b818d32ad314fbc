#!/usr/bin/env python3
"""Measure d, the one-rounding sensitivity of every Gauss-ILRMA / AuxIVA output, over the envelope grids (CPU, NumPy).

For every state of tests/ilrma_envelope_np.py's grids the oracle is evaluated on the state and on three copies whose
real and imaginary parts are multiplied by 1 + s * u, s in {-1, 0, 1}, with u = 2^-52 on the float64 state and 2^-23
on the float32-rounded one.  d is the largest entry-wise difference per output kind over a grid, rounded up to two
digits; the tests' tolerance is max(256 * d, floor).  The D_ILRMA / D_AUXIVA tables and MAX_COND_MEASURED of
tests/ilrma_envelope_np.py hold what this prints.

    python tools/ilrma_tolerance_probe.py                           # both grids, both dtypes, one JSON document
    python tools/ilrma_tolerance_probe.py --cases m2_k1_d2_f3_t1    # grid cases by name (either grid)
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ilrma_envelope_np as env  # noqa: E402

DTYPES = ("float64", "float32")


def round_up(v, digits=2):
    """v rounded up to `digits` significant digits (0 stays 0)."""
    if v <= 0:
        return 0.0
    e = math.floor(math.log10(v)) - (digits - 1)
    return float("%.*e" % (digits - 1, math.ceil(v / 10 ** e * (1 - 1e-12)) * 10 ** e))


def probe_case(case, dtype):
    """({kind: d}, largest regular cond(W U)) of one grid case."""
    u = env.U64 if dtype == "float64" else env.U32
    own = {}
    if case in env.ILRMA_GRID:
        states, refs = env.ilrma_case(case, dtype)
        domain = env.ILRMA_GRID[case][2]
        ds = [(env.ilrma_sensitivity(s, domain, u, seed=i), env.ilrma_kind) for i, s in enumerate(states)]
    else:
        states, refs = env.auxiva_case(case, dtype)
        ds = [(env.auxiva_sensitivity(s, u, seed=i), env.auxiva_kind) for i, s in enumerate(states)]
    for d, kind_of in ds:
        for k, v in d.items():
            own[kind_of(k)] = max(own.get(kind_of(k), 0.0), v)
    return own, env.max_cond(refs)


def probe(cases, dtype, verbose):
    total, cond = {}, 0.0
    for case in cases:
        t0 = time.time()
        own, c = probe_case(case, dtype)
        cond = max(cond, c)
        for k, v in own.items():
            total[k] = max(total.get(k, 0.0), v)
        if verbose:
            print("%s %-24s %5.1f s  cond %.1e  %s" % (dtype, case, time.time() - t0, c,
                                                      {k: "%.1e" % v for k, v in own.items()}), file=sys.stderr)
    return {k: round_up(v) for k, v in total.items()}, cond


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="*", help="grid cases by name (default: both grids in full)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    names = a.cases or list(env.ILRMA_GRID) + list(env.AUXIVA_GRID)
    out = {"D_ILRMA": {}, "D_AUXIVA": {}, "tolerances": {}}
    cond = 0.0
    for table, grid in (("D_ILRMA", env.ILRMA_GRID), ("D_AUXIVA", env.AUXIVA_GRID)):
        cases = [c for c in names if c in grid]
        for dt in DTYPES:
            if cases:
                out[table][dt], c = probe(cases, dt, not a.quiet)
                cond = max(cond, c)
                floor = env.FLOOR64 if dt == "float64" else env.FLOOR32
                out["tolerances"][table + "_" + dt] = {k: env.tolerance(v, floor) for k, v in out[table][dt].items()}
    out["MAX_COND_MEASURED"] = round_up(cond)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
