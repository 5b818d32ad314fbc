#!/usr/bin/env python3
"""Measure d, the one-rounding sensitivity of every MNMF / FastMNMF output, over the envelope grids (CPU, NumPy only).

For every case of tests/envelope_np.py's grids the NumPy restatement is evaluated on the state and on three copies
whose real and imaginary parts are multiplied by 1 + s * u, s in {-1, 0, 1} (u = 2^-52; for FastMNMF also 2^-23 on the
float32-rounded state).  d is the largest entry-wise difference per output over the grid; the tests' tolerance is
256 * d with a floor (see the docstring of tests/envelope_np.py, which holds the numbers this prints).

    python tools/mnmf_tolerance_probe.py            # both grids, one JSON document
    python tools/mnmf_tolerance_probe.py --cases m2_n1_k1_f3_t1 m4_n2_k8_f33_t64   # MNMF cases by name
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import envelope_np as env  # noqa: E402


def _merge(total, d, kind_of):
    for k, v in d.items():
        total[kind_of(k)] = max(total.get(kind_of(k), 0.0), v)


def probe_mnmf(cases, verbose):
    total, few = {}, {}
    for case in cases:
        t0 = time.time()
        own = {}
        for i, state in enumerate(env.mnmf_states(case)):
            d = env.mnmf_sensitivity(state, env.U64, seed=i)
            if env.few_frames(case):  # its spatial d stays out of the grid's (the T < 2 M exception)
                few[case] = max([few.get(case, 0.0)] + [v for k, v in d.items() if env.mnmf_kind(k) == "spatial"])
                d = {k: v for k, v in d.items() if env.mnmf_kind(k) != "spatial"}
            _merge(own, d, env.mnmf_kind)
        _merge(total, own, lambda k: k)
        if verbose:
            print("mnmf %-26s %5.1f s  %s" % (case, time.time() - t0, {k: "%.1e" % v for k, v in own.items()}),
                  file=sys.stderr)
    return total, few


def probe_fastmnmf(cases, dtype, verbose):
    total = {}
    u = env.U64 if dtype == "float64" else env.U32
    for case in cases:
        t0 = time.time()
        own = {}
        for i, state in enumerate(env.fastmnmf_states(case, dtype)):
            _merge(own, env.fastmnmf_sensitivity(state, u, seed=i), env.fastmnmf_kind)
        _merge(total, own, lambda k: k)
        if verbose:
            print("fastmnmf %s %-22s %5.1f s  %s" % (dtype, case, time.time() - t0,
                                                     {k: "%.1e" % v for k, v in own.items()}), file=sys.stderr)
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="*", help="MNMF grid cases by name (default: both grids in full)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    out = {}
    d, few = probe_mnmf(a.cases or list(env.MNMF_GRID), not a.quiet)
    out["D_MNMF"], out["D_MNMF_SPATIAL_FEW_FRAMES"] = d, few
    if not a.cases:
        out["D_FASTMNMF"] = {dt: probe_fastmnmf(list(env.FASTMNMF_GRID), dt, not a.quiet)
                             for dt in ("float64", "float32")}
    out["tolerances"] = {
        "mnmf": {k: env.tolerance(v) for k, v in d.items()},
        "mnmf_spatial_few_frames": {k: env.tolerance(v) for k, v in few.items()},
    }
    for dt, dd in out.get("D_FASTMNMF", {}).items():
        floor = env.FLOOR64 if dt == "float64" else env.FLOOR32
        out["tolerances"]["fastmnmf_" + dt] = {k: env.tolerance(v, floor) for k, v in dd.items()}
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
