#!/usr/bin/env python3
"""Gradient IVA / FDICA milliseconds per iteration on the device, with and without the loss (assx_gradbss_iterate), and
the time of FDICA's permutation solver (assx_fdica_solve_permutation), at (n_channels, n_bins, n_frames) = (2, 1025,
2048) and (4, 1025, 4096).  Prints ONE JSON line per class and size.

    python tools/gradbss_bench.py [--iters 10] [--warmup 2] [--repeats 5] [--sizes 2,1025,2048 4,1025,4096]

A figure is the median over `repeats` windows of `iters` iterations each (the solver: one call per window), every window
between two device synchronisations on the host clock, after `warmup` iterations; min and max are printed beside it.
Clocks are whatever the device runs at (nothing is pinned), and the device's name is printed.  The state is the general
one of the envelope sweep (tests/gradbss_envelope_np.py); every window starts from the same copy of it.

Algorithmic bytes per iteration: IVA reads X twice (the weight sweep, then the moment sweep), FDICA once, plus W read
and written; `GB_per_s` is that over the time without the loss.  `regime` says where X sits between the sweeps: an X
below the 256 MiB Infinity Cache can be served from it ("cache"), a larger one comes from HBM ("hbm"); 268.7 MB (256.3
MiB) at the larger size is at the edge.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INFINITY_CACHE_BYTES = 256 * 2 ** 20


def stats(times):
    return round(statistics.median(times) * 1e3, 3), [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)]


def bench(cls, M, F, T, iters, warmup, repeats):
    import numpy as np
    import torch
    import gradbss_np as gb
    import gradbss_envelope_np as genv
    from audio_source_separation_amd import _lib
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype="float64")
    model, natural = gb.CLASSES[cls]
    code = _lib.GRADBSS_IVA if model == "iva" else _lib.GRADBSS_FDICA
    Xh, Wh = genv.state(M, F, T, 900 + M)
    X, W0 = (torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev) for a in (Xh, Wh))
    ws = eng.gradbss_workspace(M, F, T)
    status = eng.new_status(1)

    def window(n, with_loss):
        W = W0.clone()
        loss = eng.empty((n + 1,), dtype=torch.float64) if with_loss else None
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        eng.gradbss_iterate(n, code, natural, X, W, ws, loss=loss, status=status)
        torch.cuda.synchronize(eng.dev)
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(torch.view_as_real(W)).all()) and int(status.max().item()) == 0
        return dt / max(n, 1)

    x_bytes = 16 * M * F * T
    w_bytes = 2 * 16 * F * M * M
    alg = (2 if model == "iva" else 1) * x_bytes + w_bytes
    out = {"metric": "gradbss_ms_per_iteration", "class": cls, "n_channels": M, "n_bins": F, "n_frames": T,
           "x_MB": round(x_bytes / 1e6, 1), "workspace_MiB": round(ws.numel() / 2 ** 20, 1),
           "regime": "cache" if x_bytes < INFINITY_CACHE_BYTES else "hbm (edge of the Infinity Cache)"
           if x_bytes < 1.1 * INFINITY_CACHE_BYTES else "hbm", "algorithmic_bytes_per_iteration": alg}
    for with_loss in (False, True):
        window(warmup, with_loss)
        med, span = stats([window(iters, with_loss) for _ in range(repeats)])
        key = "ms_per_iteration" + ("_with_loss" if with_loss else "")
        out[key], out[key + "_min_max"] = med, span
    out["GB_per_s"] = round(alg / (out["ms_per_iteration"] * 1e-3) / 1e9, 1)
    if model == "fdica":
        def solve():
            W = W0.clone()
            torch.cuda.synchronize(eng.dev)
            t0 = time.perf_counter()
            eng.fdica_solve_permutation(X, W, ws)
            torch.cuda.synchronize(eng.dev)
            return time.perf_counter() - t0
        solve()
        out["solver_ms"], out["solver_ms_min_max"] = stats([solve() for _ in range(repeats)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["2,1025,2048", "4,1025,4096"])
    ap.add_argument("--classes", nargs="+", default=["GradLaplaceIVA", "NaturalGradLaplaceIVA", "GradLaplaceFDICA",
                                                     "NaturalGradLaplaceFDICA"])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gradbss_bench.py needs a GPU: a timing taken anywhere else says nothing")
    head = {"dtype": "float64", "device": torch.cuda.get_device_name(0), "clocks": "not pinned", "iters": a.iters,
            "warmup": a.warmup, "repeats": a.repeats, "statistic": "median"}
    for size in a.sizes:
        M, F, T = (int(v) for v in size.split(","))
        for cls in a.classes:
            print(json.dumps(dict(head, **bench(cls, M, F, T, a.iters, a.warmup, a.repeats))), flush=True)


if __name__ == "__main__":
    main()
