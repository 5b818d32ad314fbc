#!/usr/bin/env python3
"""ProxLaplaceIVA milliseconds per iteration on the device, with and without the loss (assx_pdsbss_iterate), and the time of
the operator norm (assx_pdsbss_operator_norm, once per call of the model), at (n_channels, n_bins, n_frames) = (2, 1025,
2048) and (4, 1025, 4096).  Prints ONE JSON line per size.

    python tools/pdsbss_bench.py [--iters 10] [--warmup 2] [--repeats 5] [--sizes 2,1025,2048 4,1025,4096]

A figure is the median over `repeats` windows of `iters` iterations each (the norm: one call per window), every window
between two device synchronisations on the host clock, after `warmup` iterations; min and max are printed beside it.
Clocks are whatever the device runs at (nothing is pinned), and the device's name is printed.  X is the seeded complex
Gaussian of the envelope sweeps, W starts at the identity and y at zero, as in a call of the model; every window starts
from the same copies.  Parameters: regularizer 1, both prox steps 1, relaxation 1.75 (the reference's own example).

Algorithmic bytes per iteration, from the shapes: sweep 1 reads X and y, sweep 2 reads X and y and writes y; the per-bin
arrays (W, D, the partials of G) and the (n_sources, n_frames) slice partials are small beside them and left out.  With
N = M that is 5 |X|.  `GB_per_s` is that over the time without the loss.  `regime` says where X and y sit between the
sweeps: together below the 256 MiB Infinity Cache they can be served from it ("cache"), else from HBM.
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


def bench(M, F, T, iters, warmup, repeats):
    import numpy as np
    import torch
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype="float64")
    rng = np.random.default_rng(900 + M)
    Xh = (rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))) * (0.1 + rng.random((1, F, 1)))
    X = torch.from_numpy(np.ascontiguousarray(Xh)).to(eng.dev)
    W0 = torch.eye(M, dtype=torch.complex128, device=eng.dev).repeat(F, 1, 1).contiguous()
    ws = eng.pdsbss_workspace(M, F, T)
    status = eng.new_status(1)
    norm = eng.pdsbss_operator_norm(X, ws, status=status)
    par = dict(C=1.0, mu1=1.0, mu2=1.0, alpha=1.75)

    def window(n, with_loss):
        W, y = W0.clone(), torch.zeros((F, M, T), dtype=torch.complex128, device=eng.dev)
        loss = eng.empty((n + 1,), dtype=torch.float64) if with_loss else None
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        eng.pdsbss_iterate(n, X, norm, W, y, ws, loss=loss, status=status, **par)
        torch.cuda.synchronize(eng.dev)
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(torch.view_as_real(W)).all()) and int(status.max().item()) == 0
        return dt / max(n, 1)

    def norm_once():
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        eng.pdsbss_operator_norm(X, ws, norm=norm, status=status)
        torch.cuda.synchronize(eng.dev)
        return time.perf_counter() - t0

    x_bytes = 16 * M * F * T
    alg = 5 * x_bytes
    out = {"metric": "pdsbss_ms_per_iteration", "class": "ProxLaplaceIVA", "n_channels": M, "n_bins": F, "n_frames": T,
           "x_MB": round(x_bytes / 1e6, 1), "workspace_MiB": round(ws.numel() / 2 ** 20, 1),
           "regime": "cache" if 2 * x_bytes < INFINITY_CACHE_BYTES else "hbm", "algorithmic_bytes_per_iteration": alg}
    for with_loss in (False, True):
        window(warmup, with_loss)
        med, span = stats([window(iters, with_loss) for _ in range(repeats)])
        key = "ms_per_iteration" + ("_with_loss" if with_loss else "")
        out[key], out[key + "_min_max"] = med, span
    out["GB_per_s"] = round(alg / (out["ms_per_iteration"] * 1e-3) / 1e9, 1)
    norm_once()
    out["operator_norm_ms"], out["operator_norm_ms_min_max"] = stats([norm_once() for _ in range(repeats)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["2,1025,2048", "4,1025,4096"])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pdsbss_bench.py needs a GPU: a timing taken anywhere else says nothing")
    head = {"dtype": "float64", "device": torch.cuda.get_device_name(0), "clocks": "not pinned", "iters": a.iters,
            "warmup": a.warmup, "repeats": a.repeats, "statistic": "median"}
    for size in a.sizes:
        M, F, T = (int(v) for v in size.split(","))
        print(json.dumps(dict(head, **bench(M, F, T, a.iters, a.warmup, a.repeats))), flush=True)


if __name__ == "__main__":
    main()
