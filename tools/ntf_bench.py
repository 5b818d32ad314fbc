#!/usr/bin/env python3
"""EUCNTF milliseconds per update through assx_ntf_iterate, with and without the loss, at the reference's own test size
(N = 2 channels, I = 513 bins, n_basis = 6, src/algorithm/ntf.py:104-123, with J = 1024 frames) and at N = 4, I = 1025,
J = 4096, n_basis = 32.  Prints ONE JSON line with the launches per update, the traffic contract -- X read three times
per update, once per numerator, and a fourth time for a stand-alone loss; computed from the shapes (DESIGN.md section
12) -- and the bytes per second each shape achieves against it.

    python tools/ntf_bench.py [--iters 50] [--warmup 5] [--repeats 5]

A figure is the median over `repeats` windows of `iters` updates each, every window between two device synchronisations
on the host clock; clocks are whatever the device runs at (nothing is pinned), and the device's name is printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_BPS = 8.0e12        # MI355X HBM3E peak
ACHIEVABLE_HBM_BPS = 6.3e12  # what a streaming kernel reaches

SHAPES = {"reference": (2, 513, 1024, 6), "large": (4, 1025, 4096, 32)}
LAUNCHES_PER_UPDATE = 8  # gram, basis, gram, activation, apply, gram, partitioning, apply; the loss adds two per CALL


def contract(N, I, J, K):
    """Bytes an update must move: X three times; a stand-alone loss reads it once more (float64)."""
    x = 8 * N * I * J
    return {"X": x, "update": 3 * x, "loss": x}


def bench_device(N, I, J, K, with_loss, iters, warmup, repeats):
    import torch
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype="float64")
    g = torch.Generator(device=eng.dev).manual_seed(0)

    def rand(*shape):
        return torch.rand(shape, dtype=torch.float64, device=eng.dev, generator=g)

    X = torch.einsum("bnk,bik,bkj->bnij", rand(1, N, 3), rand(1, I, 3), rand(1, 3, J)).contiguous()
    Z0, T0, V0 = rand(1, N, K), rand(1, I, K), rand(1, K, J)
    ws = eng.ntf_workspace(1, N, I, J, K)
    loss = eng.empty((iters, 1), dtype=torch.float64) if with_loss else None

    def window(n):
        Z, T, V = Z0.clone(), T0.clone(), V0.clone()
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        eng.ntf_iterate(n, X, Z, T, V, ws, loss=None if loss is None else loss[:n])
        torch.cuda.synchronize(eng.dev)
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(Z).all()) and bool(torch.isfinite(T).all()) and bool(torch.isfinite(V).all())
        return dt / max(n, 1)

    window(warmup)
    times = [window(iters) for _ in range(repeats)]
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", choices=sorted(SHAPES), help="only this shape")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ntf_bench.py needs a GPU: a timing taken anywhere else says nothing")
    out = {"metric": "ntf_ms_per_update", "dtype": "float64", "device": torch.cuda.get_device_name(0),
           "clocks": "not pinned", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "statistic": "median",
           "launches_per_update": LAUNCHES_PER_UPDATE, "hbm_peak_TBps": PEAK_HBM_BPS / 1e12,
           "hbm_achievable_TBps": ACHIEVABLE_HBM_BPS / 1e12, "results": []}
    for name in ([a.shape] if a.shape else ("reference", "large")):
        N, I, J, K = SHAPES[name]
        c = contract(N, I, J, K)
        r = {"shape": name, "N": N, "I": I, "J": J, "K": K, "contract_bytes": c,
             "floor_ms": round(c["update"] / ACHIEVABLE_HBM_BPS * 1e3, 4)}
        for with_loss in (False, True):
            med, lo, hi = bench_device(N, I, J, K, with_loss, a.iters, a.warmup, a.repeats)
            key = "ms_per_update_loss" if with_loss else "ms_per_update"
            r[key] = round(med * 1e3, 4)
            r[key + "_min_max"] = [round(lo * 1e3, 4), round(hi * 1e3, 4)]
        r["achieved_GBps"] = round(c["update"] / (r["ms_per_update"] * 1e-3) / 1e9, 1)
        # with the loss, every update but the last reads X three times still: the loss rides on the basis pass
        r["achieved_GBps_loss"] = round((c["update"] + c["loss"] / a.iters) / (r["ms_per_update_loss"] * 1e-3) / 1e9, 1)
        out["results"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
