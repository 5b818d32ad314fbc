#!/usr/bin/env python3
"""ComplexEUCNMF milliseconds per iteration through assx_cnmf_iterate, with and without the loss, at the reference's own
test size F = 513, n_basis = 6 (src/algorithm/nmf.py:908-927) with T = 1024, and at n_basis = 32.  Prints ONE JSON line
with the launches per iteration and the traffic contract of every pass -- the bytes it must move once, computed from
the shapes -- and the bytes per second the whole iteration achieves against their sum.

    python tools/cnmf_bench.py [--iters 50] [--warmup 3]
    python tools/cnmf_bench.py --kernel-stats STATS.csv [--shape k6]

Per-pass rates need per-kernel times: run the first form for ONE shape (--shape) under
`rocprofv3 --kernel-trace --stats` in a run of its own, then give the second form the *_kernel_stats.csv it wrote; it
prints each pass's mean time and achieved bytes per second (no GPU needed for that).
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_BPS = 8.0e12        # MI355X HBM3E peak
ACHIEVABLE_HBM_BPS = 6.3e12  # what a streaming kernel reaches

SHAPES = {"k6": (513, 1024, 6), "k32": (513, 1024, 32)}
LAUNCHES_PER_ITER = 4  # residual, basis, activation, finalize; the loss adds two launches per CALL, not per iteration
KERNELS = {"cn_resid_kernel": "residual", "cn_basis_kernel": "basis", "cn_act_kernel": "activation",
           "cn_finalize_kernel": "finalize"}


def slabs(F):
    return min((F + 7) // 8, 32)


def contract(F, T, K):
    """Bytes each pass must move once per iteration (float64; X, ZX complex)."""
    phi, ft, kt, fk = 8 * F * K * T, F * T, 8 * K * T, 8 * F * K
    part = 16 * slabs(F) * K * T
    c = {"residual": phi + 16 * ft + kt + fk + 24 * ft,       # Phi, X, V, T in; ZX, tv out
         "basis": phi + 24 * ft + kt + fk + fk,               # Phi, ZX, tv, V, T in; T' out
         "activation": 2 * phi + 24 * ft + kt + 2 * fk + part,  # Phi in and out; ZX, tv, V, T, T' in; slab partials out
         "finalize": part + 2 * kt + 2 * fk}                  # partials, V, T' in; V, T out
    c["iteration"] = sum(c.values())
    return c


def bench_device(F, T, K, with_loss, iters, warmup):
    import numpy as np
    import torch
    from audio_source_separation_amd.algorithm.nmf import ComplexEUCNMF
    g = torch.Generator(device="cuda").manual_seed(0)
    mag = torch.rand((F, 3), dtype=torch.float64, device="cuda", generator=g) \
        @ torch.rand((3, T), dtype=torch.float64, device="cuda", generator=g)
    X = torch.polar(mag, 2 * np.pi * torch.rand((F, T), dtype=torch.float64, device="cuda", generator=g))

    def run(n):
        np.random.seed(0)
        model = ComplexEUCNMF(n_basis=K, recordable_loss=with_loss)
        model(X, iteration=n)
        if with_loss:
            np.asarray(model.loss)
        return model

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(0)
    torch.cuda.synchronize()
    fixed = time.perf_counter() - t0  # reset, draws and uploads: subtracted below
    t0 = time.perf_counter()
    model = run(iters)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0 - fixed) / iters
    assert np.all(np.isfinite(model.basis)) and np.all(np.isfinite(model.activation))
    return dt


def kernel_stats(path, F, T, K):
    c = contract(F, T, K)
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for kernel, name in KERNELS.items():
                if kernel in row["Name"]:
                    ns = float(row["AverageNs"])
                    out[name] = {"calls": int(row["Calls"]), "mean_us": round(ns / 1e3, 2), "bytes": c[name],
                                 "achieved_TBps": round(c[name] / ns / 1e3, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=sorted(SHAPES), help="only this shape")
    ap.add_argument("--kernel-stats", help="a rocprofv3 *_kernel_stats.csv of a run with --shape")
    a = ap.parse_args()
    if a.kernel_stats:
        F, T, K = SHAPES[a.shape or "k6"]
        print(json.dumps({"metric": "cnmf_pass_bytes_per_s", "shape": a.shape or "k6", "F": F, "T": T, "K": K,
                          "hbm_peak_TBps": PEAK_HBM_BPS / 1e12, "hbm_achievable_TBps": ACHIEVABLE_HBM_BPS / 1e12,
                          "passes": kernel_stats(a.kernel_stats, F, T, K)}))
        return
    import torch
    out = {"metric": "cnmf_ms_per_iter", "dtype": "float64", "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "launches_per_iter": LAUNCHES_PER_ITER, "hbm_peak_TBps": PEAK_HBM_BPS / 1e12,
           "hbm_achievable_TBps": ACHIEVABLE_HBM_BPS / 1e12, "results": []}
    for name in ([a.shape] if a.shape else sorted(SHAPES, key=lambda s: SHAPES[s][2])):
        F, T, K = SHAPES[name]
        c = contract(F, T, K)
        r = {"shape": name, "F": F, "T": T, "K": K, "contract_bytes": c,
             "floor_ms": round(c["iteration"] / ACHIEVABLE_HBM_BPS * 1e3, 4)}
        for with_loss in (False, True):
            dt = bench_device(F, T, K, with_loss, a.iters, a.warmup)
            r["ms_per_iter_loss" if with_loss else "ms_per_iter"] = round(dt * 1e3, 4)
        r["achieved_TBps"] = round(c["iteration"] / (r["ms_per_iter"] * 1e-3) / 1e12, 3)
        out["results"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
