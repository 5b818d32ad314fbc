#!/usr/bin/env python3
"""MultichannelISNMF (Sawada's MNMF) milliseconds per iteration through assx_mnmf_iterate, with and without the loss,
at three shapes:  M = N = 4, K = 10, F = 1025, T = 4096;  M = 8, N = 4, K = 10 (same F, T);  and the reference
notebook's call, NumPy in and out, M = N = 2, K = 30, F = 2049, T = 128, 200 iterations.  Prints ONE JSON line with
the FLOP and byte floors of every shape, computed from the shapes.

    python tools/mnmf_bench.py [--iters 20] [--warmup 3] [--cpu-baseline]

--cpu-baseline adds the seconds per iteration of the NumPy restatement (tests/mnmf_np.py) on this host's CPU at the
first shape (one iteration, float64).  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` separately.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audio_source_separation_amd.bss.mnmf import MultichannelISNMF  # noqa: E402

PEAK_F64_FLOPS = 78.6e12  # MI355X float64 vector peak
PEAK_HBM_BPS = 8.0e12     # MI355X HBM3E peak

SHAPES = {"m4_n4_k10": (4, 4, 10, 1025, 4096), "m8_n4_k10": (8, 4, 10, 1025, 4096)}


def floors(M, N, K, F, T):
    """Per iteration: FLOP of the arithmetic the kernels must do and the bytes every pass must move once.
    An evaluation per (f, t): lam (2NK), X^ (2N M(M+1)), Cholesky + triangular inverse + P (about 4 M^3 complex
    multiply-adds counted as 4 M^3), y (8 M^2), a_n and b_n (10 N M^2).  Three evaluations (basis, activation, latent)
    plus the spatial pass (one evaluation + the lam P and lam y y^H sums, 4 N M^2) and the three reductions (4 N K
    each).  The loss adds one evaluation without the a, b terms."""
    ev = 2 * N * K + 2 * N * M * (M + 1) + 4 * M ** 3 + 8 * M * M + 10 * N * M * M
    flop = F * T * (3 * ev + (ev - 10 * N * M * M + 4 * N * M * M) + 3 * 4 * N * K)
    flop_loss = F * T * (ev - 10 * N * M * M + 4 * M * M)
    X = M * F * T * 16
    ab = 2 * N * F * T * 8
    nbytes = 3 * (X + ab) + 3 * ab + X  # three evaluations write a, b; three reductions read them; spatial reads X
    return {"flop_per_iter": flop, "flop_loss": flop_loss, "bytes_per_iter": nbytes, "bytes_loss": X,
            "floor_ms": round(max(flop / PEAK_F64_FLOPS, nbytes / PEAK_HBM_BPS) * 1e3, 4),
            "floor_ms_loss": round(max((flop + flop_loss) / PEAK_F64_FLOPS, (nbytes + X) / PEAK_HBM_BPS) * 1e3, 4)}


def bench_device(M, N, K, F, T, with_loss, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((M, F, T), dtype=torch.complex128, device="cuda", generator=g)
    rng = np.random.default_rng(0)
    Z0 = rng.random((N, K)) * 1e-2 + 1 / N
    Z0 /= Z0.sum(axis=0)
    T0, V0 = rng.random((F, K)), rng.random((K, T))

    def run(n):
        model = MultichannelISNMF(n_basis=K, n_sources=N, recordable_loss=with_loss)
        model.latent, model.basis, model.activation = Z0.copy(), T0.copy(), V0.copy()
        model(X, iteration=n)
        if with_loss:
            np.asarray(model.loss)
        return model

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(0)
    torch.cuda.synchronize()
    fixed = time.perf_counter() - t0  # reset + uploads + separate: subtracted below
    t0 = time.perf_counter()
    run(iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0 - fixed) / iters


def bench_notebook(iters=200):
    """The reference notebook's call: NumPy in and out, the whole call timed (uploads, loss, output download)."""
    M, N, K, F, T = 2, 2, 30, 2049, 128
    rng = np.random.default_rng(1)
    X = rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))
    MultichannelISNMF(n_basis=K, n_sources=N)(X, iteration=2)
    torch.cuda.synchronize()
    np.random.seed(0)
    t0 = time.perf_counter()
    model = MultichannelISNMF(n_basis=K, n_sources=N, normalize=True)
    Y = model(X, iteration=iters)
    loss = np.asarray(model.loss)
    dt = time.perf_counter() - t0
    assert Y.shape == (N, F, T) and np.all(np.isfinite(loss))
    return {"shape": "notebook_m2_n2_k30_f2049_t128", "iterations": iters, "seconds_total": round(dt, 4),
            "ms_per_iter": round(dt / iters * 1e3, 4), **floors(M, N, K, F, T)}


def cpu_baseline(M, N, K, F, T):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mnmf_np as mn
    rng = np.random.default_rng(0)
    X = rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))
    Z0 = rng.random((N, K)) * 1e-2 + 1 / N
    Z0 /= Z0.sum(axis=0)
    t0 = time.perf_counter()
    mn.update_once(X, rng.random((F, K)), rng.random((K, T)), Z0, mn.init_spatial(M, N, F))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--notebook-iters", type=int, default=200)
    a = ap.parse_args()
    out = {"metric": "mnmf_ms_per_iter", "dtype": "float64", "device": torch.cuda.get_device_name(0), "results": []}
    for name, (M, N, K, F, T) in SHAPES.items():
        r = {"shape": name, "M": M, "N": N, "K": K, "F": F, "T": T, **floors(M, N, K, F, T)}
        for with_loss in (False, True):
            dt = bench_device(M, N, K, F, T, with_loss, a.iters, a.warmup)
            r["ms_per_iter_loss" if with_loss else "ms_per_iter"] = round(dt * 1e3, 4)
        out["results"].append(r)
    out["results"].append(bench_notebook(a.notebook_iters))
    if a.cpu_baseline:
        out["cpu_restatement_s_per_iter_m4_n4_k10"] = round(cpu_baseline(*SHAPES["m4_n4_k10"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
