#!/usr/bin/env python3
"""FastMultichannelISNMF iterations per second at M = N = 4, F = 1025, T = 4096 (n_basis 4 and 10, float64 and float32,
with and without the loss), through assx_fastmnmf_iterate.  Prints ONE JSON line; the algorithmic bytes of every pass
 are computed from the shapes.

    python tools/fastmnmf_bench.py [--iters 50] [--warmup 5] [--cpu-baseline] [--k 4 10] [--dtype float64 float32]

--cpu-baseline adds the seconds per iteration of the NumPy restatement (tests/fastmnmf_np.py) on this host's CPU, one
iteration at float64 (labelled as such).  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` separately.
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

from audio_source_separation_amd.bss.mnmf import FastMultichannelISNMF  # noqa: E402

M = N = 4
F, T = 1025, 4096


def pass_bytes(K, es):
    """Algorithmic bytes per pass: every array a pass must read or write once (model arrays included)."""
    X = M * F * T * 2 * es
    xt = M * F * T * es
    Rw = M * F * T * es
    H = N * K * T * es
    W = N * F * K * es
    part = min(F, 16) * 2 * N * K * T * es
    return {
        "P1_project": X + xt + H + W,
        "P2_basis": xt + H + 2 * W,
        "P3_activation": xt + W + 2 * H + 2 * part,
        "P4_scm": xt + H + W,
        "P5_mix": Rw + H + W,
        "P5_cov_ip": X + Rw,
        "P6_normalize": 2 * W + 2 * H,
    }


def bench(K, dtype, with_loss, iters, warmup):
    g = torch.Generator(device="cuda").manual_seed(0)
    cd = torch.complex128 if dtype == "float64" else torch.complex64
    X = torch.randn((M, F, T), dtype=cd, device="cuda", generator=g)
    rng = np.random.default_rng(0)
    W0, H0 = rng.random((N, F, K)), rng.random((N, K, T))

    def run(n):
        model = FastMultichannelISNMF(n_basis=K, recordable_loss=with_loss, dtype=dtype)
        model.basis, model.activation = W0.copy(), H0.copy()
        model(X, iteration=n)
        return model

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(0)
    torch.cuda.synchronize()
    fixed = time.perf_counter() - t0  # reset + uploads + separate: subtracted below
    t0 = time.perf_counter()
    model = run(iters)
    if with_loss:
        np.asarray(model.loss)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0 - fixed) / iters
    es = 8 if dtype == "float64" else 4
    pb = pass_bytes(K, es)
    total = sum(pb.values())
    return {"K": K, "dtype": dtype, "loss": with_loss, "ms_per_iter": round(dt * 1e3, 4), "it_per_s": round(1 / dt, 1),
            "bytes_per_iter": total, "effective_TBps": round(total / dt / 1e12, 3)}


def cpu_baseline(K):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fastmnmf_np as fm
    rng = np.random.default_rng(0)
    X = rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))
    W0, H0 = rng.random((N, F, K)), rng.random((N, K, T))
    Q, g = fm.initial_state(M, N, F)
    t0 = time.perf_counter()
    W, H, g, Q = fm.step(X, W0, H0, g, Q)
    fm.loss(X, W, H, g, Q)
    return {"K": K, "s_per_iter_numpy_restatement_host_cpu": round(time.perf_counter() - t0, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--k", type=int, nargs="+", default=[4, 10], help="n_basis values (profiling runs: one)")
    ap.add_argument("--dtype", nargs="+", default=["float64", "float32"])
    a = ap.parse_args()
    rows = []
    for K in a.k:
        for dtype in a.dtype:
            for with_loss in (False, True):
                rows.append(bench(K, dtype, with_loss, a.iters, a.warmup))
    out = {"metric": "fastmnmf_iterate", "M": M, "N": N, "F": F, "T": T, "iters": a.iters,
           "pass_bytes_f64": {"K4": pass_bytes(4, 8), "K10": pass_bytes(10, 8)}, "results": rows}
    if a.cpu_baseline:
        out["cpu_baseline"] = [cpu_baseline(4)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
