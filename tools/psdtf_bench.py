#!/usr/bin/env python3
"""LDPSDTF milliseconds per update and per loss on the device (assx_psdtf_iterate without a loss; assx_psdtf_loss), at
n_bins in {16, 32, 64}, n_frames = 1024, n_basis = 8, batch 1 and 8, each next to the time the NumPy restatement
(tests/psdtf_np.py on numpy.linalg) takes for ONE problem of the batch on the same host.  Prints ONE JSON line.

    python tools/psdtf_bench.py [--iters 10] [--warmup 2] [--repeats 5] [--bins 16 32 64]

A device figure is the median over `repeats` windows of `iters` calls each, every window between two device
synchronisations on the host clock; clocks are whatever the device runs at (nothing is pinned), and the device's name is
printed.  The restatement is timed once per shape (it takes seconds).
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

T, K = 1024, 8


def problem(M, B):
    import numpy as np
    import psdtf_np as pt
    Xs, Vs, Hs = zip(*(pt.synthetic(M, T, K, 100 + b) for b in range(B)))
    V, H = zip(*(pt.normalize(v, h) for v, h in zip(Vs, Hs)))
    return np.stack(Xs), np.stack(V), np.stack(H)


def bench_device(X, V, H, iters, warmup, repeats):
    import torch
    from audio_source_separation_amd._device import to_device
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype="float64")
    Xd, V0, H0 = (to_device(a, torch.float64, eng.dev) for a in (X, V, H))
    B, _, M = V0.shape[:3]
    ws = eng.psdtf_workspace(B, M, T, K)
    status = eng.new_status(B)
    loss = eng.empty((B,), dtype=torch.float64)

    def window(n, what):
        Vd, Hd = V0.clone(), H0.clone()
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        if what == "update":
            eng.psdtf_iterate(n, Xd, Vd, Hd, ws, status=status)
        else:
            for _ in range(n):
                eng.psdtf_loss(Xd, Vd, Hd, ws, loss=loss, status=status)
        torch.cuda.synchronize(eng.dev)
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(Vd).all()) and bool(torch.isfinite(Hd).all()) and int(status.max().item()) == 0
        return dt / max(n, 1)

    out = {}
    for what in ("update", "loss"):
        window(warmup, what)
        times = [window(iters, what) for _ in range(repeats)]
        out["ms_per_" + what] = round(statistics.median(times) * 1e3, 4)
        out["ms_per_%s_min_max" % what] = [round(min(times) * 1e3, 4), round(max(times) * 1e3, 4)]
    return out


def bench_restatement(X, V, H):
    import psdtf_np as pt
    t0 = time.perf_counter()
    Vn, Hn = pt.update(X, V, H, 1e-12)
    t1 = time.perf_counter()
    pt.loss(X, Vn, Hn, 1e-12)
    t2 = time.perf_counter()
    return {"restatement_ms_per_update_one_problem": round((t1 - t0) * 1e3, 1),
            "restatement_ms_per_loss_one_problem": round((t2 - t1) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bins", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("psdtf_bench.py needs a GPU: a timing taken anywhere else says nothing")
    out = {"metric": "psdtf_ms_per_update", "dtype": "float64", "device": torch.cuda.get_device_name(0),
           "clocks": "not pinned", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "statistic": "median",
           "n_frames": T, "n_basis": K, "results": []}
    for M in a.bins:
        for B in a.batches:
            X, V, H = problem(M, B)
            r = {"n_bins": M, "B": B}
            r.update(bench_device(X, V, H, a.iters, a.warmup, a.repeats))
            if B == a.batches[0]:
                host = bench_restatement(X[0], V[0], H[0])
            r.update(host)
            out["results"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
