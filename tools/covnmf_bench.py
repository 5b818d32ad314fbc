#!/usr/bin/env python3
"""Covariance-domain MultichannelISNMF milliseconds per `update_once` (assx_covnmf_iterate without a loss) and per loss
(assx_covnmf_loss) on the device, at n_bins = 513, n_frames = 512, n_basis = 10 and n_channels in {4, 2, 8}.  Prints ONE
JSON line.

    python tools/covnmf_bench.py [--iters 5] [--warmup 2] [--repeats 5] [--channels 4 2 8]

A figure is the median over `repeats` windows of `iters` iterations each, every window between two device
synchronisations on the host clock, after `warmup` iterations; clocks are whatever the device runs at (nothing is
pinned), and the device's name is printed.  The state is the general one of the envelope sweep
(tests/covnmf_envelope_np.py); every window starts from the same copy of it.
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

F, T, K = 513, 512, 10


def bench(M, iters, warmup, repeats):
    import numpy as np
    import torch
    import covnmf_envelope_np as cenv
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype="float64")
    X, Tb0, V0, H0 = (torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev) for a in cenv.state(M, K, F, T, 500 + M))
    ws = eng.covnmf_workspace(M, F, T, K)
    status = eng.new_status(1)
    loss = eng.empty((1,), dtype=torch.float64)

    def window(n, what):
        Tb, V, H = Tb0.clone(), V0.clone(), H0.clone()
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        if what == "update_once":
            eng.covnmf_iterate(n, X, Tb, V, H, ws, status=status)
        else:
            for _ in range(n):
                eng.covnmf_loss(X, Tb, V, H, ws, loss=loss, status=status)
        torch.cuda.synchronize(eng.dev)
        dt = time.perf_counter() - t0
        assert all(bool(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all()) for a in (Tb, V, H))
        assert int(status.max().item()) == 0
        return dt / max(n, 1)

    out = {"n_channels": M, "workspace_MiB": round(ws.numel() / 2 ** 20, 1)}
    for what in ("update_once", "loss"):
        window(warmup, what)
        times = [window(iters, what) for _ in range(repeats)]
        out["ms_per_" + what] = round(statistics.median(times) * 1e3, 3)
        out["ms_per_%s_min_max" % what] = [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--channels", type=int, nargs="+", default=[4, 2, 8])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("covnmf_bench.py needs a GPU: a timing taken anywhere else says nothing")
    out = {"metric": "covnmf_ms_per_update_once", "dtype": "float64", "device": torch.cuda.get_device_name(0),
           "clocks": "not pinned", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "statistic": "median",
           "n_bins": F, "n_frames": T, "n_basis": K, "results": [bench(M, a.iters, a.warmup, a.repeats) for M in a.channels]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
