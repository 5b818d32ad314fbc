#!/usr/bin/env python3
"""GaussIPSDTA and tIPSDTA milliseconds per iteration and per loss on the device (assx_[t]ipsdta_iterate without a loss;
assx_[t]ipsdta_loss), each next to the time the NumPy restatement (tests/ipsdta_np.py, tests/tipsdta_np.py on numpy.linalg)
takes for the same problem on the same host.  The iteration is also timed in its two parts, assx_[t]ipsdta_update_source and
assx_[t]ipsdta_update_spatial with all its sweeps, and the t model next to assx_ipsdta_iterate (the Gauss model) at the same
shape in the same run for scale.  nu = 1.  Prints ONE JSON line per model.

    python tools/ipsdta_bench.py [--model gauss|t|both] [--iters 5] [--warmup 1] [--repeats 5] [--no-restatement]

Shapes (n_channels, n_bins, n_frames, n_basis, spatial_iteration, n_blocks): (2, 513, 256, 10, 10, 128), blocks of 4 and one
of 5, and the same with 512 blocks, blocks of 1 and one of 2.  A device figure is the median over `repeats` windows of
`iters` iterations each, every window between two device synchronisations on the host clock; clocks are whatever the device
runs at (nothing is pinned), and the device's name is printed.  The restatement is timed once per shape (it takes seconds).
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

SHAPES = ((2, 513, 256, 10, 10, 128), (2, 513, 256, 10, 10, 512))
EPS = 1e-12
NU = 1.0


def bench_device(model, X, W, U, H, sp, nblk, iters, warmup, repeats):
    import torch
    import ipsdta_np as ip
    from audio_source_separation_amd._device import to_device
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype="float64")
    Xd, W0, U0 = (to_device(a, torch.complex128, eng.dev) for a in (X, W, ip.pack(U)))
    H0 = to_device(H, torch.float64, eng.dev)
    M, F, T = X.shape
    ws_gauss = eng.ipsdta_workspace(M, F, T, H.shape[1], nblk)
    # the entry points of the model, its workspace and, for the t model, nu
    if model == "gauss":
        pre, ws, nu = "ipsdta_", ws_gauss, ()
    else:
        pre, ws, nu = "tipsdta_", eng.tipsdta_workspace(M, F, T, H.shape[1], nblk, NU), (NU,)
    status = eng.new_status(1)
    loss = eng.empty((1,), dtype=torch.float64)

    def window(n, what):
        Wd, Ud, Hd = W0.clone(), U0.clone(), H0.clone()
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        if what == "iteration":
            getattr(eng, pre + "iterate")(n, sp, Xd, Wd, Ud, Hd, ws, nblk, *nu, eps=EPS, status=status)
        elif what == "source_update":
            for _ in range(n):
                getattr(eng, pre + "update_source")(Xd, Wd, Ud, Hd, ws, nblk, *nu, eps=EPS, status=status)
        elif what == "spatial_update":
            for _ in range(n):
                getattr(eng, pre + "update_spatial")(Xd, Wd, Ud, Hd, ws, nblk, *nu, n_sweeps=sp, eps=EPS, status=status)
        elif what == "gauss_iteration":
            eng.ipsdta_iterate(n, sp, Xd, Wd, Ud, Hd, ws_gauss, nblk, eps=EPS, status=status)
        else:
            for _ in range(n):
                getattr(eng, pre + "loss")(Xd, Wd, Ud, Hd, ws, nblk, *nu, eps=EPS, loss=loss, status=status)
        torch.cuda.synchronize(eng.dev)
        dt = time.perf_counter() - t0
        assert all(bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all()) for t in (Wd, Ud, Hd))
        assert int(status.item()) == 0
        return dt / max(n, 1)

    out = {}
    for what in ("iteration", "loss", "source_update", "spatial_update") + (("gauss_iteration",) if model == "t" else ()):
        window(warmup, what)
        times = [window(iters, what) for _ in range(repeats)]
        out["ms_per_" + what] = round(statistics.median(times) * 1e3, 4)
        out["ms_per_%s_min_max" % what] = [round(min(times) * 1e3, 4), round(max(times) * 1e3, 4)]
    return out


def bench_restatement(model, X, W, U, H, sp, nblk):
    import ipsdta_np as ip
    import tipsdta_np as tp
    rs, nu = (ip, ()) if model == "gauss" else (tp, (NU,))
    t0 = time.perf_counter()
    Un, Hn = rs.update_source(X, W, U, H, EPS, nblk, *nu)
    Wn = rs.update_spatial(X, W, Un, Hn, EPS, nblk, *nu, sp)
    t1 = time.perf_counter()
    rs.loss(X, Wn, Un, Hn, EPS, nblk, *nu)
    t2 = time.perf_counter()
    return {"restatement_ms_per_iteration": round((t1 - t0) * 1e3, 1), "restatement_ms_per_loss": round((t2 - t1) * 1e3, 1)}


def launches(M, F, sp, nblk):
    """kernel launches of one t iteration without a loss"""
    g = 2 if F % nblk else 1  # block sizes present
    steps = M * (F // nblk + (F // nblk + 1 if F % nblk else 0))
    return (2 * g + 2) + (g + 2) + 1 + g + (1 + 2 * steps) * sp


def bench_model(model, a):
    import torch
    import ipsdta_np as ip
    out = {"metric": ("ipsdta" if model == "gauss" else "tipsdta") + "_ms_per_iteration", "dtype": "float64"}
    if model == "t":
        out["nu"] = NU
    out.update({"device": torch.cuda.get_device_name(0), "clocks": "not pinned", "iters": a.iters, "warmup": a.warmup,
                "repeats": a.repeats, "statistic": "median", "results": []})
    for M, F, T, K, sp, nblk in SHAPES:
        X, W, U, H = ip.synthetic(M, F, T, K, nblk, 100)
        r = {"n_channels": M, "n_bins": F, "n_frames": T, "n_basis": K, "spatial_iteration": sp, "n_blocks": nblk}
        if model == "t":
            r["launches_per_iteration"] = launches(M, F, sp, nblk)
        r.update(bench_device(model, X, W, U, H, sp, nblk, a.iters, a.warmup, a.repeats))
        if not a.no_restatement:
            r.update(bench_restatement(model, X, W, U, H, sp, nblk))
        out["results"].append(r)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("gauss", "t", "both"), default="both")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ipsdta_bench.py needs a GPU: a timing taken anywhere else says nothing")
    for model in ("gauss", "t") if a.model == "both" else (a.model,):
        bench_model(model, a)


if __name__ == "__main__":
    main()
