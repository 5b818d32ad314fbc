#!/usr/bin/env python3
"""SHA-256 of everything the MNMF and FastMNMF entry points write, for A/B runs of two builds of the library.

    ASSX_LIB_PATH=/path/to/other/libassx.so python tools/mnmf_digest.py > a.txt
    python tools/mnmf_digest.py > b.txt && diff a.txt b.txt

For every case of `envelope_np.MNMF_GRID` and `envelope_np.FASTMNMF_GRID` (the latter in float64 and float32) the
grid's seeded state is uploaded and every `Engine.mnmf_*` / `Engine.fastmnmf_*` entry point is called once from that
state, the way tests/test_gpu_mnmf_envelope.py and tests/test_gpu_fastmnmf_envelope.py call them; the two `*_iterate`
entries run 3 iterations with the loss on.  One line `case entry sha256` per output array.  No tolerance and no
reference: both models promise fixed-order reductions, so two builds that compute the same sums print the same lines.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import envelope_np as env  # noqa: E402
from audio_source_separation_amd.ops import Engine  # noqa: E402

ITERATIONS = 3


def line(case, entry, tensor):
    a = np.ascontiguousarray(tensor.cpu().numpy())
    print(case, entry, hashlib.sha256(a.tobytes()).hexdigest())


def uploader(eng, states):
    """A function that returns fresh device copies of the seeded state, batch axis first."""
    host = [np.ascontiguousarray(np.stack([s[i] for s in states])) for i in range(len(states[0]))]

    def fresh():
        out = []
        for a in host:
            t = torch.from_numpy(a)
            out.append(t.to(eng.prec.cplx if t.is_complex() else eng.prec.real).to(eng.dev).contiguous())
        return out
    return fresh


def mnmf(case):
    M, N, K, F, T, seeds = env.MNMF_GRID[case]
    B = len(seeds)
    eng = Engine(device="cuda:0")
    fresh = uploader(eng, env.mnmf_states(case))
    ws = eng.mnmf_workspace(B, M, N, F, T, K)
    for i, step in enumerate(("update_basis", "update_activation", "update_latent")):
        dev, status = fresh(), eng.new_status(B)
        getattr(eng, "mnmf_" + step)(*dev, ws, status=status)
        line(case, "mnmf_" + step, dev[i + 1])
        line(case, "mnmf_" + step + ".status", status)
    for normalize in (True, False):
        dev, status = fresh(), eng.new_status(B)
        eng.mnmf_update_spatial(*dev, ws, normalize=normalize, status=status)
        line(case, "mnmf_update_spatial.normalize=%d" % normalize, dev[4])
        line(case, "mnmf_update_spatial.normalize=%d.status" % normalize, status)
    dev, status = fresh(), eng.new_status(B)
    line(case, "mnmf_loss", eng.mnmf_loss(*dev, ws, status=status))
    for r in env.reference_ids(M):
        line(case, "mnmf_separate.ref=%d" % r, eng.mnmf_separate(*dev, ref=r, status=status))
    line(case, "mnmf_loss+separate.status", status)
    dev, status = fresh(), eng.new_status(B)
    loss = eng.empty((ITERATIONS + 1, B), dtype=torch.float64)
    eng.mnmf_iterate(ITERATIONS, *dev, ws, status=status, loss=loss)
    for name, t in zip(("Tb", "V", "Z", "H"), dev[1:]):
        line(case, "mnmf_iterate." + name, t)
    line(case, "mnmf_iterate.loss", loss)
    line(case, "mnmf_iterate.status", status)


def fastmnmf(case, dtype):
    M, N, K, F, T, seeds = env.FASTMNMF_GRID[case]
    B = len(seeds)
    eng = Engine(dtype=dtype, device="cuda:0")
    fresh = uploader(eng, env.fastmnmf_states(case, dtype))
    ws = eng.fastmnmf_workspace(B, M, N, F, T, K)
    tag = case + "/" + dtype

    X, W, H, g, Q = fresh()
    loss = eng.empty((B,), dtype=torch.float64)
    eng.fastmnmf_project(X, Q, W, H, g, ws, loss=loss)
    line(tag, "fastmnmf_project.loss", loss)
    X, W, H, g, Q = fresh()
    eng.fastmnmf_project(X, Q, W, H, g, ws)  # x~ is internal: the two updates below read it
    eng.fastmnmf_update_nmf(X, W, H, g, ws)
    line(tag, "fastmnmf_update_nmf.W", W)
    line(tag, "fastmnmf_update_nmf.H", H)
    X, W, H, g, Q = fresh()
    eng.fastmnmf_project(X, Q, W, H, g, ws)
    eng.fastmnmf_update_scm(X, W, H, g, ws)
    line(tag, "fastmnmf_update_scm.g", g)
    X, W, H, g, Q = fresh()
    status = eng.new_status(B)
    eng.fastmnmf_update_diagonalizer_model(X, Q, W, H, g, ws, status=status)
    line(tag, "fastmnmf_update_diagonalizer_model.Q", Q)
    line(tag, "fastmnmf_update_diagonalizer_model.status", status)
    X, W, H, g, Q = fresh()
    eng.fastmnmf_normalize_power(X, Q, W, H, g)
    for name, t in zip(("W", "H", "g", "Q"), (W, H, g, Q)):
        line(tag, "fastmnmf_normalize_power." + name, t)
    X, W, H, g, Q = fresh()
    status = eng.new_status(B)
    for r in env.reference_ids(M):
        line(tag, "fastmnmf_separate.ref=%d" % r, eng.fastmnmf_separate(X, Q, W, H, g, ref=r, status=status))
    line(tag, "fastmnmf_separate.status", status)
    X, W, H, g, Q = fresh()
    status = eng.new_status(B)
    loss = eng.empty((ITERATIONS + 1, B), dtype=torch.float64)
    eng.fastmnmf_iterate(ITERATIONS, X, Q, W, H, g, ws, status=status, loss=loss)
    for name, t in zip(("W", "H", "g", "Q"), (W, H, g, Q)):
        line(tag, "fastmnmf_iterate." + name, t)
    line(tag, "fastmnmf_iterate.loss", loss)
    line(tag, "fastmnmf_iterate.status", status)


def main():
    for case in env.MNMF_GRID:
        mnmf(case)
    for case in env.FASTMNMF_GRID:
        for dtype in ("float64", "float32"):
            fastmnmf(case, dtype)


if __name__ == "__main__":
    main()
