#!/usr/bin/env python3
"""SHA-256 of everything the GaussIPSDTA and tIPSDTA entry points write, for A/B runs of two builds of the library.

    ASSX_LIB_PATH=/path/to/other/libassx.so python tools/ipsdta_digest.py > a.txt
    python tools/ipsdta_digest.py > b.txt && diff a.txt b.txt

`ipsdta_to_psd` runs on seeded Hermitian matrices of every size 1..8, half of them indefinite (the Jacobi branch).  For
every case of `SIZE_CASES` in tests/test_gpu_ipsdta.py and tests/test_gpu_tipsdta.py the test's seeded start
(`ipsdta_np.synthetic`) is uploaded and every `Engine.ipsdta_*` / `Engine.tipsdta_*` entry point is called once from
that start; the spatial update and `*_iterate` (2 iterations, the loss on) run 2 sweeps, and none where there are fewer
frames than channels, as in the tests.  One line `case entry sha256` per output array.  No tolerance and no reference:
both models promise fixed-order sums, so two builds that compute the same sums print the same lines.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ipsdta_np as ip  # noqa: E402
from test_gpu_ipsdta import SIZE_CASES as GAUSS_CASES  # noqa: E402
from test_gpu_tipsdta import SIZE_CASES as T_CASES  # noqa: E402
from audio_source_separation_amd.ops import Engine  # noqa: E402

ITERATIONS = 2
EPS = 1e-12


def line(case, entry, tensor):
    a = np.ascontiguousarray(tensor.cpu().numpy())
    print(case, entry, hashlib.sha256(a.tobytes()).hexdigest())


def to_psd(eng):
    for n in range(1, 9):
        rng = np.random.default_rng(40 + n)
        A = rng.standard_normal((64, n, n)) + 1j * rng.standard_normal((64, n, n))
        A[:32] = A[:32] @ A[:32].conj().transpose(0, 2, 1)  # positive semi-definite; the rest indefinite once hermitized
        line("n%d" % n, "ipsdta_to_psd", eng.ipsdta_to_psd(torch.from_numpy(A).to(eng.dev).contiguous(), eps=EPS))


def model(eng, case):
    """Every entry point of the Gauss model (a case of 5) or of the t model (a case of 6: nu last)."""
    M, F, T, K, nblk = case[:5]
    nu = tuple(case[5:])
    pre = "tipsdta_" if nu else "ipsdta_"
    tag = "m%d_f%d_t%d_k%d_b%d" % case[:5] + ("_nu%g" % nu if nu else "")
    sp = 2 if T >= M else 0
    host = ip.synthetic(M, F, T, K, nblk, 7000 + sum(case[:5]))
    host = (host[0], host[1], ip.pack(host[2]), host[3])
    ws = getattr(eng, pre + "workspace")(M, F, T, K, nblk, *nu)

    def fresh():
        return [torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev).contiguous() for a in host]

    def call(entry, written, **kw):
        X, W, U, H = fresh()
        status = eng.new_status(1)
        getattr(eng, pre + entry)(X, W, U, H, ws, nblk, *nu, eps=EPS, status=status, **kw)
        for name in written:
            line(tag, "%s%s.%s" % (pre, entry, name), {"W": W, "U": U, "H": H}[name])
        line(tag, "%s%s.status" % (pre, entry), status)

    call("update_basis", "U")
    call("update_activation", "H")
    for normalize in (True, False):
        call("update_source", "UH", normalize=normalize)
    call("update_spatial", "W", n_sweeps=sp)
    loss = eng.empty((1,), dtype=torch.float64)
    call("loss", "", loss=loss)
    line(tag, pre + "loss.loss", loss)
    if not nu:
        X, W, U, H = fresh()
        eng.ipsdta_normalize(U, H, F, nblk)
        line(tag, "ipsdta_normalize.U", U)
        line(tag, "ipsdta_normalize.H", H)
    X, W, U, H = fresh()
    status, loss = eng.new_status(1), eng.empty((ITERATIONS,), dtype=torch.float64)
    getattr(eng, pre + "iterate")(ITERATIONS, sp, X, W, U, H, ws, nblk, *nu, eps=EPS, loss=loss, status=status)
    for name, t in (("W", W), ("U", U), ("H", H), ("loss", loss), ("status", status)):
        line(tag, "%siterate.%s" % (pre, name), t)


def main():
    eng = Engine(dtype="float64", device="cuda:0")
    to_psd(eng)
    for case in GAUSS_CASES + T_CASES:
        model(eng, case)


if __name__ == "__main__":
    main()
