#!/usr/bin/env python3
"""SHA-256 of everything the entry points of the seven factorisation families write, for A/B runs of two builds of the
library.

    ASSX_LIB_PATH=/path/to/other/libassx.so python tools/family_digest.py > a.txt
    python tools/family_digest.py > b.txt && diff a.txt b.txt

One line `case entry sha256` per output array.  No tolerance and no reference: every family promises fixed-order sums,
so two builds that compute the same sums print the same lines.  Every `Engine.*` entry point of a family is called once
from a seeded state; `*_iterate` runs with the loss on.  The states are the ones the GPU tests use:

  MNMF, FastMNMF  every case of `envelope_np.MNMF_GRID` / `FASTMNMF_GRID` (the latter in float64 and float32), the way
                  tests/test_gpu_mnmf_envelope.py and tests/test_gpu_fastmnmf_envelope.py call them; 3 iterations
  CovNMF          every case of `covnmf_envelope_np.GRID`; 2 iterations
  ComplexEUCNMF   `EDGES` of tests/test_gpu_cnmf.py; 2 iterations
  EUCNTF          `ENVELOPE` of tests/test_gpu_ntf.py; 2 iterations
  LDPSDTF         `psdtf_to_psd` on `psdtf_np.psd_cases` of every size of the test; the first recorded state of every
                  fixture of tests/golden/psdtf; 2 iterations.  The fixtures stop at 4 bases, so one case of the
                  tool's own (9 bins, 130 frames, 17 bases) crosses the 8-basis pass and the 64-frame slabs of the
                  contraction
  IPSDTA          `ipsdta_to_psd` on seeded Hermitian matrices of every size 1..8, half of them indefinite (the Jacobi
                  branch); every case of `SIZE_CASES` of tests/test_gpu_ipsdta.py and tests/test_gpu_tipsdta.py from the
                  test's seeded start; the spatial update and `*_iterate` (2 iterations) run 2 sweeps, and none where
                  there are fewer frames than channels, as in the tests

Between them the cases cross every boundary of a fixed-order sum: more than 64 frames and not a multiple of 64, 17 bases
(a second chunk of 16), 9 or more bins (a second slab), and for the MNMFs 130 frames (three spatial slices, more than
one evaluation workgroup).
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cnmf_np as cn  # noqa: E402
import covnmf_envelope_np as cvenv  # noqa: E402
import envelope_np as env  # noqa: E402
import ipsdta_np as ip  # noqa: E402
import ntf_np as nt  # noqa: E402
import psdtf_np as pt  # noqa: E402
from test_gpu_cnmf import EDGES as CNMF_CASES  # noqa: E402
from test_gpu_ipsdta import SIZE_CASES as GAUSS_CASES  # noqa: E402
from test_gpu_ntf import ENVELOPE as NTF_CASES  # noqa: E402
from test_gpu_psdtf import SIZES as PSD_SIZES  # noqa: E402
from test_gpu_tipsdta import SIZE_CASES as T_CASES  # noqa: E402
from audio_source_separation_amd.ops import Engine  # noqa: E402

ITERATIONS = 3       # MNMF and FastMNMF
SHORT = 2            # every other family
EPS = 1e-12
PSDTF_OWN = (9, 130, 17, 5)  # n_bins, n_frames, n_basis, seed


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


def covnmf(eng, case):
    M, K, F, T, _ = cvenv.GRID[case]
    fresh = uploader(eng, [cvenv.case_state(case)])  # the model has no batch axis
    ws = eng.covnmf_workspace(M, F, T, K)

    def start():
        return [t[0] for t in fresh()], eng.new_status(1)

    for i, step in enumerate(("update_basis", "update_activation")):
        dev, status = start()
        getattr(eng, "covnmf_" + step)(*dev, ws, eps=EPS, status=status)
        line(case, "covnmf_" + step, dev[i + 1])
        line(case, "covnmf_" + step + ".status", status)
    for normalize in (True, False):
        dev, status = start()
        eng.covnmf_update_spatial(*dev, ws, normalize=normalize, eps=EPS, status=status)
        line(case, "covnmf_update_spatial.normalize=%d" % normalize, dev[3])
        line(case, "covnmf_update_spatial.normalize=%d.status" % normalize, status)
    dev, status = start()
    line(case, "covnmf_reconstruct", eng.covnmf_reconstruct(*dev[1:]))
    line(case, "covnmf_loss", eng.covnmf_loss(*dev, ws, eps=EPS, status=status))
    line(case, "covnmf_loss.status", status)
    dev, status = start()
    loss = eng.empty((SHORT,), dtype=torch.float64)
    eng.covnmf_iterate(SHORT, *dev, ws, eps=EPS, loss=loss, status=status)
    for name, t in zip(("Tb", "V", "H", "loss", "status"), dev[1:] + [loss, status]):
        line(case, "covnmf_iterate." + name, t)


def cnmf(eng, F, T, K, p):
    tag = "f%d_t%d_k%d_p%g" % (F, T, K, p)
    fresh = uploader(eng, [cn.synthetic(F, T, K, seed=F * 1000 + T * 7 + K)])
    ws = eng.cnmf_workspace(1, F, T, K)
    X, Tb, V, Phi = fresh()
    eng.cnmf_update(X, Tb, V, Phi, ws, regularizer=0.1, p=p, eps=EPS)
    for name, t in (("Tb", Tb), ("V", V), ("Phi", Phi)):
        line(tag, "cnmf_update." + name, t)
    X, Tb, V, Phi = fresh()
    line(tag, "cnmf_loss", eng.cnmf_loss(X, Tb, V, Phi, ws, eps=EPS))
    line(tag, "cnmf_beta", eng.cnmf_beta(Tb, V, eps=EPS))
    line(tag, "cnmf_reconstruct", eng.cnmf_reconstruct(Tb, V, Phi))
    loss = eng.empty((SHORT, 1), dtype=torch.float64)
    eng.cnmf_iterate(SHORT, X, Tb, V, Phi, ws, regularizer=0.1, p=p, eps=EPS, loss=loss)
    for name, t in (("Tb", Tb), ("V", V), ("Phi", Phi), ("loss", loss)):
        line(tag, "cnmf_iterate." + name, t)


def ntf(eng, N, I, J, K):
    tag = "n%d_i%d_j%d_k%d" % (N, I, J, K)
    fresh = uploader(eng, [nt.synthetic(N, I, J, K, seed=N * 100000 + I * 1000 + J * 7 + K)])
    ws = eng.ntf_workspace(1, N, I, J, K)
    X, Z, Tb, V = fresh()
    eng.ntf_update(X, Z, Tb, V, ws, eps=EPS)
    for name, t in (("Z", Z), ("Tb", Tb), ("V", V)):
        line(tag, "ntf_update." + name, t)
    X, Z, Tb, V = fresh()
    line(tag, "ntf_loss", eng.ntf_loss(X, Z, Tb, V, ws))
    line(tag, "ntf_reconstruct", eng.ntf_reconstruct(Z, Tb, V))
    loss = eng.empty((SHORT, 1), dtype=torch.float64)
    eng.ntf_iterate(SHORT, X, Z, Tb, V, ws, eps=EPS, loss=loss)
    for name, t in (("Z", Z), ("Tb", Tb), ("V", V), ("loss", loss)):
        line(tag, "ntf_iterate." + name, t)


def psdtf_to_psd(eng):
    for n in PSD_SIZES:
        for kind, A in pt.psd_cases(n, 40 + n):
            Ad = torch.from_numpy(A).to(eng.dev).contiguous()
            line("n%d_%s" % (n, kind), "psdtf_to_psd", eng.psdtf_to_psd(Ad, eps=1e-3))


def psdtf(eng, tag, X, V, H, eps, normalize):
    """X (T,M,M), V (K,M,M), H (K,T)"""
    fresh = uploader(eng, [(X, V, H)])
    K, M, T = V.shape[0], V.shape[1], H.shape[1]
    ws = eng.psdtf_workspace(1, M, T, K)

    def call(entry, written, *args, **kw):
        X, V, H = fresh()
        status = eng.new_status(1)
        getattr(eng, "psdtf_" + entry)(X, V, H, *args, eps=eps, status=status, **kw)
        for name in written:
            line(tag, "psdtf_%s.%s" % (entry, name), {"V": V, "H": H}[name])
        line(tag, "psdtf_%s.status" % entry, status)

    call("update_basis", "V", ws)
    call("update_activation", "H")
    call("update", "VH", ws, normalize=normalize)
    X, V, H = fresh()
    eng.psdtf_normalize(V, H)
    line(tag, "psdtf_normalize.V", V)
    line(tag, "psdtf_normalize.H", H)
    X, V, H = fresh()
    status = eng.new_status(1)
    line(tag, "psdtf_loss", eng.psdtf_loss(X, V, H, ws, eps=eps, status=status))
    line(tag, "psdtf_loss.status", status)
    line(tag, "psdtf_reconstruct", eng.psdtf_reconstruct(V, H))
    status, loss = eng.new_status(1), eng.empty((SHORT, 1), dtype=torch.float64)
    eng.psdtf_iterate(SHORT, X, V, H, ws, eps=eps, normalize=normalize, loss=loss, status=status)
    for name, t in (("V", V), ("H", H), ("loss", loss), ("status", status)):
        line(tag, "psdtf_iterate." + name, t)


def ipsdta_to_psd(eng):
    for n in range(1, 9):
        rng = np.random.default_rng(40 + n)
        A = rng.standard_normal((64, n, n)) + 1j * rng.standard_normal((64, n, n))
        A[:32] = A[:32] @ A[:32].conj().transpose(0, 2, 1)  # positive semi-definite; the rest indefinite once hermitized
        line("n%d" % n, "ipsdta_to_psd", eng.ipsdta_to_psd(torch.from_numpy(A).to(eng.dev).contiguous(), eps=EPS))


def ipsdta(eng, case):
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
    status, loss = eng.new_status(1), eng.empty((SHORT,), dtype=torch.float64)
    getattr(eng, pre + "iterate")(SHORT, sp, X, W, U, H, ws, nblk, *nu, eps=EPS, loss=loss, status=status)
    for name, t in (("W", W), ("U", U), ("H", H), ("loss", loss), ("status", status)):
        line(tag, "%siterate.%s" % (pre, name), t)


def main():
    for case in env.MNMF_GRID:
        mnmf(case)
    for case in env.FASTMNMF_GRID:
        for dtype in ("float64", "float32"):
            fastmnmf(case, dtype)
    eng = Engine(dtype="float64", device="cuda:0")
    ipsdta_to_psd(eng)
    for case in GAUSS_CASES + T_CASES:
        ipsdta(eng, case)
    for case in cvenv.GRID:
        covnmf(eng, case)
    for F, T, K, p in CNMF_CASES:
        cnmf(eng, F, T, K, p)
    for d in NTF_CASES:
        ntf(eng, d["N"], d["I"], d["J"], d["K"])
    psdtf_to_psd(eng)
    for f in pt.fixture_files():
        fx = np.load(f)
        V, H = pt.state(fx, 0)
        psdtf(eng, os.path.basename(f)[:-4], pt.frames_first(fx["X"]), pt.kmm(V), H, float(fx["eps"]),
              bool(fx["normalize"]))
    M, T, K, seed = PSDTF_OWN
    psdtf(eng, "own_m%d_t%d_k%d" % (M, T, K), *pt.synthetic(M, T, K, seed), EPS, True)


if __name__ == "__main__":
    main()
