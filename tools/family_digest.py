#!/usr/bin/env python3
"""SHA-256 of everything the entry points of the seven factorisation families and of the four per-bin BSS families
write, for A/B runs of two builds of the library.

    ASSX_LIB_PATH=/path/to/other/libassx.so python tools/family_digest.py > a.txt
    python tools/family_digest.py > b.txt && diff a.txt b.txt

`python tools/family_digest.py factorisations` or `... perbin` prints one of the two groups alone; the lines of a group
do not depend on whether the other runs.

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
  gradient BSS    every case of `gradbss_envelope_np.GRID`: update and iterate of the four classes, both losses and
                  FDICA's permutation solver; 2 iterations
  ProxLaplaceIVA  every case of `pdsbss_envelope_np.GRID`: operator norm, adjoint, forward, both proxes, update, loss
                  and iterate; 2 iterations
  beamformers     every case of `beamform_envelope_np.GRID`: the calls of tests/test_gpu_beamform_envelope.py (`bf_*`,
                  `pca_basis`, `mdp_scale`)
  GaussIDLMA      the sizes and options of `idlma_np.CASES` from a seeded W and network output: the single entry points
                  and `idlma_step` twice, the network's next input fed back as its output

Between them the cases cross every boundary of a fixed-order sum: more than 64 frames and not a multiple of 64, 17 bases
(a second chunk of 16), 9 or more bins (a second slab), and for the MNMFs 130 frames (three spatial slices, more than
one evaluation workgroup); for the per-bin families the row split between 6 and 7 channels, a second frame chunk, a
partial last wave of frames and more than one bin slice.
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
import beamform_envelope_np as benv  # noqa: E402
import envelope_np as env  # noqa: E402
import gradbss_envelope_np as genv  # noqa: E402
import gradbss_np as gb  # noqa: E402
import idlma_np as idl  # noqa: E402
import ipsdta_np as ip  # noqa: E402
import pdsbss_envelope_np as penv  # noqa: E402
import ntf_np as nt  # noqa: E402
import psdtf_np as pt  # noqa: E402
from test_gpu_cnmf import EDGES as CNMF_CASES  # noqa: E402
from test_gpu_ipsdta import SIZE_CASES as GAUSS_CASES  # noqa: E402
from test_gpu_ntf import ENVELOPE as NTF_CASES  # noqa: E402
from test_gpu_psdtf import SIZES as PSD_SIZES  # noqa: E402
from test_gpu_tipsdta import SIZE_CASES as T_CASES  # noqa: E402
from audio_source_separation_amd import _lib  # noqa: E402
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


def dev(eng, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=eng.dev)


def gradbss(eng, case):
    M, F, T, seed = genv.GRID[case]
    X, W = genv.state(M, F, T, seed)
    Xd, ws = dev(eng, X), eng.gradbss_workspace(M, F, T)
    code = {"iva": _lib.GRADBSS_IVA, "fdica": _lib.GRADBSS_FDICA}
    for cls, (model, natural) in gb.CLASSES.items():
        Wd, status = dev(eng, W), eng.new_status(1)
        eng.gradbss_update(code[model], natural, Xd, Wd, ws, status=status)
        line(case, "gradbss_update.%s.W" % cls, Wd)
        line(case, "gradbss_update.%s.status" % cls, status)
        Wd, status, loss = dev(eng, W), eng.new_status(1), eng.empty((SHORT + 1,), dtype=torch.float64)
        eng.gradbss_iterate(SHORT, code[model], natural, Xd, Wd, ws, loss=loss, status=status)
        for name, t in (("W", Wd), ("loss", loss), ("status", status)):
            line(case, "gradbss_iterate.%s.%s" % (cls, name), t)
    for model in gb.MODELS:
        line(case, "gradbss_loss." + model, eng.gradbss_loss(code[model], Xd, dev(eng, W), ws))
    Wd = dev(eng, W)
    order, perm = eng.fdica_solve_permutation(Xd, Wd, ws)
    for name, t in (("order", order), ("perm", perm), ("W", Wd)):
        line(case, "fdica_solve_permutation." + name, t)


def pdsbss(eng, case):
    X, W, y, norm, par = penv.state(*penv.GRID[case])
    M, F, T = X.shape
    Xd, ws, status = dev(eng, X), eng.pdsbss_workspace(M, F, T), eng.new_status(1)
    nd = torch.tensor([norm], dtype=torch.float64, device=eng.dev)
    line(case, "pdsbss_operator_norm", eng.pdsbss_operator_norm(Xd, ws, status=status))
    line(case, "pdsbss_adjoint", eng.pdsbss_adjoint(Xd, nd, dev(eng, y), ws))
    line(case, "pdsbss_forward", eng.pdsbss_forward(Xd, nd, dev(eng, y), dev(eng, W)))
    line(case, "pdsbss_prox_logdet", eng.pdsbss_prox_logdet(dev(eng, W), par["mu1"], status=status))
    line(case, "pdsbss_prox_group", eng.pdsbss_prox_group(dev(eng, y), ws, C=par["C"], mu=1 / par["mu2"]))
    loss, terms = eng.empty((1,), dtype=torch.float64), eng.empty((2,), dtype=torch.float64)
    eng.pdsbss_loss(Xd, dev(eng, W), ws, C=par["C"], loss=loss, terms=terms)
    line(case, "pdsbss_loss", loss)
    line(case, "pdsbss_loss.terms", terms)
    Wd, yd = dev(eng, W), dev(eng, y)
    eng.pdsbss_update(Xd, nd, Wd, yd, ws, status=status, **par)
    line(case, "pdsbss_update.W", Wd)
    line(case, "pdsbss_update.y", yd)
    Wd, yd, loss = dev(eng, W), dev(eng, y), eng.empty((SHORT + 1,), dtype=torch.float64)
    eng.pdsbss_iterate(SHORT, Xd, nd, Wd, yd, ws, loss=loss, status=status, **par)
    for name, t in (("W", Wd), ("y", yd), ("loss", loss), ("status", status)):
        line(case, "pdsbss_iterate." + name, t)


def beamform(eng, case):
    """The calls of tests/test_gpu_beamform_envelope.py's `run`."""
    X, A, R, Ys, ref, eps = benv.state(*benv.GRID[case])
    M, F, T = X.shape
    Xd, Ad, Yd, status = dev(eng, X), dev(eng, A), dev(eng, Ys), eng.new_status(1)
    Wf, s = eng.bf_ds_weights(Ad, ref)
    for name, t in (("Wf", Wf), ("s", s)):
        line(case, "bf_ds_weights." + name, t)
    line(case, "bf_apply.ds", eng.bf_apply(Xd, Wf, s))
    Wf, s = eng.bf_ml_weights(Ad, dev(eng, R), ref, eps, status)
    for name, t in (("Wf", Wf), ("s", s)):
        line(case, "bf_ml_weights." + name, t)
    line(case, "bf_apply.ml", eng.bf_apply(Xd, Wf, s))
    line(case, "mdp_scale", eng.mdp_scale(Yd, Xd))
    line(case, "mdp_scale.one_channel", eng.mdp_scale(Yd, Xd[ref:ref + 1].contiguous()))
    C = eng.cov_accumulate(Xd.unsqueeze(0)).reshape(F, M, M)
    V, w, Wp = eng.pca_basis(C, status)
    for name, t in (("V", V), ("w", w), ("Wf", Wp)):
        line(case, "pca_basis." + name, t)
    line(case, "bf_apply.pca", eng.bf_apply(Xd, Wp))
    line(case, "beamform.status", status)


def idlma(eng, case):
    """The single entry points once, then idlma_step twice with the identity in the network's place."""
    name, M, F, T, domain, _, seed, opt = case
    rng = np.random.default_rng(5000 + seed)
    X = idl.convolutive_mixture(M, F, T, seed)
    W = np.eye(M) + 0.3 / np.sqrt(M) * env._cgauss(rng, (F, M, M))
    raw = (0.05 + rng.random((M, F, T))).astype(np.float32)
    flooring, ref = opt.get("dnn_flooring", 1e-5), opt.get("reference_id", 0)
    Xd, ws = dev(eng, X), eng.idlma_workspace(M, F, T)
    line(name, "idlma_dnn_input", eng.idlma_dnn_input(Xd, dev(eng, W), domain=domain))
    d, R = eng.empty((M, F, T), dtype=torch.float32), eng.empty((M, F, T), dtype=torch.float64)
    eng.idlma_variance(dev(eng, raw), d, R, domain=domain, dnn_flooring=flooring, eps=EPS)
    line(name, "idlma_variance.dnn_output", d)
    line(name, "idlma_variance.R", R)
    line(name, "idlma_loss", eng.idlma_loss(Xd, dev(eng, W), R, ws))
    Wd = dev(eng, W)
    eng.idlma_normalize_pb(Wd, dev(eng, env._cgauss(rng, (M, F))))
    line(name, "idlma_normalize_pb", Wd)
    Wd, status = dev(eng, W), eng.new_status(1)
    eng.idlma_space_update(Xd.unsqueeze(0), Wd.unsqueeze(0), R.unsqueeze(0), domain=2, eps=float(np.float32(EPS)),
                           status=status)
    line(name, "idlma_space_update.W", Wd)
    line(name, "idlma_space_update.status", status)
    Wd, status, out = dev(eng, W), eng.new_status(1), dev(eng, raw)
    for i in range(SHORT):
        loss, inp = eng.empty((1,), dtype=torch.float64), eng.empty((M, F, T), dtype=torch.float32)
        eng.idlma_step(Xd, Wd, out, d, ws, domain=domain, dnn_flooring=flooring, eps=EPS, ref=ref, loss=loss,
                       next_input=inp, status=status)
        for what, t in (("W", Wd), ("dnn_output", d), ("loss", loss), ("next_input", inp), ("status", status)):
            line(name, "idlma_step.%d.%s" % (i, what), t)
        out = inp


def factorisations():
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


def perbin():
    eng = Engine(dtype="float64", device="cuda:0")
    for case in genv.GRID:
        gradbss(eng, case)
    for case in penv.GRID:
        pdsbss(eng, case)
    for case in benv.GRID:
        beamform(eng, case)
    for case in idl.CASES:
        idlma(eng, case)


def main():
    groups = {"factorisations": factorisations, "perbin": perbin}
    unknown = [name for name in sys.argv[1:] if name not in groups]
    if unknown:
        sys.exit("family_digest.py: unknown group %s; the groups are %s" % (", ".join(unknown), ", ".join(groups)))
    for name in sys.argv[1:] or groups:
        groups[name]()


if __name__ == "__main__":
    main()
