"""FastMultichannelISNMF's kernels over the whole size envelope, one entry point at a time, in float64 and float32.

For every case of `envelope_np.FASTMNMF_GRID` ONE general state is built on the host from a seeded generator (X complex
Gaussian with a per-bin scale; W, H, g uniform in [0.05, 1.05]; Q = I + 0.3 / sqrt(M) x complex Gaussian, cond(Q) < 1e3
asserted), uploaded, and ONE entry point of `Engine` is called on it: `fastmnmf_project` (x~ is internal: checked through
the loss it returns and through the two updates that read it), `fastmnmf_update_nmf`, `fastmnmf_update_scm`,
`fastmnmf_update_diagonalizer_model`, `fastmnmf_normalize_power`, `fastmnmf_separate` with non-zero `ref` (M // 2 and
M - 1), and the free function `update_diagonalizer`.  Each starts from the same uploaded state.  The result is compared
with the matching function of tests/fastmnmf_np.py by the global metric (1e-9 in float64) and by the entry-wise metrics
of tests/envelope_np.py (W, H, g element by element; Q per (f) matrix; the output per (n, f) row).  float32 runs the same
grid against the float64 restatement evaluated on the float32-rounded state.

Which case covers what (name = m<M>_n<N>_k<K>_f<F>_t<T>; N * K in brackets):

    M = 2   m2_n1_k1_f3_t1 (N = 1, K = 1, F = 3, T = 1), m2_n6_k16_f1_t64 (N = 6, K = 16, F = 1, T = 64),
            m2_n8_k64_f15_t577 (N = 8, K = 64, [512], F = 15, T = 577)
    M = 3   m3_n8_k48_f70_t63 ([384], F = 70, T = 63), m3_n1_k17_f16_t130 (K = 17, [17], F = 16, T = 130)
    M = 4   m4_n4_k10_f17_t1000 (F = 17, T = 1000), m4_n7_k33_f15_t65 (N = 7, K = 33, T = 65),
            m4_n1_k64_f70_t64 (N = 1, K = 64)
    M = 5   m5_n6_k17_f19_t200, m5_n8_k64_f16_t130 ([512])
    M = 6   m6_n3_k16_f16_t65, m6_n1_k16_f33_t577 ([16], F = 33)
    M = 7   m7_n7_k33_f5_t67, m7_n2_k15_f17_t64 (K = 15)
    M = 8   m8_n8_k64_f33_t577 (the largest of everything), m8_n6_k1_f3_t63 (K = 1 with N > 1)

The diagonaliser update skips a channel when cond(Q V_m) >= threshold.  The host asserts that every cond(Q V_m) of a case
is three orders of magnitude away from the threshold, so no case tests a branch decided by rounding.  One case sits on
the far side: m2_n1_k1_f3_t1 has T < M, V_m has rank one, the restatement's cond is 1e16 or more and Q stays as it was.
In float32 a rank-deficient V_m cannot be told from a well-conditioned one at a threshold of 1e12 (the computed cond is
about 1 / 2^-23), so that case's two diagonaliser checks run in float64 only; its other outputs run in both.

Tolerances: 256 x d, d = the restatement's own sensitivity to ONE rounding (2^-52, or 2^-23 for float32) of its
inputs, measured over this grid by tools/mnmf_tolerance_probe.py.  Measured d -> tolerance:

    float64  loss 1.4e-15 -> 3.6e-13   W 1.6e-15 -> 4.1e-13   H 1.4e-15 -> 3.6e-13   g 4.0e-15 -> 1.0e-12
             Q 6.3e-16 -> 1.6e-13      separate 1.7e-15 -> 4.4e-13
    float32  loss 4.2e-7 -> 1.1e-4     W 5.8e-7 -> 1.5e-4     H 5.8e-7 -> 1.5e-4     g 3.1e-7 -> 7.9e-5
             Q 1.8e-7 -> 5.4e-5 (the floor, 1e-13 x 2^29)     separate 5.1e-7 -> 1.3e-4
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import envelope_np as env  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(env.FASTMNMF_GRID)
DTYPES = ["float64", "float32"]
NAMES = ("W", "H", "g", "Q")
DIAG_CASES = [(c, d) for d in DTYPES for c in CASES if not (d == "float32" and env.diagonalizer_skips(c))]


def upload(case, dtype):
    """engine, dict of X, W, H, g, Q on the device with the batch axis, workspace, the host state and the references."""
    import torch
    from audio_source_separation_amd.ops import Engine
    eng = Engine(dtype=dtype, device="cuda:0")
    states, refs = env.fastmnmf_case(case, dtype)
    dev = {}
    for i, name in enumerate(("X",) + NAMES):
        a = torch.from_numpy(np.ascontiguousarray(np.stack([s[i] for s in states])))
        dev[name] = a.to(eng.prec.cplx if a.is_complex() else eng.prec.real).to(eng.dev).contiguous()
    M, N, K, F, T, seeds = env.FASTMNMF_GRID[case]
    ws = eng.fastmnmf_workspace(len(seeds), M, N, F, T, K)
    return eng, dev, ws, states, refs


def host(t):
    a = t.cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def check(case, dtype, output, got, refs):
    tol = env.fastmnmf_tolerance(output, dtype)
    kind = env.fastmnmf_kind(output)
    for b, ref in enumerate(refs):
        g = env.rel(got[b], ref[output])
        e = env.entrywise(kind, got[b], ref[output])
        print("%s[%d] %s %s: rel %.3e  entry-wise %.3e (< %.2e)" % (case, b, dtype, output, g, e, tol))
        assert g < (env.REL_TOL if dtype == "float64" else tol), (case, b, output, g)
        assert e < tol, (case, b, output, e, tol)


def unchanged(dev, states, skip=()):
    for i, name in enumerate(NAMES):
        if name not in skip:
            assert np.array_equal(host(dev[name]), np.stack([s[i + 1] for s in states])), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_project_loss(case, dtype):
    import torch
    eng, dev, ws, states, refs = upload(case, dtype)
    loss = eng.empty((len(states),), dtype=torch.float64)
    eng.fastmnmf_project(dev["X"], dev["Q"], dev["W"], dev["H"], dev["g"], ws, loss=loss)
    check(case, dtype, "loss", host(loss), refs)
    unchanged(dev, states)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_update_nmf(case, dtype):
    eng, dev, ws, states, refs = upload(case, dtype)
    eng.fastmnmf_project(dev["X"], dev["Q"], dev["W"], dev["H"], dev["g"], ws)
    eng.fastmnmf_update_nmf(dev["X"], dev["W"], dev["H"], dev["g"], ws)
    check(case, dtype, "nmf_W", host(dev["W"]), refs)
    check(case, dtype, "nmf_H", host(dev["H"]), refs)
    unchanged(dev, states, ("W", "H"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_update_scm(case, dtype):
    eng, dev, ws, states, refs = upload(case, dtype)
    eng.fastmnmf_project(dev["X"], dev["Q"], dev["W"], dev["H"], dev["g"], ws)
    eng.fastmnmf_update_scm(dev["X"], dev["W"], dev["H"], dev["g"], ws)
    check(case, dtype, "scm_g", host(dev["g"]), refs)
    unchanged(dev, states, ("g",))


@pytest.mark.parametrize("case,dtype", DIAG_CASES)
def test_update_diagonalizer_model(case, dtype):
    eng, dev, ws, states, refs = upload(case, dtype)
    status = eng.new_status(len(states))
    eng.fastmnmf_update_diagonalizer_model(dev["X"], dev["Q"], dev["W"], dev["H"], dev["g"], ws, status=status)
    # no singular system anywhere; the condition guard reports a rejection exactly where the restatement skips
    from audio_source_separation_amd import _lib
    assert int(status.max()) == (_lib.STATUS_COND_REJECT if env.diagonalizer_skips(case) else 0)
    check(case, dtype, "diagonalizer_Q", host(dev["Q"]), refs)
    unchanged(dev, states, ("Q",))


@pytest.mark.parametrize("case,dtype", DIAG_CASES)
def test_update_diagonalizer_free_function(case, dtype):
    from audio_source_separation_amd.bss.mnmf import update_diagonalizer
    states, refs = env.fastmnmf_case(case, dtype)
    for b, (X, W, H, g, Q) in enumerate(states):
        Q0 = Q.copy()
        got = update_diagonalizer(X, Q, g, basis=W, activation=H, dtype=dtype, device="cuda:0")
        assert np.array_equal(Q, Q0)  # the caller's array is not written into
        check(case, dtype, "diagonalizer_Q", [np.asarray(got).astype(np.complex128)], [refs[b]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_normalize_power(case, dtype):
    eng, dev, ws, states, refs = upload(case, dtype)
    eng.fastmnmf_normalize_power(dev["X"], dev["Q"], dev["W"], dev["H"], dev["g"])
    for name in NAMES:
        check(case, dtype, "normalize_" + name, host(dev[name]), refs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_separate_nonzero_reference(case, dtype):
    eng, dev, ws, states, refs = upload(case, dtype)
    M = env.FASTMNMF_GRID[case][0]
    ids = env.reference_ids(M)[1:]
    assert ids and ids[-1] == M - 1 and 0 not in ids
    for r in ids:
        status = eng.new_status(len(states))
        Y = eng.fastmnmf_separate(dev["X"], dev["Q"], dev["W"], dev["H"], dev["g"], ref=r, status=status)
        assert int(status.max()) == 0
        check(case, dtype, "separate_%d" % r, host(Y), refs)
    unchanged(dev, states)
