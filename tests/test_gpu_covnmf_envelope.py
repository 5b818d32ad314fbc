"""The covariance-domain MultichannelISNMF kernels over their whole size envelope, one entry point at a time.

For every case of `covnmf_envelope_np.GRID` ONE general state is built on the host from a seeded generator (target = the
mean of M consecutive outer products of complex Gaussian frames plus 0.1 x its mean diagonal x I; basis, activation
uniform in [0.05, 1.05]; spatial = G G^H + 0.1 I over its trace, different per (f, k), so every off-diagonal has a real
and an imaginary part), uploaded, and ONE entry point of `Engine` is called on it: `covnmf_update_basis`,
`covnmf_update_activation`, `covnmf_update_spatial` (normalize on and off), `covnmf_reconstruct`, `covnmf_loss`.  Each
starts from the same uploaded state, never from another's output, so a failure names its kernel.  The result is compared
with the matching function of tests/covnmf_np.py by the global metric at the project's 1e-9 AND by an entry-wise metric
(docstring of tests/envelope_np.py) that a single wrong element cannot hide behind.  The host asserts that no
denominator of the restatement comes within six orders of magnitude of its eps clamp.

Which case covers what (name = m<M>_k<K>_f<F>_t<T>):

    M = 2   m2_k1_f3_t1 (K = 1, F = 3, T = 1), m2_k15_f1_t64 (K = 15, F = 1, T = 64), m2_k16_f33_t65 (K = 16, F = 33:
            three bins in some activation slices, T = 65), m2_k64_f17_t577 (K = 64: two 32-basis groups of the spatial
            sums, F = 17, T = 577: 10 tiles over 8 slices with a ragged last tile)
    M = 3   m3_k17_f3_t63 (K = 17: a second chunk of one basis), m3_k33_f17_t130 (K = 33: three chunks), m3_k1_f1_t577
    M = 4   m4_k16_f17_t64, m4_k33_f33_t130, m4_k64_f3_t65, m4_k15_f1_t1 (one point in all)
    M = 5   m5_k17_f17_t65, m5_k1_f33_t63, m5_k64_f1_t130
    M = 6   m6_k33_f3_t577, m6_k16_f17_t63, m6_k15_f33_t64
    M = 7   m7_k64_f3_t130, m7_k17_f1_t65, m7_k1_f17_t64
    M = 8   m8_k64_f17_t130 (M = 8 and K = 64 together: the largest LDS and register footprint, the evaluation kernel
            with scratch), m8_k33_f3_t63, m8_k16_f1_t577, m8_k15_f33_t65

    T  1, 63, 64, 65, 130, 577 all occur;  F  1, 3, 17, 33 all occur;  K  1, 15, 16, 17, 33, 64 all occur;  every M has a
    case with more than one wave of frames and one with a ragged last wave.

Tolerances: 256 x d, d = the restatement's own sensitivity to ONE rounding of its inputs, measured over this grid by
tools/covnmf_tolerance_probe.py (floor 1e-13).  Measured d and the tolerance that follows:

    basis 6.5e-15 -> 1.7e-12    activation 5.2e-15 -> 1.3e-12    spatial 1.3e-12 -> 3.3e-10
    reconstruct 1.1e-15 -> 2.8e-13    loss 3.6e-15 -> 9.2e-13

The K = 1 cases set these figures (m7_k1_f17_t64, m5_k1_f33_t63: with one basis P = (Tb V H)^-1 and every output carries
cond(H)); without them d is below 9e-14 for spatial and below 2.1e-15 for the rest.  On an MI355X the kernels differ from
the restatement by at most 1.7e-15 (basis), 3.6e-15 (activation), 1.0e-12 (spatial, m7_k1_f17_t64, the case that sets d),
6.0e-16 (reconstruct) and 3.3e-16 (loss); every test prints its figures.

The one exception: m2_k1_f3_t1 and m4_k15_f1_t1 have fewer frames than 2 M.  As in the MNMF sweep their `update_spatial`
is held to 256 x its own d and stays out of the grid's figure; with a full-rank target those d are small (1.8e-15 ->
4.6e-13 and 2.8e-14 -> 7.2e-12; the kernels: 6.8e-16 and 4.1e-14), so the exception asks for more there, not less.  Both
cases are in the grid for their other outputs and for the T < 64 paths.  No other output and no other case has a
tolerance of its own.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import envelope_np as env  # noqa: E402
import covnmf_envelope_np as cenv  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(cenv.GRID)
NAMES = ("X", "Tb", "V", "H")


def upload(case):
    """(engine, [X, Tb, V, H] on the device, workspace, status, state, reference)."""
    import torch
    from audio_source_separation_amd.ops import Engine
    eng = Engine(device="cuda:0")
    state, ref = cenv.grid_case(case)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev) for a in state]
    M, K, F, T, _ = cenv.GRID[case]
    return eng, dev, eng.covnmf_workspace(M, F, T, K), eng.new_status(1), state, ref


def check(case, output, got, ref):
    kind = cenv.kind(output)
    tol = cenv.tolerance(case, output)
    got = np.asarray(got)
    g = env.rel(got, ref[output])
    e = cenv.entrywise(kind, got, ref[output])
    print("%s %s: rel %.3e (< %.0e)  entry-wise %.3e (< %.2e)" % (case, output, g, env.REL_TOL, e, tol))
    assert g < env.REL_TOL, (case, output, g)
    assert e < tol, (case, output, e, tol)


def unchanged(dev, state, skip):
    """An entry point writes its own array only."""
    for i, name in enumerate(NAMES):
        if name != skip:
            assert np.array_equal(dev[i].cpu().numpy(), state[i]), name


def test_grid_covers_the_envelope():
    Ms, Ks, Fs, Ts = (set(v[i] for v in cenv.GRID.values()) for i in range(4))
    assert Ms == set(range(2, 9)) and Ks == {1, 15, 16, 17, 33, 64} and Fs == {1, 3, 17, 33}
    assert Ts == {1, 63, 64, 65, 130, 577}
    assert any(v[0] == 8 and v[1] == 64 for v in cenv.GRID.values())
    assert set(cenv.D_SPATIAL_FEW_FRAMES) == {c for c in cenv.GRID if cenv.few_frames(c)}


@pytest.mark.parametrize("case", CASES)
def test_update_basis(case):
    eng, dev, ws, status, state, ref = upload(case)
    eng.covnmf_update_basis(*dev, ws, status=status)
    assert int(status.max()) == 0
    check(case, "basis", dev[1].cpu().numpy(), ref)
    unchanged(dev, state, "Tb")


@pytest.mark.parametrize("case", CASES)
def test_update_activation(case):
    eng, dev, ws, status, state, ref = upload(case)
    eng.covnmf_update_activation(*dev, ws, status=status)
    assert int(status.max()) == 0
    check(case, "activation", dev[2].cpu().numpy(), ref)
    unchanged(dev, state, "V")


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "plain"])
@pytest.mark.parametrize("case", CASES)
def test_update_spatial(case, normalize):
    eng, dev, ws, status, state, ref = upload(case)
    eng.covnmf_update_spatial(*dev, ws, normalize=normalize, status=status)
    assert int(status.max()) == 0
    H = dev[3].cpu().numpy()
    check(case, "spatial_normalized" if normalize else "spatial_plain", H, ref)
    assert np.array_equal(H, H.conj().swapaxes(-1, -2))  # exactly Hermitian
    unchanged(dev, state, "H")


@pytest.mark.parametrize("case", CASES)
def test_reconstruct(case):
    eng, dev, ws, status, state, ref = upload(case)
    Xh = eng.covnmf_reconstruct(*dev[1:])
    check(case, "reconstruct", Xh.cpu().numpy(), ref)
    unchanged(dev, state, None)


@pytest.mark.parametrize("case", CASES)
def test_loss(case):
    eng, dev, ws, status, state, ref = upload(case)
    loss = eng.covnmf_loss(*dev, ws, status=status)
    assert int(status.max()) == 0
    check(case, "loss", loss.cpu().numpy()[0], ref)
    unchanged(dev, state, None)
