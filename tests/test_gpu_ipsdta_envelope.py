"""GaussIPSDTA's kernels (csrc/assx_ipsdta.hip) entry by entry from general states, one entry point at a time.

For every case of `ipsdta_envelope_np.GRID` ONE general state is built on the host from a seeded generator (X a convolutive
mixture; W_f a random unitary with rows scaled by [0.5, 1.5], so y != x, the LU of the loss has to swap rows and a mix-up
of W's rows and columns shows; U = G G^H / nb + 0.1 I per (source, basis, block), dense complex Hermitian and different
in every block; H uniform in [0.1, 1.1]; normalised), uploaded, and ONE entry point of `Engine` is called on it:
`ipsdta_update_basis`, `ipsdta_update_activation`, `ipsdta_normalize` (on the state before its normalisation, where the
traces are not one), `ipsdta_update_spatial` with n_sweeps 1 and 2, `ipsdta_loss`.  Each starts from the same uploaded
state, never from another's output, so a failure names its kernel.  The result is compared with the LAPACK restatement
(tests/ipsdta_np.py) by the family's pooled metric at the family's one-stage tolerance AND by an entry-wise metric
(docstring of tests/ipsdta_envelope_np.py): U per (source, basis, block), W per (bin, row), H per entry.  Each test also
asserts status 0, that the arrays the call does not own are bit for bit unchanged, and that an updated basis is exactly
Hermitian in every block.  The host asserts the conditions listed in tests/ipsdta_envelope_np.py when it builds a case.

Which case covers what (name = m<M>_f<F>_t<T>_k<K>_b<n_blocks>; KC = 8 is the contraction kernel's chunk of bases):

    m8_f16_t65_k9_b2    two blocks of 8 with M = 8: ip_model_kernel<8>, ip_basis_kernel<8> and a full Wl in ip_sweep_kernel,
                        the largest register, scratch and LDS footprint; K = KC + 1; T = 65
    m7_f15_t63_k8_b3    M = 7 (ip_topsd_kernel<7>), blocks of 5, no remainder group; K = KC; T = 63
    m6_f11_t64_k7_b2    M = 6 (ip_topsd_kernel<6>), one block of 5 and one of 6, both groups; K = KC - 1; T = 64
    m8_f8_t130_k17_b1   a single block of 8; K = 17: two full chunks and one of one; T = 130
    m4_f13_t257_k64_b2  blocks of 6 and 7; K = 64; T = 257: a second trip of the frame loops with one frame
    m5_f12_t40_k16_b3   M = 5, blocks of 4; K = 16: two exact chunks; T < 64
    m3_f9_t577_k3_b4    blocks of 2 and 3; T = 577: three trips of the 256-thread frame loops with a ragged last one
    m2_f300_t8_k1_b300  300 blocks of one bin: ip_logdet_w and ip_norm_kernel take a second trip; T below one wave
    m3_f515_t9_k2_b257  256 blocks of 2 and one of 3: a third trip over the bins, a second over the blocks, a high group of one
    m5_f5_t1_k1_b1      a single frame (the exception below); no spatial comparison

Tolerances: 256 x d, floor 1e-13, d measured on the CPU over this grid by `tools/ipsdta_tolerance_probe.py --envelope`
(restatement on LAPACK against the restatement on the kernels' algorithms, and against itself one ulp away):

    basis 5.4e-14 -> 1.4e-11    activation 1.7e-15 -> 4.4e-13    spatial 9.1e-12 -> 2.4e-9    loss 1.1e-15 -> 2.9e-13
    normalize_U 6.8e-16, normalize_H 8.1e-16 -> the floor, 1e-13

The exception: m5_f5_t1_k1_b1 has T < M, where Q has rank T and is inverted through its eps shift alone, so it is left out
of the spatial tests; and T below the block size, where S_k has rank T and the square root turns a rounding into its
root: its basis comparison is held to 256 x its own d of 2.0e-8 = 5.1e-6, which is weak and says so.  Its activation,
normalisation and loss use the common tolerances.

On an MI355X the kernels differ from the restatement entry-wise by at most 3.5e-14 (basis, m3_f515_t9_k2_b257), 1.4e-15
(activation), 7.6e-16 (normalize_U), 7.5e-16 (normalize_H), 5.0e-12 (spatial, m3_f515_t9_k2_b257) and 2.7e-16 (loss);
the single-frame basis by 8.7e-9.  The pooled figures: basis 1.8e-14, spatial 3.8e-12 (m7_f15_t63_k8_b3, against the
family's 1.2e-11), the rest as entry-wise.  No kernel had to change.  The file's 49 tests take 4.3 s there, 1.8 s of it
the first Engine; the slowest call is 0.45 s (most of it the host reference of the case, computed once and cached).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ipsdta_envelope_np as ev  # noqa: E402
import ipsdta_np as ip  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL = "gauss"
CASES = list(ev.GRID)


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(dtype="float64")


@pytest.mark.parametrize("case", CASES)
def test_update_basis(eng, case):
    d = ev.Device(eng, case, MODEL)
    d.call("update_basis")
    got = d.fetch()
    U = d.basis(got)
    ev.check(case, MODEL, "basis", U)
    for p in ip.to_parts(U):
        assert np.array_equal(p, ip.ct(p))  # exactly Hermitian in every block
    d.unchanged(got, "U")


@pytest.mark.parametrize("case", CASES)
def test_update_activation(eng, case):
    d = ev.Device(eng, case, MODEL)
    d.call("update_activation")
    got = d.fetch()
    ev.check(case, MODEL, "activation", got["H"])
    d.unchanged(got, "H")


@pytest.mark.parametrize("case", CASES)
def test_normalize(eng, case):
    d = ev.Device(eng, case, MODEL, raw=True)
    eng.ipsdta_normalize(d.U, d.H, d.F, d.nblk)
    got = d.fetch()
    ev.check(case, MODEL, "normalize_U", d.basis(got))
    ev.check(case, MODEL, "normalize_H", got["H"])
    d.unchanged(got, "UH")


@pytest.mark.parametrize("case", ev.SPATIAL_CASES)
def test_update_spatial(eng, case):
    for n_sweeps in (1, 2):  # each from a fresh upload of the same state
        d = ev.Device(eng, case, MODEL)
        d.call("update_spatial", n_sweeps=n_sweeps)
        got = d.fetch()
        ev.check(case, MODEL, "spatial_%d" % n_sweeps, got["W"])
        d.unchanged(got, "W")


@pytest.mark.parametrize("case", CASES)
def test_loss(eng, case):
    d = ev.Device(eng, case, MODEL)
    loss = d.call("loss")
    got = d.fetch()
    assert loss.shape == (1,)
    ev.check(case, MODEL, "loss", np.float64(loss.item()))
    d.unchanged(got, "")
