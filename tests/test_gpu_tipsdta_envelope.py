"""tIPSDTA's kernels (csrc/assx_ipsdta.hip, the Student-t instantiations) entry by entry from general states, one entry
point at a time.

The grid, the general states and the method are those of tests/test_gpu_ipsdta_envelope.py (see there which case covers
which path); every case has its own nu from {0.5, 4, 1000} (ipsdta_envelope_np.GRID).  ONE entry point of `Engine` is
called on the uploaded state: `tipsdta_update_basis`, `tipsdta_update_activation`, `tipsdta_update_spatial` with n_sweeps
1 and 2, `tipsdta_loss`, and the result is compared with the LAPACK restatement (tests/tipsdta_np.py) by the family's
pooled metric at the family's one-stage tolerance AND entry-wise (U per (source, basis, block), W per (bin, row), H per
entry).  The normalisation has no Student-t entry point: both models call `ipsdta_normalize`, which the Gauss file tests.
What the Student-t model adds to the paths of the Gauss file:

    m7_f15_t63_k8_b3, m6_f11_t64_k7_b2   ip_tstep_kernel<7>, ip_tstep_kernel<6>
    m8_f16_t65_k9_b2, m8_f8_t130_k17_b1  ip_tstep_kernel<8> and ip_tq_kernel with blocks of 8: 8 steps per source and group
    m6_f11_t64_k7_b2, m4_f13_t257_k64_b2 the low group stepped before the high one with blocks of 5..7
    m3_f9_t577_k3_b4                     three trips of the frame loops of ip_tstep_kernel, ip_pi_kernel over 577 frames
    m2_f300_t8_k1_b300                   a step grid of 300 blocks; pi summed over 300 blocks
    m3_f515_t9_k2_b257                   step grids of 256 blocks and of one; ip_logdet_w's third trip in ip_tloss_kernel

Tolerances: 256 x d, floor 1e-13, d measured on the CPU over this grid by `tools/ipsdta_tolerance_probe.py --envelope`:

    basis 5.3e-14 -> 1.4e-11    activation 1.5e-15 -> 3.9e-13    spatial 4.6e-12 -> 1.2e-9    loss 4.5e-16 -> 1.2e-13

The exception: m5_f5_t1_k1_b1 (T < M and T below the block size) is left out of the spatial tests and its basis
comparison is held to 256 x its own d of 2.3e-8 = 5.9e-6, which is weak and says so; its activation and loss use the
common tolerances.

On an MI355X the kernels differ from the restatement entry-wise by at most 3.8e-14 (basis, m3_f515_t9_k2_b257), 1.4e-15
(activation), 5.8e-12 (spatial, m3_f515_t9_k2_b257) and 1.8e-16 (loss); the single-frame basis by 1.0e-8.  The pooled
figures: basis 2.2e-14, spatial 1.9e-12, the rest as entry-wise.  No kernel had to change.  The file's 39 tests take
4.1 s there, 1.6 s of it the first Engine; the slowest call is 0.45 s (most of it the host reference of the case).
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

MODEL = "t"
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
