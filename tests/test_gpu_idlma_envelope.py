"""Every entry point of csrc/assx_idlma.hip against the NumPy restatement (tests/idlma_np.py) over the size envelope: every
M in 2..8, F in {1, 3, 17}, domain in {1, 1.5, 2}, and the frame counts of tests/beamform_envelope_np.py -- around the wave,
the workgroup and the frame chunk -- plus T = M and the seams of these kernels' own partition: a partial and a whole
16-byte store (66, 68) and one thread past a chunk (chunk + 4).  Entry-wise metrics.

Tolerances, per problem, by the recipe of tools/idlma_tolerance_probe.py with the restatement standing in for the reference:
FACTOR x the largest of (the kernel model against the restatement, the restatement's own move when everything it reads
moves to a neighbouring double: the largest of N_DRAWS draws), at least FACTOR x 2^-52; a float32 map at least
FACTOR x 2^-24, out of powf FACTOR x 2^-22.  The scale is assx_projection_back_scale's, which is not new here: it is held
through the normalised W.
What is exact by construction is compared bit for bit: dnn_output and R for domains 1 and 2, the fused calls against the
single ones."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import idlma_np as idl  # noqa: E402
import beamform_envelope_np as benv  # noqa: E402
from test_gpu_idlma import dev, host, one_step, same, single_calls  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 16
RES = 2.0 ** -52
N_DRAWS = 3
CHANNELS = tuple(range(2, 9))
BINS = (1, 3, 17)
DOMAINS = (1, 1.5, 2)


def frames(M):
    return tuple(sorted(set(benv.FRAMES) | set(idl.ENVELOPE_EXTRA_FRAMES) | {M}))


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


def problem(M, F, T, domain):
    rng = np.random.default_rng(M * 100003 + F * 1009 + T * 7 + int(domain * 2))
    X = rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))
    W0 = np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1)) + 0.2 * (rng.standard_normal((F, M, M))
                                                                    + 1j * rng.standard_normal((F, M, M)))
    raw = (0.2 + rng.random((M, F, T))).astype(np.float32)
    raw[rng.random((M, F, T)) < 0.02] = 0.0  # both floors are met; too few entries to starve a bin
    return X, W0, raw


def test_grid_follows_the_library_constant():
    from audio_source_separation_amd import _lib
    assert idl.FRAME_CHUNK == _lib.IDLMA_FRAME_CHUNK == benv.FRAME_CHUNK
    for M in CHANNELS:
        assert {M, 63, 64, 65, 66, 68, 255, 256, 257} <= set(frames(M))
        assert {_lib.IDLMA_FRAME_CHUNK + k for k in (-1, 0, 1, 4)} <= set(frames(M))


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("F", BINS)
@pytest.mark.parametrize("M", CHANNELS)
def test_entry_points(eng, M, F, domain):
    p = dict(domain=float(domain), dnn_flooring=1e-5, eps=1e-12, reference_id=M - 1)
    f32 = 2.0 ** -24
    for T in frames(M):
        X, W0, raw = problem(M, F, T, domain)
        moved = []
        for draw in range(N_DRAWS):
            rng = np.random.default_rng(10 * T + draw)
            moved.append((idl.one_ulp(X, rng), idl.one_ulp(W0, rng), rng))
        # ---- the network's input, alone
        inp = host(eng.idlma_dnn_input(dev(eng, X), dev(eng, W0), domain=p["domain"]))
        want = idl.network_input(X, W0, p["domain"])
        tol = FACTOR * max([f32] + [idl.d_metric(idl.network_input(Xm, Wm, p["domain"]), want) for Xm, Wm, _ in moved])
        assert inp.dtype == np.float32 and idl.d_metric(inp, want) <= tol, (T, idl.d_metric(inp, want), tol)
        # ---- the float32 arithmetic on the network's output, both floors met
        d_dev, R_dev = eng.empty((M, F, T), dtype=torch.float32), eng.empty((M, F, T), dtype=torch.float64)
        eng.idlma_variance(dev(eng, raw), d_dev, R_dev, domain=p["domain"], dnn_flooring=p["dnn_flooring"], eps=p["eps"])
        d = idl.source_output(raw, p["domain"], p["dnn_flooring"])
        R = idl.variance(d, p["domain"], p["eps"])
        if domain == 1.5:
            assert idl.d_metric(host(d_dev), d) <= FACTOR * 2.0 ** -22
            assert idl.d_metric(host(R_dev), idl.variance(host(d_dev), p["domain"], p["eps"])) <= FACTOR * 2.0 ** -22
        else:
            assert same(host(d_dev), d) and same(host(R_dev), R.astype(np.float64))
        # ---- one iteration after the network, single calls against the restatement in the kernels' form.  The source
        # model is kept off its floors here: a variance of 1e-10 next to ones makes W U_n of a bin with few frames
        # ill-conditioned, and a tolerance measured as a sensitivity says nothing there
        raw = np.maximum(raw, np.float32(0.2))
        got = single_calls(eng, X, W0, raw, p)
        d = idl.source_output(raw, p["domain"], p["dnn_flooring"])
        if domain == 1.5:
            assert idl.d_metric(got["d"], d) <= FACTOR * 2.0 ** -22
            d, R = got["d"], got["R"].astype(np.float32)  # what follows is held to the restatement on the same source model
        else:
            R = idl.variance(d, p["domain"], p["eps"])
            assert same(got["d"], d) and same(got["R"], R.astype(np.float64))

        def restated(X, W0):
            W_ip = idl.space_update(X, W0, R)
            W1 = idl.normalize_scaled(W_ip, idl.pb_scale(idl.separate(X, W_ip), X[p["reference_id"]]))
            return W_ip, W1

        W_ip, W1 = restated(X, W0)
        again = [restated(Xm, Wm) for Xm, Wm, _ in moved]
        tol_ip = FACTOR * max([RES] + [idl.w_metric(a[0], W_ip) for a in again])
        tol_W = FACTOR * max([tol_ip / FACTOR] + [idl.w_metric(a[1], W1) for a in again])
        assert idl.w_metric(got["W_ip"], W_ip) <= tol_ip, (T, idl.w_metric(got["W_ip"], W_ip), tol_ip)
        assert idl.w_metric(got["W"], W1) <= tol_W, (T, idl.w_metric(got["W"], W1), tol_W)
        # the normalisation, the loss and the next input as functions of what the GPU itself handed them
        scaled = idl.normalize_scaled(got["W_ip"], got["scale"])
        assert np.max(np.abs(got["W"] - scaled) / np.abs(scaled)) <= FACTOR * RES
        k_loss = idl.kernel_loss(X, got["W"], d, p["domain"], p["eps"], R=R)
        r_loss = idl.loss(X, got["W"], d, p["domain"], p["eps"], R=R)
        tol_loss = FACTOR * max([RES, idl.loss_metric(k_loss, r_loss, X)] + [idl.loss_metric(
            idl.loss(Xm, idl.one_ulp(got["W"], rng), d, p["domain"], p["eps"], R=R), r_loss, X) for Xm, _, rng in moved])
        assert idl.loss_metric(got["loss"][0], r_loss, X) <= tol_loss, (T, got["loss"][0], r_loss, tol_loss)
        assert idl.loss_metric(got["loss"][0], k_loss, X) <= tol_loss, (T, got["loss"][0], k_loss, tol_loss)
        want = idl.network_input(X, got["W"], p["domain"])
        tol = FACTOR * max([f32] + [idl.d_metric(idl.network_input(Xm, idl.one_ulp(got["W"], rng), p["domain"]), want)
                                    for Xm, _, rng in moved])
        assert idl.d_metric(got["inp"], want) <= tol, (T, idl.d_metric(got["inp"], want), tol)
        # ---- the same in one call, bit for bit
        fused = one_step(eng, X, W0, raw, p)
        assert same(fused["W"], got["W"]) and same(fused["d"], got["d"]), T
        assert same(fused["loss"], got["loss"]) and same(fused["inp"], got["inp"]), T
