"""AuxIVA's kernels (Laplace and Gauss) over their size envelope, one entry point at a time, in float64 and float32.

The counterpart of tests/test_gpu_ilrma_envelope.py for `ilrma_envelope_np.AUXIVA_GRID`: assx_auxiva_weights with the
loss, and assx_auxiva_spatial_update with the IP, ISS and IP2 sweeps (pairs (0, 1) and (M - 1, 0)), each on the seeded
entry state, against oracle/oracle_np.py in float64 by the entry-wise metrics, at 256 x the d that
tools/ilrma_tolerance_probe.py measured on the oracle alone (D_AUXIVA).  The spatial updates take the weights of the
state (the oracle's `auxiva_weights`, rounded with the state for float32), so every entry point starts from the same
input as its reference.  The scratch is filled with 0xFF bytes before every call; the weights and the IP update run a
second time on `AUXIVA_STREAM_CASES` with ASSX_G = 3.  Status words as in the ILRMA file: 0, or ASSX_STATUS_COND_REJECT
in every utterance of the T < M cases.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ilrma_envelope_np as env  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(env.AUXIVA_GRID)
DTYPES = ["float64", "float32"]
_ENGINES = {}


def engine(dtype):
    from audio_source_separation_amd.ops import Engine
    if dtype not in _ENGINES:
        _ENGINES[dtype] = Engine(dtype=dtype, device="cuda:0")
    return _ENGINES[dtype]


def to_dev(eng, a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(eng.prec.cplx if t.is_complex() else eng.prec.real).to(eng.dev).contiguous()


def host(t):
    a = t.cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


class Case:
    def __init__(self, case, dtype):
        self.case, self.dtype = case, dtype
        self.M, self.F, self.T, seeds = env.AUXIVA_GRID[case]
        self.B = len(seeds)
        self.eng = engine(dtype)
        self.states, self.refs = env.auxiva_case(case, dtype)
        self.rejected = self.T < self.M
        self.ambiguous = self.rejected and dtype == "float32"

    def __getitem__(self, field):
        i = env.AUXIVA_FIELDS.index(field)
        return to_dev(self.eng, np.stack([s[i] for s in self.states]))

    def poison(self):
        self.eng._scratch(self.B, self.M, self.F, self.T, 1)
        self.eng._ws.buf.fill_(0xFF)

    def check(self, output, got):
        tol = env.auxiva_tolerance(output, self.dtype)
        got = host(got)
        assert got.shape[0] == self.B
        for b, ref in enumerate(self.refs):
            e = env.entrywise(env.auxiva_kind(output), got[b], ref[output])
            print("%s[%d] %s %s: entry-wise %.3e (< %.2e)" % (self.case, b, self.dtype, output, e, tol))
            assert e < tol, (self.case, b, output, e, tol)


def expect_status(c, status):
    from audio_source_separation_amd import _lib
    st = status.cpu().numpy()
    if c.rejected:
        # every utterance reports the rejection.  ASSX_STATUS_SINGULAR may come with it: whether the elimination of a
        # rank-deficient W U meets an exact zero pivot is a rounding accident (numpy.linalg.solve itself raises
        # "Singular matrix" on the m3_f70_t2 states and not on the m2_f3_t1 ones)
        assert np.all(st & _lib.STATUS_COND_REJECT), st
    else:
        assert not st.any(), st


def code_of(kind):
    from audio_source_separation_amd import _lib
    return _lib.IVA_LAPLACE if kind == "laplace" else _lib.IVA_GAUSS


params = pytest.mark.parametrize("case,dtype", [(c, d) for d in DTYPES for c in CASES])
kinds = pytest.mark.parametrize("kind", env.KINDS)


def _weights_and_loss(c, kind):
    X, W = c["X"], c["W"]
    c.poison()
    r, loss = c.eng.auxiva_weights(X, W, code_of(kind), with_loss=True)
    c.check("weights_" + kind, r)
    c.check("loss_" + kind, loss)
    assert np.array_equal(host(W), host(c["W"]))


def _spatial_ip(c, kind):
    W = c["W"]
    status = c.eng.new_status(c.B)
    c.poison()
    c.eng.auxiva_spatial_update(c["X"], W, c["r_" + kind], status=status)
    if c.ambiguous:
        return
    expect_status(c, status)
    c.check("spatial_ip_W_" + kind, W)
    if c.rejected:
        assert np.array_equal(host(W), host(c["W"]))


@kinds
@params
def test_weights_and_loss(case, dtype, kind):
    _weights_and_loss(Case(case, dtype), kind)


@kinds
@params
def test_spatial_update_ip(case, dtype, kind):
    _spatial_ip(Case(case, dtype), kind)


@kinds
@params
def test_spatial_update_iss(case, dtype, kind):
    from audio_source_separation_amd import _lib
    c = Case(case, dtype)
    if c.rejected:  # 0 / 0 in the reference itself (tests/ilrma_envelope_np.py)
        assert "spatial_iss_W_" + kind not in c.refs[0]
        return
    W = c["W"]
    c.poison()
    c.eng.auxiva_spatial_update(c["X"], W, c["r_" + kind], spatial=_lib.SPATIAL_ISS)
    c.check("spatial_iss_W_" + kind, W)


@kinds
@params
def test_spatial_update_ip2(case, dtype, kind):
    from audio_source_separation_amd import _lib
    c = Case(case, dtype)
    for i, pair in enumerate(env.ip2_pairs(c.M)):
        W = c["W"]
        status = c.eng.new_status(c.B)
        c.poison()
        c.eng.auxiva_spatial_update(c["X"], W, c["r_" + kind], status=status, spatial=_lib.SPATIAL_IP2, pair=pair)
        if c.ambiguous:
            continue
        expect_status(c, status)
        c.check("spatial_ip2_W_%d_%s" % (i, kind), W)
        others = [n for n in range(c.M) if n not in pair]
        assert np.array_equal(host(W)[:, :, others], host(c["W"])[:, :, others])


@pytest.fixture
def few_workgroups():
    """Force the flat partitions down to a handful of workgroups (ASSX_G): ranges that start and end inside a bin and
    cross utterances.  The variable is removed afterwards."""
    def _set(g):
        os.environ["ASSX_G"] = str(g)
    yield _set
    os.environ.pop("ASSX_G", None)


@kinds
@pytest.mark.parametrize("step", [_weights_and_loss, _spatial_ip], ids=["weights", "spatial_ip"])
@pytest.mark.parametrize("case,dtype", [(c, d) for d in DTYPES for c in env.AUXIVA_STREAM_CASES])
def test_streaming_entry_points_on_three_workgroups(few_workgroups, case, dtype, step, kind):
    few_workgroups(3)
    step(Case(case, dtype), kind)
