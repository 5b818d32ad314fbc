"""Gauss-ILRMA's kernels over their size envelope, one entry point at a time, in float64 and float32.

For every case of `ilrma_envelope_np.ILRMA_GRID` the seeded state(s) of the case are uploaded (several states = one
batched call) and ONE entry point of `ops.Engine` is called on them; the result is compared with the matching output
of `ilrma_envelope_np.ilrma_reference` (oracle/oracle_np.py in float64, on the float32-rounded state for float32) by
the entry-wise metric of its kind, every utterance against its own reference.  The tolerance is 256 x d of the kind,
d measured on the reference alone by tools/ilrma_tolerance_probe.py (tests/ilrma_envelope_np.py: D_ILRMA).  What the
grid covers is asserted by tests/test_ilrma_envelope_cpu.py::test_grids_cover_the_dispatch_boundaries.

Entry points: assx_demix, assx_ilrma_power_map, assx_cov_accumulate (three weight kinds), assx_ilrma_source_update with
`loss_prev`, assx_ilrma_loss, assx_ilrma_spatial_update (IP with and without `U_out`, with C / power_bins; ISS; IP2 for
the pairs (0, 1) and (M - 1, 0)), assx_ilrma_cov_partials (return code: its records are read through `U_out`),
assx_demix_power, assx_power_from_cov, assx_ilrma_normalize_power_bins, assx_ilrma_normalize_pb,
assx_projection_back_scale, assx_nmf_half_sums, assx_nmf_apply_sums, assx_ordered_sum.  The scratch is filled with 0xFF
bytes (NaN in both precisions) before every call that goes through partial records.  The streaming entry points run a
second time on `ILRMA_STREAM_CASES` with ASSX_G = 3, so that a workgroup's range starts and ends inside a bin and
crosses utterances.

Status words: 0 where the reference accepts every row, ASSX_STATUS_COND_REJECT in every utterance of the T < M cases
(float64; for float32 see the docstring of tests/ilrma_envelope_np.py).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ilrma_envelope_np as env  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(env.ILRMA_GRID)
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
    """A grid case on the device: `dev[field]` is the field of every state stacked along a leading utterance axis."""

    def __init__(self, case, dtype):
        self.case, self.dtype = case, dtype
        self.M, self.K, self.domain, self.F, self.T, seeds = env.ILRMA_GRID[case]
        self.B = len(seeds)
        self.eng = engine(dtype)
        self.states, self.refs = env.ilrma_case(case, dtype)
        self.rejected = self.T < self.M
        self.ambiguous = self.rejected and dtype == "float32"  # rank-deficient W U at a threshold of 1e12 in float32
        self._dev = {}

    def __getitem__(self, field):
        if field not in self._dev:
            i = env.ILRMA_FIELDS.index(field)
            self._dev[field] = to_dev(self.eng, np.stack([s[i] for s in self.states]))
        return self._dev[field].clone()

    def ref(self, output):
        return to_dev(self.eng, np.stack([r[output] for r in self.refs]))

    def ref64(self, output):
        import torch
        return torch.from_numpy(np.ascontiguousarray(np.stack([r[output] for r in self.refs]))).to(self.eng.dev)

    def poison(self):
        """0xFF bytes over the whole scratch: a partial record that is read without having been written is NaN."""
        self.eng._scratch(self.B, self.M, self.F, self.T, self.K)
        self.eng._ws.buf.fill_(0xFF)

    def check(self, output, got):
        tol = env.ilrma_tolerance(output, self.dtype)
        kind = env.ilrma_kind(output)
        got = host(got) if hasattr(got, "cpu") else np.asarray(got)
        assert got.shape[0] == self.B
        for b, ref in enumerate(self.refs):
            e = env.entrywise(kind, got[b], ref[output])
            print("%s[%d] %s %s: entry-wise %.3e (< %.2e)" % (self.case, b, self.dtype, output, e, tol))
            assert e < tol, (self.case, b, output, e, tol)

    def unchanged(self, *fields_and_tensors):
        for field, t in fields_and_tensors:
            assert np.array_equal(host(t), host(self[field])), field


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


params = pytest.mark.parametrize("case,dtype", [(c, d) for d in DTYPES for c in CASES])


@params
def test_demix(case, dtype):
    c = Case(case, dtype)
    X, W = c["X"], c["W"]
    c.check("demix", c.eng.demix(X, W))
    c.check("demix_scaled", c.eng.demix(X, W, scale=c["scale"]))
    c.unchanged(("X", X), ("W", W))


@params
def test_power_map(case, dtype):
    c = Case(case, dtype)
    c.check("power_map", c.eng.ilrma_power_map(c["X"], c["W"]))


@params
def test_cov_accumulate(case, dtype):
    c = Case(case, dtype)
    X = c["X"]
    for output, r in (("cov_nt", c["r_nt"]), ("cov_nft", c["r_nft"]), ("cov_none", None)):
        c.poison()
        U = c.eng.cov_accumulate(X, r)
        c.check(output, U)
        assert np.array_equal(host(U), host(U).conj().swapaxes(-1, -2))  # Hermitian by construction


def _source_update(c):
    import torch
    X, W, Tb, V = c["X"], c["W"], c["Tb"], c["V"]
    lp = c.eng.empty((c.B,), dtype=torch.float64)
    c.poison()
    c.eng.ilrma_source_update(X, W, Tb, V, domain=c.domain, loss_prev=lp)
    c.check("source_Tb", Tb)
    c.check("source_V", V)
    c.check("source_loss_prev", lp)
    c.unchanged(("X", X), ("W", W))


def _loss(c):
    c.poison()
    c.check("loss", c.eng.ilrma_loss(c["X"], c["W"], c["Tb"], c["V"], domain=c.domain))


def _spatial_ip_dense(c):
    X, W, Tb, V = c["X"], c["W"], c["Tb"], c["V"]
    U = c.eng.empty((c.B, c.M, c.F, c.M, c.M), complex_=True)
    status = c.eng.new_status(c.B)
    c.poison()
    c.eng.ilrma_spatial_update(X, W, Tb, V, domain=c.domain, status=status, U_out=U)
    c.check("spatial_ip_U", U)
    if not c.ambiguous:
        expect_status(c, status)
        c.check("spatial_ip_W", W)
        if c.rejected:
            c.unchanged(("W", W))
    c.unchanged(("Tb", Tb), ("V", V))


def _cov_accumulate_nt(c):
    c.poison()
    c.check("cov_nt", c.eng.cov_accumulate(c["X"], c["r_nt"]))


@params
def test_source_update_with_loss_of_entry_state(case, dtype):
    _source_update(Case(case, dtype))


@params
def test_loss(case, dtype):
    _loss(Case(case, dtype))


@params
def test_spatial_update_ip_with_dense_covariance(case, dtype):
    _spatial_ip_dense(Case(case, dtype))


@params
def test_spatial_update_ip_with_power_bins(case, dtype):
    """Without `U_out` the IP sweep reduces the covariance records itself (another kernel path than the dense one); C
    and power_bins make it emit w C w^H of the updated filters."""
    import torch
    c = Case(case, dtype)
    W = c["W"]
    C = c.ref("cov_none")[:, 0].contiguous()
    pb = torch.full((c.B, c.M, c.F), float("nan"), dtype=torch.float64, device=c.eng.dev)
    status = c.eng.new_status(c.B)
    c.poison()
    c.eng.ilrma_spatial_update(c["X"], W, c["Tb"], c["V"], domain=c.domain, status=status, C=C, power_bins=pb)
    if not c.ambiguous:
        expect_status(c, status)
        c.check("spatial_ip_W", W)
        c.check("spatial_ip_power_bins", pb)
    else:
        assert bool(torch.isfinite(W.abs()).all()) and bool(torch.isfinite(pb).all())


@params
def test_spatial_update_iss(case, dtype):
    from audio_source_separation_amd import _lib
    c = Case(case, dtype)
    if c.rejected:  # 0 / 0 in the reference itself (tests/ilrma_envelope_np.py); nothing to compare with
        assert "spatial_iss_W" not in c.refs[0]
        return
    W = c["W"]
    c.poison()
    c.eng.ilrma_spatial_update(c["X"], W, c["Tb"], c["V"], domain=c.domain, spatial=_lib.SPATIAL_ISS)
    c.check("spatial_iss_W", W)


@params
def test_spatial_update_ip2(case, dtype):
    from audio_source_separation_amd import _lib
    c = Case(case, dtype)
    for i, pair in enumerate(env.ip2_pairs(c.M)):
        W = c["W"]
        status = c.eng.new_status(c.B)
        c.poison()
        c.eng.ilrma_spatial_update(c["X"], W, c["Tb"], c["V"], domain=c.domain, status=status, spatial=_lib.SPATIAL_IP2,
                                   pair=pair)
        if c.ambiguous:
            continue
        expect_status(c, status)
        c.check("spatial_ip2_W_%d" % i, W)
        others = [n for n in range(c.M) if n not in pair]
        assert np.array_equal(host(W)[:, :, others], host(c["W"])[:, :, others])  # the other rows: bit for bit


@params
def test_cov_partials_return_code(case, dtype):
    """assx_ilrma_cov_partials is the covariance stage alone, for kernel timing: 2 <= M <= 4 only (the wide-channel path
    has no such stage), where it must accept every case; its records are compared through `U_out` above."""
    from audio_source_separation_amd._lib import AssxError
    c = Case(case, dtype)
    c.poison()
    if c.M <= 4:
        c.eng.ilrma_cov_partials(c["X"], c["Tb"], c["V"], domain=c.domain)  # raises on a non-zero return code
    else:
        with pytest.raises(AssxError, match="2 <= M <= 4"):
            c.eng.ilrma_cov_partials(c["X"], c["Tb"], c["V"], domain=c.domain)
    import torch
    torch.cuda.synchronize()


@params
def test_power_statistics(case, dtype):
    c = Case(case, dtype)
    c.poison()
    c.check("demix_power", c.eng.demix_power(c["X"], c["W"]))
    c.poison()
    C = c.ref("cov_none")[:, 0].contiguous()
    c.check("power_from_cov", c.eng.power_from_cov(C, c["W"], c.T))


@params
def test_normalize_power_bins(case, dtype):
    c = Case(case, dtype)
    W, Tb = c["W"], c["Tb"]
    c.eng.ilrma_normalize_power_bins(W, Tb, c.ref64("_power_bins_in"), domain=c.domain)
    c.check("normalize_bins_W", W)
    c.check("normalize_bins_Tb", Tb)


@params
def test_projection_back_scale_and_normalize(case, dtype):
    c = Case(case, dtype)
    if c.rejected:  # Y Y^H of rank T < M has no inverse: the reference has no such output
        assert "pb_scale_0" not in c.refs[0] and "normalize_pb_W" not in c.refs[0]
        return
    for r in env.reference_ids(c.M):
        status = c.eng.new_status(c.B)
        c.poison()
        c.check("pb_scale_%d" % r, c.eng.projection_back_scale(c["X"], c["W"], r, status))
        assert not status.cpu().numpy().any()
    W, Tb = c["W"], c["Tb"]
    c.eng.ilrma_normalize_pb(W, Tb, c.ref("pb_scale_0"), domain=c.domain)
    c.check("normalize_pb_W", W)
    c.check("normalize_pb_Tb", Tb)


@params
def test_nmf_half_sums_on_the_power_map(case, dtype):
    import torch
    from audio_source_separation_amd import _lib
    c = Case(case, dtype)
    P, Tb, V = c.ref("power_map"), c["Tb"], c["V"]
    if c.K > env.NMF_HALF_SUMS_MAX_K:
        with pytest.raises(_lib.AssxError, match="n_basis"):
            c.eng.nmf_half_sums(_lib.NMF_IS_MM, 0, P[0], Tb[0], V[0], domain=c.domain)
        return
    for half, output, shape in ((0, "half_sums_basis", (2, c.M, c.F, c.K)), (1, "half_sums_act", (2, c.M, c.K, c.T))):
        got = []
        for b in range(c.B):  # the batch axis of the NMF entry point is the sources of one utterance
            c.eng._nmf_scratch(c.M, c.F, c.T, c.K)
            c.eng._ws.buf.fill_(0xFF)
            sums = c.eng.nmf_half_sums(_lib.NMF_IS_MM, half, P[b], Tb[b], V[b], domain=c.domain)
            got.append(sums.reshape(shape))
        c.check(output, torch.stack(got))


@params
def test_nmf_apply_sums(case, dtype):
    from audio_source_separation_amd import _lib
    c = Case(case, dtype)
    Tb = c["Tb"]
    sums = c.ref("_apply_sums_in")  # (B, 2, N, F, K)
    for b in range(c.B):
        c.eng.nmf_apply_sums(_lib.NMF_IS_MM, Tb[b], sums[b].reshape(2, c.M, c.F * c.K).contiguous(), domain=c.domain)
    c.check("apply_sums", Tb)


@params
def test_ordered_sum(case, dtype):
    import torch
    c = Case(case, dtype)
    P = c.ref("power_map")  # (B, N, F, T): the N maps of an utterance are the parts
    c.check("ordered_sum", torch.stack([c.eng.ordered_sum(P[b]) for b in range(c.B)]))
    i = env.ILRMA_FIELDS.index("sum_weights")
    wts = [torch.from_numpy(np.ascontiguousarray(s[i])).to(c.eng.dev) for s in c.states]  # float64 in both precisions
    c.check("ordered_sum_weighted", torch.stack([c.eng.ordered_sum(P[b], wts[b]) for b in range(c.B)]))


# ------------------------------------------------------------------------------------------- squeezed partitions
@pytest.fixture
def few_workgroups():
    """Force the flat partitions down to a handful of workgroups (ASSX_G), so that a small input gives every workgroup
    a long range: ranges that start and end in the middle of a bin, flush several partial records and cross
    utterances.  The variable is removed afterwards."""
    def _set(g):
        os.environ["ASSX_G"] = str(g)
    yield _set
    os.environ.pop("ASSX_G", None)


@pytest.mark.parametrize("step", [_source_update, _loss, _spatial_ip_dense, _cov_accumulate_nt],
                         ids=["source_update", "loss", "spatial_ip", "cov_accumulate"])
@pytest.mark.parametrize("case,dtype", [(c, d) for d in DTYPES for c in env.ILRMA_STREAM_CASES])
def test_streaming_entry_points_on_three_workgroups(few_workgroups, case, dtype, step):
    few_workgroups(3)
    step(Case(case, dtype))
