"""GaussIDLMA without a GPU: the NumPy restatement (tests/idlma_np.py) against the reference's recorded runs
(tests/golden/idlma, tolerances of tools/idlma_tolerance_probe.py), the faults the fixtures must notice, the C-ABI and the
class's surface."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import idlma_np as idl  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "idlma")
NAMES = [c[0] for c in idl.CASES]
ENTRY_POINTS = ["assx_idlma_dnn_input", "assx_idlma_loss", "assx_idlma_normalize_pb", "assx_idlma_space_update",
                "assx_idlma_step", "assx_idlma_variance", "assx_idlma_workspace_bytes"]
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
            _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def tolerances(name):
    if "tol" not in _CACHE:
        _CACHE["tol"] = json.load(open(os.path.join(GOLDEN, "tolerances.json")))
    return _CACHE["tol"]["fixtures"][name]


def identity(fx):
    M, F, T = fx["X"].shape
    return np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1))


def test_the_cases_the_fixtures_cover():
    cases = {(c[1], c[2], c[3], c[4], c[5]) for c in idl.CASES}
    assert {(2, 5, 32, 2, "exact"), (3, 7, 48, 1, "exact"), (2, 5, 32, 1.5, "exact"), (4, 9, 64, 2, "matmul"),
            (8, 6, 40, 2, "exact"), (2, 17, 96, 2, "exact")} <= cases
    for name in NAMES:
        fx = fixture(name)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
        assert float(fx["max_cond"]) < 1e6
        for i in range(1, idl.N_ITER + 1):
            assert fx["inp_%d" % i].dtype == fx["raw_%d" % i].dtype == fx["d_%d" % i].dtype == np.float32
        assert len(fx["loss"]) == idl.N_ITER + 1
    eps_case, floor_case = fixture("idlma_m2_f17_t96_d2_epsfloor"), fixture("idlma_m3_f7_t48_d1_dnnfloor")
    assert float(eps_case["dnn_flooring"]) == 0 and np.sum(eps_case["d_1"] == 0) >= 4  # R meets the eps floor
    assert np.sum(floor_case["d_1"] == np.float32(1e-5)) >= 5
    assert int(fixture("idlma_m3_f5_t40_d2_ref1")["reference_id"]) == 1


@pytest.mark.parametrize("name", NAMES)
def test_restatement_stage_by_stage(name):
    fx, tol, p = fixture(name), tolerances(name), idl.params(fixture(name))
    X, stage, it = fx["X"], tolerances(name)["one_stage"], tolerances(name)["one_iteration"]
    net = idl.build_net(fx)
    for i in range(1, idl.N_ITER + 1):
        W0 = identity(fx) if i == 1 else fx["W_%d" % (i - 1)]
        inp = idl.network_input(X, W0, p["domain"])
        assert inp.dtype == np.float32 and idl.d_metric(inp, fx["inp_%d" % i]) <= stage["inp"]
        if "net_g" in fx:  # correctly rounded operations only
            assert np.array_equal(idl.run_net(net, fx["inp_%d" % i]), fx["raw_%d" % i])
        d = idl.source_output(fx["raw_%d" % i], p["domain"], p["dnn_flooring"])
        assert d.dtype == np.float32 and np.array_equal(d, fx["d_%d" % i])
        R = idl.variance(d, p["domain"], p["eps"])
        assert R.dtype == np.float32 and R.min() >= np.float32(p["eps"])
        assert idl.w_metric(idl.space_update(X, W0, R), fx["Wip_%d" % i]) <= stage["W"]
        Y = idl.separate(X, fx["Wip_%d" % i])
        scale = idl.pb_scale(Y, X[p["reference_id"]])
        assert idl.out_metric(scale, fx["scale_%d" % i]) <= stage["scale"]
        assert idl.w_metric(idl.normalize_refit(X, Y, scale), fx["W_%d" % i]) <= stage["W"]
        for value in (idl.loss(X, fx["W_%d" % i], d, p["domain"], p["eps"]),
                      idl.kernel_loss(X, fx["W_%d" % i], d, p["domain"], p["eps"])):
            assert idl.loss_metric(value, fx["loss"][i], X) <= stage["loss"]
        gW, gd, gl = idl.iterate(X, W0, net, **p)
        assert idl.w_metric(gW, fx["W_%d" % i]) <= it["W"] and idl.d_metric(gd, fx["d_%d" % i]) <= it["d"]
        assert idl.loss_metric(gl, fx["loss"][i], X) <= it["loss"]
    assert tol["one_stage"]["W"] >= 16 * 2.0 ** -52


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", ["refit", "scaled"])
def test_restatement_whole_run(name, form):
    fx, tol, p = fixture(name), tolerances(name)["whole_run"], idl.params(fixture(name))
    W, d, losses, out = idl.run(fx["X"], idl.build_net(fx), form=form, **p)
    assert idl.w_metric(W, fx["W_%d" % idl.N_ITER]) <= tol["W"]
    assert d.dtype == np.float32 and idl.d_metric(d, fx["d_%d" % idl.N_ITER]) <= tol["d"]
    assert idl.loss_metric(losses, fx["loss"], fx["X"]) <= tol["loss"]
    assert idl.out_metric(out, fx["output"]) <= tol["out"]


@pytest.mark.parametrize("fault", ["f64_square", "floor_first", "single_exponent", "loss_before_normalize"])
def test_the_fixtures_notice_a_planted_fault(fault):
    """One iteration from every recorded state with the fault planted: on at least one fixture a figure must leave its
    tolerance (or d its type), while the restatement without the fault stays inside on all of them."""
    caught = []
    for name in NAMES:
        fx, it, p = fixture(name), tolerances(name)["one_iteration"], idl.params(fixture(name))
        net = idl.build_net(fx)
        for i in (1, idl.N_ITER):
            W0 = identity(fx) if i == 1 else fx["W_%d" % (i - 1)]
            gW, gd, gl = idl.iterate(fx["X"], W0, net, fault=fault, raw=fx["raw_%d" % i], **p)
            bad = gd.dtype != np.float32 or idl.w_metric(gW, fx["W_%d" % i]) > it["W"] \
                or idl.d_metric(gd, fx["d_%d" % i]) > it["d"] or idl.loss_metric(gl, fx["loss"][i], fx["X"]) > it["loss"]
            if bad:
                caught.append((name, i))
    print(fault, caught)
    assert caught, fault


@pytest.mark.parametrize("name", NAMES)
def test_scaled_form_against_the_refit(name):
    fx, p = fixture(name), idl.params(fixture(name))
    bound = tolerances(name)["scaled_vs_refit"]
    assert bound < 1e-11  # rounding level
    for i in range(1, idl.N_ITER + 1):
        scaled = idl.normalize_scaled(fx["Wip_%d" % i], fx["scale_%d" % i])
        assert idl.w_metric(scaled, fx["W_%d" % i]) <= bound


def test_generator_and_probe_reproduce_the_committed_files():
    if not os.path.isdir(os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")):
        pytest.skip("the reference tree is not present")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_idlma.py"), "--verify"], capture_output=True,
                             text=True)
    assert run.returncode == 0 and run.stdout.count("identical") == len(NAMES), run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_ctypes_table_and_library_agree():
    from audio_source_separation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "assx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(assx_idlma_[a-z0-9_]+)\s*\(", text)))
    assert declared == ENTRY_POINTS
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("assx_idlma_")) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in declared:
        assert hasattr(lib, n), n
    build = open(os.path.join(ROOT, "audio_source_separation_amd", "csrc", "build.sh")).read()
    assert build.count("assx_idlma") == 2  # the SRCS list and the link line
    chunk = int(re.search(r"#define ASSX_IDLMA_FRAME_CHUNK (\d+)", raw).group(1))
    assert chunk == _lib.IDLMA_FRAME_CHUNK == idl.FRAME_CHUNK
    from audio_source_separation_amd.ops import Engine
    for n in ("workspace", "dnn_input", "variance", "normalize_pb", "loss", "step", "space_update"):
        assert callable(getattr(Engine, "idlma_" + n))


def test_workspace_query_needs_no_gpu():
    from audio_source_separation_amd import _lib
    q = _lib.lib.assx_idlma_workspace_bytes
    base = q(4, 17, 1025)
    assert base > 0 and q(5, 17, 1025) > base and q(4, 18, 1025) > base and q(4, 17, 2049) > base
    assert q(2, 1, 2) > 0 and q(8, 1, 8) > 0
    for M, F, T in ((1, 17, 65), (9, 17, 65), (4, 0, 65), (4, 17, 3), (4, -1, 65), (4, 17, -1), (8, 1, 7)):
        assert q(M, F, T) == 0, (M, F, T)
    assert q(8, 4096, 8191) > 0 and q(8, 4096, 8192) == 0  # M F T < 2^28
    assert q(2, 2 ** 31 - 1, 2 ** 31 - 1) == 0


def test_c_abi_refuses_a_null_context_without_a_gpu():
    from audio_source_separation_amd import _lib
    L, null, E_NULL = _lib.lib, ctypes.c_void_p(0), -3
    for M, F, T in ((4, 5, 6), (9, 0, -1)):
        assert L.assx_idlma_dnn_input(null, null, null, 2.0, null, M, F, T, null) == E_NULL
        assert L.assx_idlma_variance(null, null, 2.0, 1e-5, 1e-12, null, null, M, F, T, null) == E_NULL
        assert L.assx_idlma_normalize_pb(null, null, null, M, F, null) == E_NULL
        assert L.assx_idlma_loss(null, null, null, null, null, null, M, F, T, null) == E_NULL
        assert L.assx_idlma_step(null, null, null, null, 2.0, 1e-5, 1e-12, 1e12, 0, null, null, null, null, null, M, F, T,
                                 null) == E_NULL


# ------------------------------------------------------------------------------------------------ the class's surface
def test_signature_defaults_and_repr():
    from audio_source_separation_amd.sss.idlma import GaussIDLMA, IDLMAbase, update_space_model, EPS, THRESHOLD
    sig = inspect.signature(GaussIDLMA.__init__)
    assert list(sig.parameters) == ["self", "domain", "normalize", "reference_id", "callback", "dnn_flooring", "eps",
                                    "threshold", "dtype", "device"]
    want = dict(domain=2, normalize='power', reference_id=0, callback=None, dnn_flooring=1e-5, eps=1e-12, threshold=1e12,
                dtype='float64', device=None)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want
    assert sig.parameters["dtype"].kind == sig.parameters["device"].kind == inspect.Parameter.KEYWORD_ONLY
    base = inspect.signature(IDLMAbase.__init__)
    assert [(k, v.default) for k, v in base.parameters.items()][1:5] == [("normalize", True), ("callback", None),
                                                                        ("dnn_flooring", 1e-5), ("eps", 1e-12)]
    assert EPS == 1e-12 and THRESHOLD == 1e12
    assert list(inspect.signature(GaussIDLMA.update_once).parameters) == ["self", "is_source_model_update"]
    assert inspect.signature(GaussIDLMA.update_once).parameters["is_source_model_update"].default is True
    assert list(inspect.signature(GaussIDLMA.__call__).parameters) == ["self", "input", "iteration", "kwargs"]
    for n in ("update_source_model", "update_space_model", "estimate_by_dnn", "floor_dnn_output", "separate",
              "compute_negative_loglikelihood"):
        assert callable(getattr(GaussIDLMA, n))
    m = GaussIDLMA(normalize='projection-back')
    assert "GaussIDLMA" in repr(m) and m.loss == [] and m.input is None and m.callback is None
    assert not hasattr(m, "demix_filter") and not hasattr(m, "dnn_output")
    assert callable(update_space_model)  # the free function stays


class _NoParams(torch.nn.Module):
    def forward(self, x):
        return x


def _net(M=2, F=3, T=8):
    return idl.ExactNet(np.ones((M, F, 1), dtype=np.float32))


def test_every_refusal_touches_neither_a_device_nor_the_rng():
    """ValueError before a device is touched: where no GPU is present, opening one would raise RuntimeError instead."""
    from audio_source_separation_amd.sss.idlma import GaussIDLMA
    rng = np.random.default_rng(0)
    X = rng.standard_normal((2, 3, 8)) + 1j * rng.standard_normal((2, 3, 8))
    np.random.seed(5)
    state = np.random.get_state()
    torch_state = torch.random.get_rng_state()
    pb = dict(normalize='projection-back')
    with pytest.raises(ValueError, match="float64"):
        GaussIDLMA(dtype='float32', **pb)
    with pytest.raises(ValueError, match="domain"):
        GaussIDLMA(domain=2.5, **pb)
    with pytest.raises(ValueError, match="domain"):
        GaussIDLMA(domain=0.5, **pb)
    cases = [
        (dict(pb), X, dict(), "dnn"),                                                  # dnn missing
        (dict(pb), X, dict(dnn=_NoParams()), "no parameters"),
        (dict(pb), X, dict(dnn=_net()), "no CPU fallback"),                           # parameters on the CPU
        (dict(), X, dict(dnn=_net()), "Not support normalization based on power. Choose 'power' or 'projection-back'"),
        (dict(normalize='other'), X, dict(dnn=_net()), "Not support normalization based on other"),
        (dict(normalize=False), X, dict(dnn=_net()), "Set normalize=True"),
        (dict(pb), X[:1], dict(dnn=_net()), "n_channels"),
        (dict(pb), np.concatenate([X] * 5)[:9], dict(dnn=_net()), "n_channels"),
        (dict(pb), np.concatenate([X, X])[:, :, :3], dict(dnn=_net()), "n_frames >= n_channels"),
        (dict(pb), X.real, dict(dnn=_net()), "complex"),
        (dict(pb), X[0], dict(dnn=_net()), "one utterance"),
        (dict(pb), X[None], dict(dnn=_net()), "one utterance"),
        (dict(pb, reference_id=2), X, dict(dnn=_net()), "reference_id"),
        (dict(pb, reference_id=-1), X, dict(dnn=_net()), "reference_id"),
        (dict(pb, reference_id=0.0), X, dict(dnn=_net()), "reference_id"),
        (dict(pb), X, dict(dnn=_net(), domain=3), "domain"),
        (dict(pb), X, dict(dnn=_net(), dtype='float32'), "float64"),
    ]
    for ctor, x, call, text in cases:
        m = GaussIDLMA(**ctor)
        with pytest.raises(ValueError, match=re.escape(text)):
            m(x, iteration=1, **call)
        assert m._engine is None and list(m.loss) == [] and not hasattr(m, "demix_filter")
    m = GaussIDLMA(**pb)
    with pytest.raises(ValueError, match="demix_filter has shape"):
        m.demix_filter = np.zeros((3, 3, 3), dtype=complex)
        m(X, iteration=1, dnn=_net())
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()) if isinstance(a, np.ndarray))
    assert torch.equal(torch_state, torch.random.get_rng_state())


def test_loss_list_semantics():
    """`loss` is made by the constructor and every call appends to it (idlma.py:15, 52-59); here without a device: the list
    survives a refused call untouched, and is the constructor's object."""
    from audio_source_separation_amd.sss.idlma import GaussIDLMA
    m = GaussIDLMA(normalize='projection-back')
    kept = m.loss
    m.loss.append(1.5)
    with pytest.raises(ValueError):
        m(np.zeros((2, 3, 8), dtype=complex), iteration=2)
    assert m.loss is kept and list(m.loss) == [1.5]
    # the restatement's list: the entry before the loop with dnn_output = ones, then one per iteration
    fx = fixture(NAMES[0])
    p = idl.params(fx)
    first = idl.loss(fx["X"], identity(fx), np.ones(fx["X"].shape), p["domain"], p["eps"])
    assert idl.loss_metric(first, fx["loss"][0], fx["X"]) <= tolerances(NAMES[0])["one_stage"]["loss"]
