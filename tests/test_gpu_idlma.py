"""GaussIDLMA on the GPU: every entry point of csrc/assx_idlma.hip from the reference's recorded states, the fused calls
against the single ones bit for bit, and the class through its front door (tests/golden/idlma, tolerances of
tools/idlma_tolerance_probe.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import idlma_np as idl  # noqa: E402
from test_idlma_cpu import NAMES, fixture, identity, tolerances  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(device="cuda:0")


def dev(eng, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=eng.dev)


def host(t):
    return t.cpu().numpy()


def same(a, b):
    """bit for bit, NaN included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def single_calls(eng, X, W0, raw, p, want_input=True):
    """One iteration after the network as single calls: (W, dnn_output, R, scale, loss, next input)."""
    M, F, T = X.shape
    Xd, W, status = dev(eng, X), dev(eng, W0).clone(), eng.new_status(1)
    d, R = eng.empty((M, F, T), dtype=torch.float32), eng.empty((M, F, T), dtype=torch.float64)
    eng.idlma_variance(dev(eng, raw), d, R, domain=p["domain"], dnn_flooring=p["dnn_flooring"], eps=p["eps"])
    eng.idlma_space_update(Xd.unsqueeze(0), W.unsqueeze(0), R.unsqueeze(0), domain=2, eps=float(np.float32(p["eps"])),
                           status=status)
    W_ip = W.clone()
    scale = eng.projection_back_scale(Xd.unsqueeze(0), W.unsqueeze(0), p["reference_id"], status)[0]
    eng.idlma_normalize_pb(W, scale)
    ws = eng.idlma_workspace(M, F, T)
    loss = eng.idlma_loss(Xd, W, R, ws)
    inp = eng.idlma_dnn_input(Xd, W, domain=p["domain"]) if want_input else None
    assert int(status.item()) & 1 == 0
    return dict(W=host(W), W_ip=host(W_ip), d=host(d), R=host(R), scale=host(scale), loss=host(loss),
                inp=None if inp is None else host(inp))


def one_step(eng, X, W0, raw, p, want_loss=True, want_input=True):
    M, F, T = X.shape
    Xd, W, status = dev(eng, X), dev(eng, W0).clone(), eng.new_status(1)
    d = eng.empty((M, F, T), dtype=torch.float32)
    loss = eng.empty((1,), dtype=torch.float64) if want_loss else None
    inp = eng.empty((M, F, T), dtype=torch.float32) if want_input else None
    eng.idlma_step(Xd, W, dev(eng, raw), d, eng.idlma_workspace(M, F, T), loss=loss, next_input=inp, status=status,
                   domain=p["domain"], dnn_flooring=p["dnn_flooring"], eps=p["eps"], ref=p["reference_id"])
    assert int(status.item()) & 1 == 0
    return dict(W=host(W), d=host(d), loss=None if loss is None else host(loss), inp=None if inp is None else host(inp))


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_from_recorded_states(eng, name):
    fx, p = fixture(name), idl.params(fixture(name))
    stage, it = tolerances(name)["one_stage"], tolerances(name)["one_iteration"]
    X, net = fx["X"], idl.build_net(fx, eng.dev)
    exact_pow = p["domain"] in (1.0, 2.0)
    for i in (1, 2, idl.N_ITER):
        W0 = identity(fx) if i == 1 else fx["W_%d" % (i - 1)]
        inp = host(eng.idlma_dnn_input(dev(eng, X), dev(eng, W0), domain=p["domain"]))
        assert inp.dtype == np.float32 and idl.d_metric(inp, fx["inp_%d" % i]) <= stage["inp"]
        if "net_g" in fx:  # the precondition of every bitwise claim about the exact net
            with torch.no_grad():
                assert same(host(net(dev(eng, fx["inp_%d" % i]))), fx["raw_%d" % i]), "the exact net is not exact here"
        got = single_calls(eng, X, W0, fx["raw_%d" % i], p, want_input=True)
        if exact_pow:
            assert same(got["d"], fx["d_%d" % i])
            assert same(got["R"], idl.variance(fx["d_%d" % i], p["domain"], p["eps"]).astype(np.float64))
        else:
            assert idl.d_metric(got["d"], fx["d_%d" % i]) <= it["d"]
        # one stage: the sweep on the reference's variance (out of powf the GPU's own is float32 steps from it)
        Rd, Wd = dev(eng, idl.variance(fx["d_%d" % i], p["domain"], p["eps"]).astype(np.float64)), dev(eng, W0).clone()
        eng.idlma_space_update(dev(eng, X).unsqueeze(0), Wd.unsqueeze(0), Rd.unsqueeze(0), domain=2,
                               eps=float(np.float32(p["eps"])))
        assert idl.w_metric(host(Wd), fx["Wip_%d" % i]) <= stage["W"]
        assert not exact_pow or same(host(Wd), got["W_ip"])
        assert idl.w_metric(got["W"], fx["W_%d" % i]) <= it["W"]  # the iteration
        assert idl.loss_metric(got["loss"][0], fx["loss"][i], X) <= it["loss"]
        # the scale, the normalisation and the loss as single stages, from the recorded state before each
        M, F, T = X.shape
        Wip = dev(eng, fx["Wip_%d" % i]).clone()
        scale = eng.projection_back_scale(dev(eng, X).unsqueeze(0), Wip.unsqueeze(0), p["reference_id"], eng.new_status(1))[0]
        assert idl.out_metric(host(scale), fx["scale_%d" % i]) <= stage["scale"]
        eng.idlma_normalize_pb(Wip, dev(eng, fx["scale_%d" % i]))
        assert idl.w_metric(host(Wip), fx["W_%d" % i]) <= stage["W"]
        R = dev(eng, idl.variance(fx["d_%d" % i], p["domain"], p["eps"]).astype(np.float64))
        alone = host(eng.idlma_loss(dev(eng, X), dev(eng, fx["W_%d" % i]), R, eng.idlma_workspace(M, F, T)))
        assert idl.loss_metric(alone[0], fx["loss"][i], X) <= stage["loss"]
        # everything in one call: the same bits, with and without the loss and the next input
        for want_loss, want_input in ((True, True), (True, False), (False, True), (False, False)):
            fused = one_step(eng, X, W0, fx["raw_%d" % i], p, want_loss, want_input)
            assert same(fused["W"], got["W"]) and same(fused["d"], got["d"])
            assert not want_loss or same(fused["loss"], got["loss"])
            assert not want_input or same(fused["inp"], got["inp"])
        again = one_step(eng, X, W0, fx["raw_%d" % i], p)
        assert all(same(again[k], fused_k) for k, fused_k in one_step(eng, X, W0, fx["raw_%d" % i], p).items())


def test_variance_passes_nan_and_both_floors(eng):
    raw = np.array([[[np.nan, 0.0, 1e-7, 2.0, 1e-3, np.inf, 3.0]]], dtype=np.float32).repeat(2, axis=0)
    raw = np.ascontiguousarray(np.concatenate([raw, raw], axis=2))  # (2,1,14): T >= M
    for domain in (1, 1.5, 2):
        for flooring in (1e-5, 0.0):
            d, R = eng.empty(raw.shape, dtype=torch.float32), eng.empty(raw.shape, dtype=torch.float64)
            eng.idlma_variance(dev(eng, raw), d, R, domain=domain, dnn_flooring=flooring, eps=1e-12)
            want_d = idl.source_output(raw, domain, flooring)
            want_R = idl.variance(want_d, domain, 1e-12).astype(np.float64)
            if domain == 1.5:
                assert np.array_equal(np.isnan(host(d)), np.isnan(want_d)) and idl.d_metric(
                    np.nan_to_num(host(d), posinf=1.0), np.nan_to_num(want_d, posinf=1.0)) <= 16 * 2 * 2.0 ** -23
            else:
                assert same(host(d), want_d) and same(host(R), want_R)
            assert np.isnan(host(d)[0, 0, 0]) and np.isnan(host(R)[0, 0, 0])
            # a dnn_output as it stands: only R is written
            keep = dev(eng, want_d).clone()
            eng.idlma_variance(None, keep, R, domain=domain, eps=1e-12)
            assert same(host(keep), want_d)
            if domain != 1.5:
                assert same(host(R), want_R)


# ------------------------------------------------------------------------------------------------ the class
def model(fx, **kw):
    from audio_source_separation_amd.sss.idlma import GaussIDLMA
    p = idl.params(fx)
    return GaussIDLMA(domain=p["domain"], normalize='projection-back', reference_id=p["reference_id"],
                      dnn_flooring=p["dnn_flooring"], eps=p["eps"], device="cuda:0", **kw)


def check_front_door(m, out, fx, tol):
    X = fx["X"]
    assert idl.w_metric(m.demix_filter, fx["W_%d" % idl.N_ITER]) <= tol["W"]
    assert m.dnn_output.dtype == np.float32 and idl.d_metric(m.dnn_output, fx["d_%d" % idl.N_ITER]) <= tol["d"]
    assert len(m.loss) == idl.N_ITER + 1 and idl.loss_metric(np.array(m.loss), fx["loss"], X) <= tol["loss"]
    assert idl.out_metric(out, fx["output"]) <= tol["out"]
    assert same(np.asarray(m.estimation), np.asarray(out))


@pytest.mark.parametrize("name", NAMES)
def test_front_door_numpy_and_tensor(eng, name):
    fx, tol = fixture(name), tolerances(name)["whole_run"]
    net = idl.build_net(fx, eng.dev)
    m = model(fx)
    out = m(fx["X"], iteration=idl.N_ITER, dnn=net)
    assert isinstance(out, np.ndarray) and out.dtype == np.complex128
    check_front_door(m, out, fx, tol)
    m2 = model(fx)
    out2 = m2(dev(eng, fx["X"]), iteration=idl.N_ITER, dnn=net)
    assert isinstance(out2, torch.Tensor) and out2.device == eng.dev
    assert same(host(out2), out) and same(np.asarray(m2.demix_filter), np.asarray(m.demix_filter))
    assert same(np.array(m2.loss), np.array(m.loss)) and same(m2.dnn_output, m.dnn_output)


@pytest.mark.parametrize("name", ["idlma_m2_f5_t32_d15", "idlma_m3_f7_t48_d1_dnnfloor", "idlma_m4_f9_t64_d2_matmul"])
def test_public_steps_callback_and_subclass_equal_the_fast_loop(eng, name):
    from audio_source_separation_amd.sss.idlma import GaussIDLMA
    fx = fixture(name)
    net = idl.build_net(fx, eng.dev)
    fast = model(fx)
    assert fast._fast_loop_ok()
    out = fast(fx["X"], iteration=4, dnn=net)

    def agrees(m, o):
        return same(o, out) and same(np.asarray(m.demix_filter), np.asarray(fast.demix_filter)) \
            and same(np.array(m.loss), np.array(fast.loss)) and same(m.dnn_output, fast.dnn_output)

    seen = []
    with_cb = model(fx, callback=lambda mm: seen.append(len(mm.loss)))
    assert not with_cb._fast_loop_ok()
    assert agrees(with_cb, with_cb(fx["X"], iteration=4, dnn=net)) and seen == [2, 3, 4, 5]

    class Floored(GaussIDLMA):
        calls = 0

        def floor_dnn_output(self):
            type(self).calls += 1
            super().floor_dnn_output()

    p = idl.params(fx)
    sub = Floored(domain=p["domain"], normalize='projection-back', reference_id=p["reference_id"],
                  dnn_flooring=p["dnn_flooring"], eps=p["eps"], device="cuda:0")
    assert not sub._fast_loop_ok()
    assert agrees(sub, sub(fx["X"], iteration=4, dnn=net)) and Floored.calls == (4 if p["dnn_flooring"] else 0)

    # by hand, as the reference's __call__ drives it
    hand = model(fx)
    hand(fx["X"], iteration=0, dnn=net)
    assert len(hand.loss) == 1 and same(np.array(hand.loss), np.array(fast.loss)[:1])
    for _ in range(4):
        hand.update_once()
        hand.loss.append(hand.compute_negative_loglikelihood())
    assert same(np.asarray(hand.demix_filter), np.asarray(fast.demix_filter)) and same(hand.dnn_output, fast.dnn_output)
    assert same(np.array(hand.loss), np.array(fast.loss))
    Y = hand.separate(fx["X"], hand.demix_filter)
    assert idl.out_metric(Y, idl.separate(fx["X"], np.asarray(hand.demix_filter))) <= 1e-13


def test_warm_start_loss_list_and_source_model_switch(eng):
    fx = fixture("idlma_m3_f5_t40_d2_ref1")
    X, p, net = fx["X"], idl.params(fx), idl.build_net(fx, eng.dev)
    whole = model(fx)
    whole(X, iteration=6, dnn=net)
    parts = model(fx)
    parts(X, iteration=2, dnn=net)
    parts(X, iteration=4, dnn=net)  # continues from demix_filter; dnn_output starts from ones again
    assert same(np.asarray(parts.demix_filter), np.asarray(whole.demix_filter))
    assert len(parts.loss) == 3 + 5 and same(np.array(parts.loss)[:3], np.array(whole.loss)[:3])
    assert same(np.array(parts.loss)[4:], np.array(whole.loss)[3:])
    del parts.demix_filter
    parts(X, iteration=0, dnn=net)
    assert same(np.asarray(parts.demix_filter), identity(fx)) and len(parts.loss) == 9
    assert same(parts.dnn_output, np.ones(X.shape, dtype=np.float32))
    # a user's array as the warm start
    W0 = fx["W_3"]
    warm = model(fx)
    warm.demix_filter = W0.copy()
    warm(X, iteration=1, dnn=net)
    assert idl.w_metric(warm.demix_filter, fx["W_4"]) <= tolerances("idlma_m3_f5_t40_d2_ref1")["one_iteration"]["W"]
    # update_once(False): the sweep on the source model as it stands (ones after a reset)
    m = model(fx)
    m(X, iteration=0, dnn=net)
    m.update_once(is_source_model_update=False)
    W_ip = idl.space_update(X, identity(fx), np.ones(X.shape))
    want = idl.normalize_scaled(W_ip, idl.pb_scale(idl.separate(X, W_ip), X[p["reference_id"]]))
    assert idl.w_metric(m.demix_filter, want) <= tolerances("idlma_m3_f5_t40_d2_ref1")["one_iteration"]["W"]
    assert same(m.dnn_output, np.ones(X.shape, dtype=np.float32))
    # estimate_by_dnn: NumPy in, NumPy out; tensor in, tensor out
    P = idl.power(X, identity(fx))
    e = m.estimate_by_dnn(P)
    assert isinstance(e, np.ndarray) and e.dtype == np.float32 and same(e, fx["raw_1"])  # domain 2: the network alone
    assert isinstance(m.estimate_by_dnn(dev(eng, P)), torch.Tensor)


class _NaNNet(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        y = self.net(x).clone()
        y[0, 1, 2] = float("nan")
        return y


class _Bad(torch.nn.Module):
    def __init__(self, net, how):
        super().__init__()
        self.net, self.how = net, how

    def forward(self, x):
        y = self.net(x)
        return {"shape": y[:, :, :-1], "dtype": y.double(), "kind": None, "host": y.cpu()}[self.how]


def test_nan_singular_bin_and_refusals(eng):
    from audio_source_separation_amd.sss.idlma import GaussIDLMA
    fx = fixture("idlma_m2_f5_t32_d2")
    X, net = fx["X"], idl.build_net(fx, eng.dev)
    # a NaN from the network reaches dnn_output and the loss, and stays in its bin
    m = model(fx)
    m(X, iteration=0, dnn=_NaNNet(net))
    m.update_once()
    assert np.isnan(m.dnn_output[0, 1, 2]) and np.sum(np.isnan(m.dnn_output)) == 1
    assert np.isnan(m.compute_negative_loglikelihood()) and not np.isnan(m.loss[0])
    assert np.all(np.isfinite(np.asarray(m.demix_filter)[[0, 2, 3, 4]]))
    # a singular bin raises where the model is next synchronised
    Xs = X.copy()
    Xs[:, 3, :] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        model(fx)(Xs, iteration=1, dnn=net)
    # what the network returns
    for how in ("shape", "dtype", "kind", "host"):
        with pytest.raises(ValueError, match="dnn must return"):
            model(fx)(X, iteration=1, dnn=_Bad(net, how))
    # refusals that need no GPU are refused the same way with one present, before anything runs
    with pytest.raises(ValueError, match="no CPU fallback"):
        model(fx)(X, iteration=1, dnn=idl.build_net(fx, "cpu"))
    with pytest.raises(ValueError, match="Not support normalization based on power"):
        GaussIDLMA(device="cuda:0")(X, iteration=1, dnn=net)
    with pytest.raises(ValueError, match="n_frames >= n_channels"):
        model(fx)(X[:, :, :1], iteration=1, dnn=net)
    # the C-ABI's own envelope
    from audio_source_separation_amd._lib import AssxError
    Xd, Wd = dev(eng, X), dev(eng, identity(fx))
    with pytest.raises(AssxError, match="domain"):
        eng.idlma_dnn_input(Xd, Wd, domain=2.5)
    with pytest.raises(ValueError):
        eng.idlma_dnn_input(Xd, Wd[:-1].contiguous())
    with pytest.raises(ValueError, match="workspace"):
        eng.idlma_loss(Xd, Wd, eng.empty(X.shape, dtype=torch.float64), torch.empty(8, dtype=torch.uint8, device=eng.dev))
