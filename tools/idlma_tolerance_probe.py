#!/usr/bin/env python3
"""Measure the tolerances of the GaussIDLMA tests and write tests/golden/idlma/tolerances.json (CPU only; runs where the
reference tree is present, like tests/golden/idlma/make_idlma.py).  The recipe is that of DESIGN.md section 14.4.

Metrics (tests/idlma_np.py): W, per bin max|a - b| / max|b|; inp and d (float32 maps), entry-wise |a - b| / |b|; loss,
|a - b| / (|b| + M n_bins n_frames); out and scale, per source max|a - b| / max|b|.  For every fixture, against the reference:

  restatement   tests/idlma_np.py in the reference's own form (the refit, a float32 logarithm)
  kernel model  the same with the kernels' choices: W[f,n,:] *= scale[n,f] instead of the refit, log R as the float64
                logarithm rounded to float32, the loss added up in the kernel's order (idlma_np.kernel_loss)
  sensitivity   the reference against itself after every real and imaginary part of what the step reads (X and W) moved
                to a neighbouring double (the largest of N_DRAWS draws).  Where the network's output is not the same on
                every machine -- the matmul net, and the powf of a domain other than 1 and 2 -- its output is moved to a
                neighbouring float32 as well

`one_stage`: the network's input, the sweep, the scale, the normalisation and the loss, each from the recorded state before
it.  `one_iteration`: from every recorded state to the next.  `whole_run`: N_ITER iterations from the identity, compared
at the end (the loss: the largest figure over the list).  A tolerance is FACTOR x the largest of the three figures and at
least FACTOR x 2^-52; for a float32 map the figure is at least 2^-24, half a float32 step, because a float64 difference of
any size can move a rounded value by one whole step -- and at least 2 x 2^-23 for d where it comes out of powf, two
implementations of which may each be one step from the true value.  `scaled_vs_refit` is the largest W figure between the
two forms of the normalisation, recorded as measured.  A restated sweep further than LIMIT / FACTOR from the reference's
means that the restatement is not the reference's update: nothing is written then.

    python tools/idlma_tolerance_probe.py            # writes tolerances.json
    python tools/idlma_tolerance_probe.py --check    # measures and compares with the committed file
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "idlma"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import idlma_np as idl  # noqa: E402
import make_idlma as mk  # noqa: E402

FACTOR = 16
LIMIT = 1e-9
RESOLUTION = 2.0 ** -52
F32_HALF_STEP = 2.0 ** -24
N_DRAWS = 3
OUT = os.path.join(ROOT, "tests", "golden", "idlma", "tolerances.json")


class Moved(torch.nn.Module):
    """the network with every output moved to a neighbouring float32"""

    def __init__(self, net, rng):
        super().__init__()
        self.net, self.rng = net, rng

    def forward(self, x):
        return torch.from_numpy(idl.one_ulp(self.net(x).numpy(), self.rng))


def f32_sensitive(fx):
    return "net_g" not in fx or float(fx["domain"]) not in (1.0, 2.0)


def reference_at(fx, X, W, net):
    """The reference at a given state, without its reset."""
    _, GaussIDLMA = mk.reference()
    p = idl.params(fx)
    m = GaussIDLMA(domain=p["domain"], normalize='projection-back', reference_id=p["reference_id"],
                   dnn_flooring=p["dnn_flooring"], eps=p["eps"])
    M, F, T = X.shape
    m.input, m.n_sources, m.n_channels, m.n_bins, m.n_frames = X, M, M, F, T
    m.demix_filter, m.dnn, m.dnn_output = W.copy(), net, np.ones((M, F, T))
    return m


def raise_to(total, figures):
    for k, v in figures.items():
        total[k] = max(total.get(k, 0.0), float(v))


def state(fx, i):
    M, F, T = fx["X"].shape
    return np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1)) if i == 0 else fx["W_%d" % i]


def probe_fixture(fx):
    X, p = fx["X"], idl.params(fx)
    net = idl.build_net(fx)
    own = {"one_stage": {}, "one_iteration": {}, "whole_run": {}, "scaled_vs_refit": 0.0}
    stage, it, whole = own["one_stage"], own["one_iteration"], own["whole_run"]
    sens32 = f32_sensitive(fx)
    for i in range(1, idl.N_ITER + 1):
        W0, d, Wip, W1 = state(fx, i - 1), fx["d_%d" % i], fx["Wip_%d" % i], fx["W_%d" % i]
        ref_loss = fx["loss"][i]
        # ---- one stage, restated and as the kernels do it
        raise_to(stage, {"inp": idl.d_metric(idl.network_input(X, W0, p["domain"]), fx["inp_%d" % i])})
        assert np.array_equal(idl.source_output(fx["raw_%d" % i], p["domain"], p["dnn_flooring"]), d)
        got_ip = idl.space_update(X, W0, idl.variance(d, p["domain"], p["eps"]))
        raise_to(stage, {"W": idl.w_metric(got_ip, Wip)})
        own["restated_sweep"] = max(own.get("restated_sweep", 0.0), idl.w_metric(got_ip, Wip))
        Y = idl.separate(X, Wip)
        scale = idl.pb_scale(Y, X[p["reference_id"]])
        raise_to(stage, {"scale": idl.out_metric(scale, fx["scale_%d" % i])})
        refit, scaled = idl.normalize_refit(X, Y, scale), idl.normalize_scaled(Wip, fx["scale_%d" % i])
        raise_to(stage, {"W": max(idl.w_metric(refit, W1), idl.w_metric(scaled, W1))})
        own["scaled_vs_refit"] = max(own["scaled_vs_refit"], idl.w_metric(scaled, W1))
        raise_to(stage, {"loss": max(idl.loss_metric(idl.loss(X, W1, d, p["domain"], p["eps"]), ref_loss, X),
                                     idl.loss_metric(idl.kernel_loss(X, W1, d, p["domain"], p["eps"]), ref_loss, X))})
        # ---- one iteration: restatement, kernel model
        for form in ("refit", "scaled"):
            gW, gd, gl = idl.iterate(X, W0, net, form=form, **p)
            if form == "scaled":
                gl = idl.kernel_loss(X, gW, gd, p["domain"], p["eps"])
            raise_to(it, {"W": idl.w_metric(gW, W1), "d": idl.d_metric(gd, d), "loss": idl.loss_metric(gl, ref_loss, X)})
        # ---- sensitivity of the reference, stage by stage (the sweep and the loss) and over the iteration
        for draw in range(N_DRAWS):
            rng = np.random.default_rng(100 * i + draw)
            Xm, Wm = idl.one_ulp(X, rng), idl.one_ulp(W0, rng)
            m = reference_at(fx, Xm, Wm, Moved(net, rng) if sens32 else net)
            m.update_once()
            figures = {"W": idl.w_metric(m.demix_filter, W1), "d": idl.d_metric(m.dnn_output, d),
                       "loss": idl.loss_metric(m.compute_negative_loglikelihood(), ref_loss, X)}
            raise_to(it, figures)
            m = reference_at(fx, Xm, Wm, net)
            m.dnn_output = d.copy()
            m.update_space_model()
            raise_to(stage, {"W": idl.w_metric(m.demix_filter, Wip)})
            m = reference_at(fx, Xm, idl.one_ulp(W1, rng), net)
            m.dnn_output = d.copy()
            raise_to(stage, {"loss": idl.loss_metric(m.compute_negative_loglikelihood(), ref_loss, X),
                             "scale": idl.out_metric(mk.reference()[0].projection_back(
                                 m.separate(Xm, demix_filter=idl.one_ulp(Wip, rng)), reference=Xm[p["reference_id"]]),
                                 fx["scale_%d" % i])})
    # ---- the whole run
    last = idl.N_ITER
    for form in ("refit", "scaled"):
        trace = []
        gW, gd, gl, gout = idl.run(X, net, form=form, trace=trace, **p)
        if form == "scaled":
            gl = np.array([gl[0]] + [idl.kernel_loss(X, t["W"], t["d"], p["domain"], p["eps"]) for t in trace])
        raise_to(whole, {"W": idl.w_metric(gW, fx["W_%d" % last]), "d": idl.d_metric(gd, fx["d_%d" % last]),
                         "loss": idl.loss_metric(gl, fx["loss"], X), "out": idl.out_metric(gout, fx["output"])})
    for draw in range(N_DRAWS):
        rng = np.random.default_rng(7000 + draw)
        m = reference_at(fx, X, state(fx, 0), None)
        out = m(idl.one_ulp(X, rng), iteration=idl.N_ITER, dnn=Moved(net, rng) if sens32 else net)
        raise_to(whole, {"W": idl.w_metric(m.demix_filter, fx["W_%d" % last]), "d": idl.d_metric(m.dnn_output, fx["d_%d" % last]),
                         "loss": idl.loss_metric(np.array(m.loss), fx["loss"], X), "out": idl.out_metric(out, fx["output"])})
    return own


def tolerances(own, sens32, pow_path):
    tol = {}
    for group in ("one_stage", "one_iteration", "whole_run"):
        tol[group] = {}
        for k, v in own[group].items():
            floor = RESOLUTION
            if k in ("inp", "d"):
                floor = 2 * 2.0 ** -23 if (k == "d" and pow_path) else F32_HALF_STEP
            tol[group][k] = FACTOR * max(v, floor)
    tol["scaled_vs_refit"] = own["scaled_vs_refit"]
    return tol


def measure():
    table = {}
    for case in idl.CASES:
        name = case[0]
        fx = np.load(os.path.join(ROOT, "tests", "golden", "idlma", name + ".npz"), allow_pickle=False)
        own = probe_fixture(fx)
        table[name] = tolerances(own, f32_sensitive(fx), float(fx["domain"]) not in (1.0, 2.0))
        print(name, json.dumps(table[name]))
        if FACTOR * own["restated_sweep"] > LIMIT:
            raise SystemExit("%s: the restated sweep is %.3g from the reference's, above %.3g / %d: not the same update"
                             % (name, own["restated_sweep"], LIMIT, FACTOR))
    return {"factor": FACTOR, "n_draws": N_DRAWS, "fixtures": table}


def main():
    got = measure()
    if "--check" in sys.argv[1:]:
        want = json.load(open(OUT))
        same = json.dumps(want, sort_keys=True) == json.dumps(got, sort_keys=True)
        print("tolerances.json:", "reproduced" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
