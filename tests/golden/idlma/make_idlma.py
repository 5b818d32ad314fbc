#!/usr/bin/env python3
"""Generate the GaussIDLMA fixtures by running the *reference* itself on the CPU (src/sss/idlma.py of the reference tree,
ASSX_REFERENCE_SRC).  Everything written is data: the seeded mixture, the stored arrays of the test network
(tests/idlma_np.py) and what the reference computed in N_ITER iterations.

    python tests/golden/idlma/make_idlma.py            # rewrites tests/golden/idlma/*.npz
    python tests/golden/idlma/make_idlma.py --verify   # regenerates in memory and compares every array bit for bit

The reference's IP update hands numpy.linalg.solve a stack of vectors, which NumPy 2 reads as a matrix: the call is wrapped
with NumPy 1 semantics, as tests/golden/make_golden.py does.

Recorded for every iteration i: inp_i (the network's float32 input), raw_i (its output), d_i (dnn_output), Wip_i (W after
the sweep), scale_i, W_i (after normalisation); the list `loss`, the front door's `output`.  Asserted here: no NumPy warning,
every value finite, cond(W U_n) < 1e6 at every IP step, every dtype, the front door equal to the stepwise run bit for bit.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import idlma_np as idl  # noqa: E402

REFERENCE_SRC = os.environ.get("ASSX_REFERENCE_SRC", "/root/reference/src")
COND_LIMIT = 1e6
EPS = 1e-12
DNN_FLOORING = 1e-5

_orig_solve, _orig_cond = np.linalg.solve, np.linalg.cond


def _solve_numpy1(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if b.ndim == a.ndim - 1:
        return _orig_solve(a, b[..., None])[..., 0]
    return _orig_solve(a, b)


def reference():
    """(module, GaussIDLMA) of the reference with the solve wrapper in place."""
    np.linalg.solve = _solve_numpy1
    if REFERENCE_SRC not in sys.path:
        sys.path.insert(0, REFERENCE_SRC)
    import sss.idlma as mod
    return mod, mod.GaussIDLMA


class Recorder(torch.nn.Module):
    """the network with its inputs and outputs kept"""

    def __init__(self, net):
        super().__init__()
        self.net, self.inputs, self.outputs = net, [], []

    def forward(self, x):
        y = self.net(x)
        self.inputs.append(x.numpy().copy())
        self.outputs.append(y.numpy().copy())
        return y


def new_model(case_opts, domain):
    _, GaussIDLMA = reference()
    return GaussIDLMA(domain=domain, normalize='projection-back', reference_id=case_opts.get("reference_id", 0),
                      dnn_flooring=case_opts.get("dnn_flooring", DNN_FLOORING), eps=EPS)


def make_case(name, M, F, T, domain, kind, seed, opts):
    mod, _ = reference()
    X = idl.convolutive_mixture(M, F, T, seed)
    net_arrays = idl.draw_net(kind, M, F, T, seed, zero_g=opts.get("zero_g", False))
    net = Recorder(idl.build_net(net_arrays))
    conds, scales = [], []

    def cond(a, *args, **kwargs):
        c = _orig_cond(a, *args, **kwargs)
        conds.append(float(np.max(c)))
        return c

    orig_pb = mod.projection_back

    def pb(Y, reference):
        s = orig_pb(Y, reference=reference)
        scales.append(np.array(s))
        return s

    rec = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        np.linalg.cond, mod.projection_back = cond, pb
        try:
            # stepwise, as the reference's __call__ drives it
            m = new_model(opts, domain)
            m.input = X
            m._reset(dnn=net)
            losses = [m.compute_negative_loglikelihood()]
            sweep = m.update_space_model

            def update_space_model():
                sweep()
                rec["Wip_%d" % len(losses)] = m.demix_filter.copy()

            m.update_space_model = update_space_model
            for i in range(1, idl.N_ITER + 1):
                m.update_once()
                rec["inp_%d" % i], rec["raw_%d" % i] = net.inputs[-1], net.outputs[-1]
                rec["d_%d" % i], rec["scale_%d" % i], rec["W_%d" % i] = m.dnn_output.copy(), scales[-1], m.demix_filter.copy()
                assert m.dnn_output.dtype == np.float32 and net.inputs[-1].dtype == np.float32
                losses.append(m.compute_negative_loglikelihood())
            # the front door
            front = new_model(opts, domain)
            out = front(X, iteration=idl.N_ITER, dnn=Recorder(idl.build_net(net_arrays)))
        finally:
            np.linalg.cond, mod.projection_back = _orig_cond, orig_pb
    assert np.array_equal(front.demix_filter, m.demix_filter) and np.array_equal(front.dnn_output, m.dnn_output), name
    assert np.array_equal(np.array(front.loss), np.array(losses)), name
    assert max(conds) < COND_LIMIT, (name, max(conds))
    assert len(conds) == 2 * idl.N_ITER * M
    rec.update(net_arrays)
    rec.update(X=X, loss=np.array(losses, dtype=np.float64), output=out, domain=np.float64(domain), eps=np.float64(EPS),
               dnn_flooring=np.float64(opts.get("dnn_flooring", DNN_FLOORING)),
               reference_id=np.int64(opts.get("reference_id", 0)), max_cond=np.float64(max(conds)),
               versions=np.array("numpy=%s torch=%s" % (np.__version__, torch.__version__.split("+")[0])))
    for k, v in rec.items():
        if k != "versions":
            assert np.all(np.isfinite(v)), (name, k)
    assert out.dtype == np.complex128 and rec["W_1"].dtype == np.complex128 and rec["loss"].dtype == np.float64
    if opts.get("zero_g"):  # the floor the case is there for is met
        floor = np.float32(rec["dnn_flooring"]) if rec["dnn_flooring"] else np.float32(0.0)
        assert np.sum(rec["d_1"] == floor) >= M + 2, name
    return rec


def main():
    verify = "--verify" in sys.argv[1:]
    torch.manual_seed(0)
    bad = 0
    for case in idl.CASES:
        rec = make_case(*case)
        path = os.path.join(HERE, case[0] + ".npz")
        if verify:
            old = np.load(path, allow_pickle=False)
            same = sorted(old.files) == sorted(rec) and all(
                np.array_equal(old[k], rec[k]) for k in rec if k != "versions")
            print("%-34s %s" % (case[0], "identical" if same else "DIFFERENT"))
            bad += not same
        else:
            np.savez_compressed(path, **rec)
            print("%-34s %7d bytes, max cond %.1f" % (case[0], os.path.getsize(path), float(rec["max_cond"])))
            assert os.path.getsize(path) < 1 << 20
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
