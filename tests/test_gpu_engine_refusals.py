"""Every array argument of every Engine method of the six factorisation model families (FastMNMF, MNMF, ComplexEUCNMF,
EUCNTF, LDPSDTF, GaussIPSDTA / tIPSDTA) is refused with ValueError BEFORE the library is reached when it has the wrong
dtype, lies on the CPU, is a strided view, or -- a workspace -- is one byte short.

Nothing is launched with a bad argument: while the refusals are tried, the engine's library is a guard that answers the
`*_workspace_bytes` queries and raises AssertionError("reached the library") for every other entry point, so a missing
check is a test failure, not a launch.  The sizes are the smallest legal ones: B = 1, two channels / sources, 4 bins,
8 frames, n_basis 2 (n_blocks 2 for IPSDTA, n_bins 4 for PSDTF)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, F, T, K, NB, N_ITER = 2, 4, 8, 2, 2, 3
C128, F64, I32 = torch.complex128, torch.float64, torch.int32


class LibraryGuard:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return getattr(self._real, name)
        raise AssertionError("reached the library: " + name)


@pytest.fixture(scope="module")
def eng():
    from audio_source_separation_amd.ops import Engine
    return Engine(dtype="float64", device="cuda:0")


def _eye(dev, *lead, n=M, dtype=C128):
    return torch.eye(n, dtype=dtype, device=dev).expand(*lead, n, n).contiguous()


def _family(eng, name):
    """(arrays by name, [(method, positional arguments, keyword arguments)], the loss call of the positive control): a
    str among the arguments names one of the arrays.  The values make a model every kernel accepts."""
    dev = eng.dev
    g = torch.Generator(device=dev).manual_seed(0)

    def pos(*shape):
        return torch.rand(shape, dtype=F64, device=dev, generator=g) + 0.5

    def cplx(*shape):
        return torch.complex(pos(*shape) - 1.0, pos(*shape) - 1.0)

    a = {"status": eng.new_status(1), "loss": eng.empty((1,), dtype=F64)}
    if name == "FastMNMF":
        a.update(X=cplx(1, M, F, T), Q=_eye(dev, 1, F), W=pos(1, M, F, K), H=pos(1, M, K, T), g=pos(1, M, F, M),
                 ws=eng.fastmnmf_workspace(1, M, M, F, T, K), losses=eng.empty((N_ITER + 1, 1), dtype=F64),
                 out=eng.empty((1, M, F, T), dtype=C128))
        model, st = ["X", "Q", "W", "H", "g"], {"status": "status"}
        calls = [("fastmnmf_project", model + ["ws"], {"loss": "loss"}),
                 ("fastmnmf_update_nmf", ["X", "W", "H", "g", "ws"], {}),
                 ("fastmnmf_update_scm", ["X", "W", "H", "g", "ws"], {}),
                 ("fastmnmf_update_diagonalizer_model", model + ["ws"], st),
                 ("fastmnmf_normalize_power", model, {}),
                 ("fastmnmf_separate", model, dict(st, out="out")),
                 ("fastmnmf_iterate", [N_ITER] + model + ["ws"], dict(st, loss="losses"))]
        return a, calls, calls[0]
    if name == "MNMF":
        a.update(X=cplx(1, M, F, T), Tb=pos(1, F, K), V=pos(1, K, T), Z=pos(1, M, K), H=_eye(dev, 1, F, M),
                 ws=eng.mnmf_workspace(1, M, M, F, T, K), losses=eng.empty((N_ITER + 1, 1), dtype=F64),
                 out=eng.empty((1, M, F, T), dtype=C128))
        model, st = ["X", "Tb", "V", "Z", "H"], {"status": "status"}
        calls = [("mnmf_update_" + s, model + ["ws"], st) for s in ("basis", "activation", "latent", "spatial")]
        calls += [("mnmf_loss", model + ["ws"], dict(st, loss="loss")),
                  ("mnmf_separate", model, dict(st, out="out")),
                  ("mnmf_iterate", [N_ITER] + model + ["ws"], dict(st, loss="losses"))]
        return a, calls, calls[4]
    if name == "ComplexEUCNMF":
        a.update(X=cplx(1, F, T), Tb=pos(1, F, K), V=pos(1, K, T), Phi=pos(1, F, K, T), ws=eng.cnmf_workspace(1, F, T, K),
                 losses=eng.empty((N_ITER, 1), dtype=F64), beta=eng.empty((1, F, K, T), dtype=F64),
                 out=eng.empty((1, F, T), dtype=C128))
        model = ["X", "Tb", "V", "Phi", "ws"]
        calls = [("cnmf_update", model, {}),
                 ("cnmf_loss", model, {"loss": "loss"}),
                 ("cnmf_beta", ["Tb", "V"], {"out": "beta"}),
                 ("cnmf_reconstruct", ["Tb", "V", "Phi"], {"out": "out"}),
                 ("cnmf_iterate", [N_ITER] + model, {"loss": "losses"})]
        return a, calls, calls[1]
    if name == "EUCNTF":
        a.update(X=pos(1, M, F, T), Z=pos(1, M, K), Tb=pos(1, F, K), V=pos(1, K, T), ws=eng.ntf_workspace(1, M, F, T, K),
                 losses=eng.empty((N_ITER, 1), dtype=F64), out=eng.empty((1, M, F, T), dtype=F64))
        model = ["X", "Z", "Tb", "V", "ws"]
        calls = [("ntf_update", model, {}),
                 ("ntf_loss", model, {"loss": "loss"}),
                 ("ntf_reconstruct", ["Z", "Tb", "V"], {"out": "out"}),
                 ("ntf_iterate", [N_ITER] + model, {"loss": "losses"})]
        return a, calls, calls[1]
    if name == "LDPSDTF":
        a.update(X=_eye(dev, 1, T, n=F, dtype=F64), V=_eye(dev, 1, K, n=F, dtype=F64), H=pos(1, K, T),
                 A=_eye(dev, 3, n=F, dtype=F64), ws=eng.psdtf_workspace(1, F, T, K),
                 losses=eng.empty((N_ITER, 1), dtype=F64), out=eng.empty((1, T, F, F), dtype=F64))
        st = {"status": "status"}
        calls = [("psdtf_to_psd", ["A"], {}),
                 ("psdtf_update_basis", ["X", "V", "H", "ws"], st),
                 ("psdtf_update_activation", ["X", "V", "H"], st),
                 ("psdtf_normalize", ["V", "H"], {}),
                 ("psdtf_update", ["X", "V", "H", "ws"], st),
                 ("psdtf_loss", ["X", "V", "H", "ws"], dict(st, loss="loss")),
                 ("psdtf_reconstruct", ["V", "H"], {"out": "out"}),
                 ("psdtf_iterate", [N_ITER, "X", "V", "H", "ws"], dict(st, loss="losses"))]
        return a, calls, calls[5]
    pre, nu = {"GaussIPSDTA": ("ipsdta_", {}), "tIPSDTA": ("tipsdta_", {"nu": 4.0})}[name]
    blocks = _eye(dev, M, K, NB, n=F // NB)  # the packed basis: each source's and basis' nb x nb blocks end to end
    a.update(X=cplx(M, F, T), W=_eye(dev, F), U=blocks.reshape(M, K, eng.ipsdta_packed_size(F, NB)).contiguous(),
             H=pos(M, K, T), A=_eye(dev, 3), ws=getattr(eng, pre + "workspace")(M, F, T, K, NB, *nu.values()),
             losses=eng.empty((N_ITER,), dtype=F64))
    model, st = ["X", "W", "U", "H", "ws", NB], dict(nu, status="status")
    calls = [(pre + "update_" + s, model, st) for s in ("basis", "activation", "source", "spatial")]
    calls += [(pre + "loss", model, dict(st, loss="loss")),
              (pre + "iterate", [N_ITER, 1] + model, dict(st, loss="losses"))]
    if name == "GaussIPSDTA":
        calls += [("ipsdta_to_psd", ["A"], {}), ("ipsdta_normalize", ["U", "H", F, NB], {})]
    return a, calls, calls[4]


def _wrong(key, t):
    """`t` made wrong in one way at a time."""
    other = {F64: torch.float32, C128: torch.complex64, I32: torch.int64, torch.uint8: torch.int8}[t.dtype]
    yield "dtype", t.to(other)
    yield "on the CPU", t.cpu()
    if t.numel() > 1:  # the same shape, every second element of a buffer twice as large
        yield "strided", torch.empty(tuple(t.shape) + (2,), dtype=t.dtype, device=t.device)[..., 0]
    else:  # one element is always contiguous: two strided ones (enough where a minimum count is asked for)
        yield "strided", torch.empty((2, 2), dtype=t.dtype, device=t.device)[:, 0]
    if key == "ws":
        yield "one byte short", t[:-1]


def _resolve(arrays, args, kwargs):
    return ([arrays[v] if isinstance(v, str) else v for v in args],
            {k: arrays[v] if isinstance(v, str) else v for k, v in kwargs.items()})


FAMILIES = ("FastMNMF", "MNMF", "ComplexEUCNMF", "EUCNTF", "LDPSDTF", "GaussIPSDTA", "tIPSDTA")


@pytest.mark.parametrize("family", FAMILIES)
def test_every_wrong_array_is_refused_before_the_library(eng, family):
    arrays, calls, _ = _family(eng, family)
    wrong = {key: list(_wrong(key, t)) for key, t in arrays.items()}
    assert wrong["ws"][1][1].dtype == torch.uint8 and not wrong["ws"][1][1].is_cuda  # "a uint8 workspace on the CPU"
    assert all(not w[2][1].is_contiguous() for w in wrong.values())
    real, tried = eng._L, 0
    eng._L = LibraryGuard(real)
    try:
        for method, args, kwargs in calls:
            good_args, good_kwargs = _resolve(arrays, args, kwargs)
            with pytest.raises(AssertionError, match="reached the library"):  # the arrays are right: only the guard stops it
                getattr(eng, method)(*good_args, **good_kwargs)
            slots = [(i, v) for i, v in enumerate(args) if isinstance(v, str)]
            slots += [(k, v) for k, v in kwargs.items() if isinstance(v, str)]
            for slot, key in slots:
                for how, bad in wrong[key]:
                    a, kw = list(good_args), dict(good_kwargs)
                    if isinstance(slot, int):
                        a[slot] = bad
                    else:
                        kw[slot] = bad
                    with pytest.raises(ValueError):
                        getattr(eng, method)(*a, **kw)
                        pytest.fail("%s accepted %s %s" % (method, key, how))
                    tried += 1
    finally:
        eng._L = real
    assert tried >= 3 * sum(len([v for v in list(c[1]) + list(c[2].values()) if isinstance(v, str)]) for c in calls)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_correct_loss_call_goes_through(eng, family):
    arrays, _, (method, args, kwargs) = _family(eng, family)
    a, kw = _resolve(arrays, args, kwargs)
    loss = getattr(eng, method)(*a, **kw)
    assert loss is arrays["loss"] and bool(torch.isfinite(loss).all())
