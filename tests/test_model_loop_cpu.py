"""The model classes without a GPU: the one rule that sends a loop to the library's one-call `*_iterate` entry
(DeviceState._fast_loop_ok) for every public model class that has such a loop, and the refusals of
their `_reset` that run before a device is touched.  No Engine is created: a loop-rule case only constructs the model, a
refusal case raises before the first upload.  Every expected message is a literal of this file."""
import numpy as np
import pytest

from audio_source_separation_amd._loss import LazyLossList
from audio_source_separation_amd._state import DeviceState
from audio_source_separation_amd.algorithm import nmf, ntf, psdtf
from audio_source_separation_amd.bss import ilrma, ipsdta, iva, mnmf

# (class, constructor keywords): every public model class with a one-call loop
MODELS = [(nmf.EUCNMF, {}), (nmf.KLNMF, {}), (nmf.ISNMF, {}), (nmf.tNMF, {}), (nmf.CauchyNMF, dict(n_basis=2)),
          (nmf.ComplexEUCNMF, {}), (nmf.MultichannelISNMF, {}), (ntf.EUCNTF, dict(n_basis=2)), (psdtf.LDPSDTF, {}),
          (mnmf.FastMultichannelISNMF, {}), (mnmf.MultichannelISNMF, {}), (ilrma.GaussILRMA, {}),
          (iva.AuxLaplaceIVA, {}), (iva.AuxGaussIVA, {}), (ipsdta.GaussIPSDTA, {}), (ipsdta.tIPSDTA, {})]
IDS = ["%s.%s" % (c.__module__.rsplit(".", 1)[-1], c.__name__) for c, _ in MODELS]
WITH_CALLBACKS = [(c, kw) for c, kw in MODELS if "callbacks" in c.__init__.__code__.co_varnames]
WITH_RECORDABLE_LOSS = [(c, kw) for c, kw in MODELS if "recordable_loss" in c.__init__.__code__.co_varnames]
ILRMA_NORMALIZATIONS = [(False, dict(normalize=0, pb_exponent=2.0)), ('power', dict(normalize=1, pb_exponent=2.0)),
                        ('projection-back', dict(normalize=2, pb_exponent=2.0))]


def owner_of(cls):
    return next(c for c in cls.__mro__ if "_OWN_STEPS" in vars(c))


def ids_of(models):
    return [IDS[MODELS.index(m)] for m in models]


def says_yes(model):
    """the rule's answer; for GaussILRMA the plan its __call__ asks for has to agree"""
    ok = model._fast_loop_ok()
    if isinstance(model, ilrma.GaussILRMA):
        assert (model._fast_loop_plan() is not None) == ok
    return ok


def test_the_table_covers_every_family():
    assert len(WITH_CALLBACKS) == 7 and len(WITH_RECORDABLE_LOSS) == 15
    assert {owner_of(c) for c, _ in MODELS} == {
        nmf.EUCNMF, nmf.KLNMF, nmf.ISNMF, nmf.tNMF, nmf.CauchyNMF, nmf.ComplexEUCNMF, nmf.MultichannelISNMF, ntf.EUCNTF,
        psdtf.LDPSDTF, mnmf.FastMultichannelISNMF, mnmf.MultichannelISNMF, ilrma.GaussILRMA, iva.AuxIVAbase,
        ipsdta._BlockDiagonalIPSDTA}
    # one statement of the rule: a model that has conditions of its own adds them to DeviceState's
    own = {c for c, _ in MODELS if any("_fast_loop_ok" in vars(k) for k in c.__mro__ if k is not DeviceState)}
    assert own == {psdtf.LDPSDTF, mnmf.FastMultichannelISNMF, iva.AuxLaplaceIVA, iva.AuxGaussIVA}


@pytest.mark.parametrize("cls,kw", MODELS, ids=IDS)
def test_a_fresh_model_takes_the_one_call_loop(cls, kw):
    model = cls(**kw)
    assert isinstance(model.loss, LazyLossList)
    assert model._fast_loop_ok() is True


@pytest.mark.parametrize("normalize,plan", ILRMA_NORMALIZATIONS)
def test_gauss_ilrma_plans_every_normalisation_the_entry_point_knows(normalize, plan):
    assert ilrma.GaussILRMA(normalize=normalize)._fast_loop_plan() == plan
    assert ilrma.GaussILRMA(normalize=normalize, recordable_loss=False)._fast_loop_plan() == plan
    assert ilrma.GaussILRMA(normalize=normalize, partitioning=True)._fast_loop_plan() is None
    assert ilrma.GaussILRMA(normalize=normalize, callbacks=lambda m: None)._fast_loop_plan() is None


def test_gauss_ilrma_plan_keeps_its_own_conditions():
    assert ilrma.GaussILRMA(power_statistic='direct')._fast_loop_plan() is None
    assert ilrma.GaussILRMA(normalize='nope')._fast_loop_plan() is None
    assert ilrma.GaussILRMA(normalize='projection-back', domain=1)._fast_loop_plan() == dict(normalize=2, pb_exponent=1.0)


@pytest.mark.parametrize("cls,kw", MODELS, ids=IDS)
def test_every_own_step_is_an_attribute_of_the_class(cls, kw):
    steps = owner_of(cls)._OWN_STEPS
    assert len(steps) >= 3 and len(set(steps)) == len(steps)
    for name in steps:
        assert callable(getattr(cls, name)), name


def test_the_nmf_classes_name_every_routed_step():
    base = ("update", "update_once", "_record_loss")
    assert set(nmf.EUCNMF._OWN_STEPS) == set(base + ("update_once_mm",))
    assert set(nmf.KLNMF._OWN_STEPS) == set(base + ("update_once_mm",))
    assert set(nmf.ISNMF._OWN_STEPS) == set(base + ("update_once_mm", "update_once_me"))
    assert set(nmf.tNMF._OWN_STEPS) == set(base + ("update_once_mm",))
    assert set(nmf.CauchyNMF._OWN_STEPS) == set(base + ("update_once_naive", "update_once_mm", "update_once_me",
                                                        "update_once_mm_fast"))
    for cls in (nmf.EUCNMF, nmf.KLNMF, nmf.ISNMF, nmf.tNMF, nmf.CauchyNMF):  # none that the class defines is left out
        assert {n for n in vars(cls) if n.startswith("update_once")} <= set(cls._OWN_STEPS)


@pytest.mark.parametrize("cls,kw", MODELS, ids=IDS)
def test_overriding_any_one_step_keeps_the_python_loop(cls, kw):
    for name in owner_of(cls)._OWN_STEPS:
        sub = type("Sub", (cls,), {name: lambda self, *args, **kwargs: None})
        assert says_yes(sub(**kw)) is False, name
    # a subclass that overrides none of them keeps the one-call loop, and so does one more level of it
    plain = type("Plain", (cls,), {"something_else": lambda self: None})
    assert says_yes(plain(**kw)) is True
    assert says_yes(type("Deeper", (plain,), {})(**kw)) is True


@pytest.mark.parametrize("cls,kw", WITH_CALLBACKS, ids=ids_of(WITH_CALLBACKS))
def test_callbacks_keep_the_python_loop(cls, kw):
    assert says_yes(cls(callbacks=[lambda model: None], **kw)) is False
    assert says_yes(cls(callbacks=lambda model: None, **kw)) is False
    model = cls(**kw)
    model.callbacks = [lambda model: None]  # assigned later, as the keywords of a call do
    assert says_yes(model) is False


@pytest.mark.parametrize("cls,kw", MODELS, ids=IDS)
def test_a_plain_list_as_loss_keeps_the_python_loop_while_losses_are_recorded(cls, kw):
    model = cls(**kw)
    model.loss = []
    assert says_yes(model) is False
    model.loss = LazyLossList()
    assert says_yes(model) is True


@pytest.mark.parametrize("cls,kw", WITH_RECORDABLE_LOSS, ids=ids_of(WITH_RECORDABLE_LOSS))
def test_a_plain_list_as_loss_does_not_matter_when_nothing_is_recorded(cls, kw):
    model = cls(recordable_loss=False, **kw)
    assert says_yes(model) is True
    model.loss = []
    assert says_yes(model) is True


def test_the_models_own_conditions_are_added_to_the_rule():
    assert psdtf.LDPSDTF(algorithm='em')._fast_loop_ok() is False
    assert mnmf.FastMultichannelISNMF(partitioning=True)._fast_loop_ok() is False
    assert mnmf.FastMultichannelISNMF(normalize='projection-back')._fast_loop_ok() is False
    assert mnmf.FastMultichannelISNMF(normalize=False)._fast_loop_ok() is True
    assert iva.AuxIVAbase()._fast_loop_ok() is False  # no _KIND: no kernels
    assert iva.AuxLaplaceIVA(algorithm_spatial='IPA')._fast_loop_ok() is False
    for spatial in ('IP', 'IP1', 'ISS', 'pairwise', 'IP2'):
        assert iva.AuxLaplaceIVA(algorithm_spatial=spatial)._fast_loop_ok() is True


# ---- refusals before a device is touched ---------------------------------------------------------------------------
FLOAT64_ONLY = [(nmf.ComplexEUCNMF, {}, True), (nmf.MultichannelISNMF, {}, True), (ntf.EUCNTF, dict(n_basis=2), False),
                (psdtf.LDPSDTF, {}, False), (ipsdta.GaussIPSDTA, {}, False), (ipsdta.tIPSDTA, {}, False),
                (mnmf.MultichannelISNMF, {}, True)]


@pytest.mark.parametrize("cls,kw,complex_ok", FLOAT64_ONLY, ids=[IDS[[c for c, _ in MODELS].index(c)] for c, _, _ in FLOAT64_ONLY])
def test_float64_only(cls, kw, complex_ok):
    with pytest.raises(ValueError) as e:
        cls(dtype='float32', **kw)
    assert str(e.value) == "{} supports float64 only, got dtype='float32'".format(cls.__name__)
    for dtype in ('float64', 'double') + (('complex128',) if complex_ok else ()):
        assert cls(dtype=dtype, **kw).dtype == 'float64'
    if not complex_ok:
        with pytest.raises(ValueError) as e:
            cls(dtype='complex128', **kw)
        assert str(e.value) == "{} supports float64 only, got dtype='complex128'".format(cls.__name__)


def test_float64_only_names_the_model_not_a_subclass_of_sawadas_mnmf():
    class Mine(mnmf.MultichannelISNMF):
        pass

    with pytest.raises(ValueError) as e:
        Mine(dtype='float32')
    assert str(e.value) == "MultichannelISNMF supports float64 only, got dtype='float32'"


def hermitian(F, T, M):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((F, T, M, M)) + 1j * rng.standard_normal((F, T, M, M))
    return A @ A.conj().swapaxes(-1, -2) + np.eye(M)


def symmetric(M, T):
    rng = np.random.default_rng(1)
    A = rng.standard_normal((T, M, M))
    return np.ascontiguousarray((A @ A.swapaxes(-1, -2) + np.eye(M)).transpose(1, 2, 0))


def mixture(M, F, T):
    rng = np.random.default_rng(2)
    return rng.standard_normal((M, F, T)) + 1j * rng.standard_normal((M, F, T))


# (constructor, a target that passes every refusal but the one under test)
N_BASIS_CASES = [(lambda n: nmf.ComplexEUCNMF(n_basis=n), mixture(1, 4, 5)[0]),
                 (lambda n: nmf.MultichannelISNMF(n_basis=n), hermitian(3, 4, 2)),
                 (lambda n: ntf.EUCNTF(n_basis=n), np.ones((2, 3, 4))),
                 (lambda n: psdtf.LDPSDTF(n_basis=n), symmetric(3, 4)),
                 (lambda n: ipsdta.GaussIPSDTA(n_basis=n, n_blocks=2), mixture(2, 4, 5)),
                 (lambda n: ipsdta.tIPSDTA(n_basis=n, n_blocks=2), mixture(2, 4, 5))]


@pytest.mark.parametrize("make,target", N_BASIS_CASES,
                         ids=["ComplexEUCNMF", "covariance-MultichannelISNMF", "EUCNTF", "LDPSDTF", "GaussIPSDTA", "tIPSDTA"])
@pytest.mark.parametrize("n_basis,shown", [(0, "0"), (65, "65"), (-1, "-1"), (2.0, "2.0"), ("2", "'2'"), (None, "None")])
def test_n_basis_out_of_range_or_not_an_int(make, target, n_basis, shown):
    with pytest.raises(ValueError) as e:
        make(n_basis)(target, iteration=1)
    assert str(e.value) == "n_basis must be an int in [1, 64], got " + shown


def raises(model, target, message, **kwargs):
    with pytest.raises(ValueError) as e:
        model(target, iteration=1, **kwargs)
    assert str(e.value) == message
    assert model._engine is None  # refused before a device was touched


def test_wrong_number_of_dims():
    raises(nmf.ComplexEUCNMF(), np.ones(4, dtype=complex), "target must be (n_bins, n_frames), got 1 dims")
    raises(nmf.ComplexEUCNMF(), np.ones((2, 2, 3, 4), dtype=complex), "target must be (n_bins, n_frames), got 4 dims")
    raises(nmf.MultichannelISNMF(), hermitian(3, 4, 2)[0],
           "target must be (n_bins, n_frames, n_channels, n_channels), got 3 dims")
    raises(ntf.EUCNTF(n_basis=2), np.ones((3, 4)), "target must be (n_channels, n_bins, n_frames), got 2 dims")
    raises(ntf.EUCNTF(n_basis=2), np.ones((1, 1, 2, 3, 4)), "target must be (n_channels, n_bins, n_frames), got 5 dims")
    raises(psdtf.LDPSDTF(), np.ones((3, 3)), "target must be (n_bins, n_bins, n_frames), got 2 dims")
    for cls in (ipsdta.GaussIPSDTA, ipsdta.tIPSDTA):
        raises(cls(), mixture(2, 4, 5)[None], "input must be (n_channels, n_bins, n_frames), got 4 dims")
    for cls in (mnmf.FastMultichannelISNMF, mnmf.MultichannelISNMF):
        raises(cls(), mixture(2, 4, 5)[0], "input must be (n_channels, n_bins, n_frames), got 2 dims")
        raises(cls(), mixture(2, 4, 5)[None, None], "input must be (n_channels, n_bins, n_frames), got 5 dims")


def test_empty_target():
    raises(nmf.MultichannelISNMF(), np.zeros((0, 4, 2, 2), dtype=complex), "target must not be empty, got shape (0, 4, 2, 2)")
    raises(nmf.MultichannelISNMF(), np.zeros((3, 0, 2, 2), dtype=complex), "target must not be empty, got shape (3, 0, 2, 2)")
    raises(ntf.EUCNTF(n_basis=2), np.zeros((2, 0, 4)), "target must not be empty, got shape (2, 0, 4)")
    raises(ntf.EUCNTF(n_basis=2), np.zeros((2, 3, 0)), "target must not be empty, got shape (2, 3, 0)")
    raises(ntf.EUCNTF(n_basis=2), np.zeros((0, 2, 3, 4)), "target must not be empty, got shape (0, 2, 3, 4)")
    raises(psdtf.LDPSDTF(), np.zeros((3, 3, 0)), "target must not be empty, got shape (3, 3, 0)")
    raises(psdtf.LDPSDTF(), np.zeros((0, 3, 3, 4)), "target must not be empty, got shape (0, 3, 3, 4)")
    for cls in (ipsdta.GaussIPSDTA, ipsdta.tIPSDTA):
        raises(cls(), np.zeros((2, 0, 5), dtype=complex), "input must not be empty, got shape (2, 0, 5)")
        raises(cls(), np.zeros((2, 4, 0), dtype=complex), "input must not be empty, got shape (2, 4, 0)")


def test_non_square_target():
    raises(nmf.MultichannelISNMF(), np.ones((3, 4, 2, 3), dtype=complex),
           "target must be square in its last two axes, got shape (3, 4, 2, 3)")
    raises(psdtf.LDPSDTF(), np.ones((3, 2, 4)), "target must be square in its first two axes, got shape (3, 2, 4)")


def test_real_where_complex_is_required_and_the_reverse():
    raises(nmf.MultichannelISNMF(), hermitian(3, 4, 2).real, "MultichannelISNMF supports complex targets only")
    raises(psdtf.LDPSDTF(), symmetric(3, 4).astype(complex), "LDPSDTF supports real targets only")
    raises(ipsdta.GaussIPSDTA(), mixture(2, 4, 5).real, "GaussIPSDTA needs a complex input (n_channels, n_bins, n_frames)")
    raises(ipsdta.tIPSDTA(), mixture(2, 4, 5).real, "tIPSDTA needs a complex input (n_channels, n_bins, n_frames)")


def test_the_order_of_refusals_is_each_models_own():
    # doubly wrong calls: which error comes first is part of the interface
    raises(nmf.MultichannelISNMF(n_basis=0), hermitian(3, 4, 2).real, "n_basis must be an int in [1, 64], got 0")
    raises(nmf.MultichannelISNMF(), np.ones((3, 4, 2)), "MultichannelISNMF supports complex targets only")
    raises(psdtf.LDPSDTF(n_basis=0), np.ones((3, 2, 4), dtype=complex), "n_basis must be an int in [1, 64], got 0")
    raises(psdtf.LDPSDTF(), np.ones((3, 2, 4), dtype=complex), "LDPSDTF supports real targets only")
    raises(ntf.EUCNTF(n_basis=0), np.ones((3, 4)), "n_basis must be an int in [1, 64], got 0")
    raises(nmf.ComplexEUCNMF(n_basis=0), np.ones(4, dtype=complex), "n_basis must be an int in [1, 64], got 0")
    for cls in (ipsdta.GaussIPSDTA, ipsdta.tIPSDTA):
        raises(cls(n_basis=0), mixture(2, 4, 5).real, "%s needs a complex input (n_channels, n_bins, n_frames)" % cls.__name__)
        raises(cls(n_basis=0), np.zeros((2, 0, 5), dtype=complex), "input must not be empty, got shape (2, 0, 5)")
        raises(cls(n_basis=0, n_blocks=0), mixture(2, 4, 5), "n_basis must be an int in [1, 64], got 0")
        raises(cls(n_blocks=0), mixture(2, 4, 5), "n_blocks must be an int in [1, n_bins = 4], got 0")


def test_warm_start_arrays_of_the_wrong_shape_or_kind():
    X = hermitian(3, 4, 2)  # n_bins 3, n_frames 4, n_channels 2; n_basis 5
    new = lambda: nmf.MultichannelISNMF(n_basis=5)  # noqa: E731
    raises(new(), X, "spatial has shape (3, 5, 2, 3), the target needs (3, 5, 2, 2)", spatial=np.ones((3, 5, 2, 3), dtype=complex))
    raises(new(), X, "basis has shape (5, 3), the target needs (3, 5)", basis=np.ones((5, 3)))
    raises(new(), X, "activation has shape (5, 5), the target needs (5, 4)", activation=np.ones((5, 5)))
    raises(new(), X, "MultichannelISNMF supports a real basis only", basis=np.ones((3, 5), dtype=complex))
    raises(new(), X, "MultichannelISNMF supports a real activation only", activation=np.ones((5, 5), dtype=complex))
    # attribute by attribute: a wrong spatial before a complex basis, the kind of an array before its shape
    raises(new(), X, "spatial has shape (1,), the target needs (3, 5, 2, 2)", spatial=np.ones(1), basis=np.ones((3, 5), dtype=complex))
    raises(new(), X, "MultichannelISNMF supports a real basis only", basis=np.ones(1, dtype=complex), activation=np.ones(1))

    S = symmetric(3, 4)  # n_bins 3, n_frames 4; n_basis 2
    raises(psdtf.LDPSDTF(), S, "basis has shape (3, 3, 5), the target needs (3, 3, 2)", basis=np.ones((3, 3, 5)))
    raises(psdtf.LDPSDTF(), S, "activation has shape (2, 5), the target needs (2, 4)", activation=np.ones((2, 5)))
    raises(psdtf.LDPSDTF(), S, "LDPSDTF supports a real basis only", basis=np.ones((3, 3, 2), dtype=complex))
    raises(psdtf.LDPSDTF(), S, "LDPSDTF supports a real activation only", activation=np.ones((2, 4), dtype=complex))
    skew = np.ones((3, 3, 2))
    skew[0, 1, 0] = 2.0
    raises(psdtf.LDPSDTF(), S, "LDPSDTF supports symmetric bases only", basis=skew, activation=np.ones((2, 5)))
    Sb = np.stack([S, S])  # a batched target needs the leading axis on the warm start too
    raises(psdtf.LDPSDTF(), Sb, "basis has shape (3, 3, 2), the target needs (2, 3, 3, 2)", basis=np.ones((3, 3, 2)))


def test_keep_or_draw_draws_only_what_is_absent():
    class Model(DeviceState):
        pass

    m, drawn = Model(), []

    def draw():
        drawn.append(1)
        return np.arange(3)

    m._keep_or_draw("a", draw)
    assert drawn == [1] and np.array_equal(m.a, [0, 1, 2])
    kept = m.a
    m._keep_or_draw("a", draw)
    assert drawn == [1] and m.a is kept
    m._keep_or_draw("a", draw, np.float64)  # a copy of the wanted type, still no draw
    assert drawn == [1] and m.a is not kept and m.a.dtype == np.float64 and np.array_equal(m.a, kept)
