"""The two argument checks every factorisation-model call of Engine goes through (ops.check_array,
ops.check_workspace), on small host tensors: CPU stands for "the engine's device", a `meta` tensor for "another
device".  Every refusal is a ValueError that names the model and the argument."""
import pytest
import torch

from audio_source_separation_amd.ops import check_array, check_workspace

CPU = torch.device("cpu")


def refused(*args, **kwargs):
    with pytest.raises(ValueError) as e:
        check_array("EUCNTF", "activation", *args, **kwargs)
    assert "EUCNTF" in str(e.value) and "activation" in str(e.value)
    return str(e.value)


@pytest.mark.parametrize("form", [dict(shape=(2, 3, 4)), dict(numel=24)])
def test_array_dtype_device_and_contiguity_in_both_forms(form):
    good = torch.zeros((2, 3, 4), dtype=torch.float64)
    check_array("EUCNTF", "activation", good, torch.float64, CPU, **form)
    assert "float32" in refused(good.float(), torch.float64, CPU, **form)
    assert "int64" in refused(torch.zeros((2, 3, 4), dtype=torch.int64), torch.int32, CPU, **form)
    assert "complex128" in refused(good.to(torch.complex128), torch.float64, CPU, **form)
    assert "meta" in refused(torch.zeros((2, 3, 4), dtype=torch.float64, device="meta"), torch.float64, CPU, **form)
    transposed = torch.zeros((2, 4, 3), dtype=torch.float64).transpose(1, 2)
    assert tuple(transposed.shape) == (2, 3, 4) and not transposed.is_contiguous()
    assert "contiguous" in refused(transposed, torch.float64, CPU, **form)
    strided = torch.zeros((2, 3, 8), dtype=torch.float64)[..., ::2]
    assert "contiguous" in refused(strided, torch.float64, CPU, **form)


def test_array_exact_shape():
    a = torch.zeros((2, 3, 4), dtype=torch.float64)
    for shape in ((2, 3, 5), (2, 3), (2, 3, 4, 1), (24,), (4, 3, 2)):
        assert "shape" in refused(a, torch.float64, CPU, shape=shape)
    check_array("EUCNTF", "activation", a, torch.float64, CPU, shape=torch.Size((2, 3, 4)))
    check_array("EUCNTF", "activation", torch.zeros((0, 3), dtype=torch.float64), torch.float64, CPU, shape=(0, 3))


def test_array_minimum_count():
    status = torch.zeros(4, dtype=torch.int32)
    check_array("MNMF", "status", status, torch.int32, CPU, numel=4)
    check_array("MNMF", "status", status, torch.int32, CPU, numel=3)        # a larger flat buffer
    check_array("MNMF", "status", status.reshape(2, 2), torch.int32, CPU, numel=4)  # any shape
    check_array("MNMF", "status", torch.zeros((3, 2), dtype=torch.int32)[1], torch.int32, CPU, numel=2)  # a row of a block
    with pytest.raises(ValueError) as e:
        check_array("MNMF", "status", status, torch.int32, CPU, numel=5)
    assert "MNMF" in str(e.value) and "status" in str(e.value) and "5" in str(e.value)
    with pytest.raises(ValueError):
        check_array("MNMF", "status", torch.zeros(0, dtype=torch.int32), torch.int32, CPU, numel=1)


def test_workspace():
    ws = torch.zeros(64, dtype=torch.uint8)
    check_workspace("LDPSDTF", ws, CPU, 64)   # exactly the needed size
    check_workspace("LDPSDTF", ws, CPU, 1)
    bad = {"one byte short": (ws[:63], 64),
           "not uint8": (torch.zeros(64, dtype=torch.int8), 64),
           "float64 of the same byte count": (torch.zeros(8, dtype=torch.float64), 64),
           "strided": (torch.zeros(128, dtype=torch.uint8)[::2], 64),
           "another device": (torch.zeros(64, dtype=torch.uint8, device="meta"), 64),
           "sizes outside the envelope": (ws, 0)}
    for what, (w, need) in bad.items():
        with pytest.raises(ValueError) as e:
            check_workspace("LDPSDTF", w, CPU, need)
        assert "LDPSDTF" in str(e.value) and "workspace" in str(e.value), what
