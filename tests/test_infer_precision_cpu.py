"""The precision argument of the inference runner (unidefense_amd/infer.py): what is refused before any GPU work."""
import pytest

from unidefense_amd.infer import PRECISIONS, InferenceRunner, inference_runner


def _res(name):
    from unidefense_amd.model import load_model
    return load_model(name)(num_classes=2, drop_rate=0.5).eval()


def test_precisions():
    assert PRECISIONS == ("fp32", "fp16")


@pytest.mark.parametrize("name", ["UDR18", "UDR50"])
def test_fp16_refused_for_the_resnet_variants(name):
    m = _res(name)
    for make in (lambda: InferenceRunner(m, 2, 256, "fp16"), lambda: m.inference_runner(2, 256, "fp16"),
                 lambda: inference_runner(m, 2, 256, precision="fp16")):
        with pytest.raises(ValueError, match=type(m).__name__):
            make()
    assert not m.__dict__.get("_ud_runners")


@pytest.mark.parametrize("precision", ["bf16", "fp8", "FP16", "half", None])
def test_unknown_precision_refused(precision):
    m = _res("UDR18")
    with pytest.raises(ValueError, match="precision"):
        InferenceRunner(m, 2, 256, precision)
    with pytest.raises(ValueError, match="precision"):
        m.inference_runner(2, 256, precision)
