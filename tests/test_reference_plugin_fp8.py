"""reference_plugin.register() and the FP8 strategy: by default the FP8 slot is left to the factory's own strategies, replace_fp8=True
takes it over and keeps the dispatch unique.  Runs against a stand-in factory with the surface register() uses (`_strategies`,
`register`, unique-match `create_linear`) and this package's LinearBase, so it needs neither the reference tree nor a GPU."""
import pytest
import torch

from rtp_llm_amd import linear, model, reference_plugin


class _Factory:
    """The part of the reference's LinearFactory (factory.py:33-145) that registration and dispatch go through."""
    _strategies = []

    @classmethod
    def register(cls, s):
        if s not in cls._strategies:
            cls._strategies.append(s)

    @classmethod
    def hits(cls, weight, weight_scales):
        return [s for s in cls._strategies if s.can_handle(None, weight, weight_scales)]


class TheirFp8(linear.LinearBase):                 # stands for the reference's ROCm FP8 block-scale strategy
    @classmethod
    def can_handle(cls, quant_config, weight, weight_scales, hw_kernel_config=None, weight_scale_2=None, input_scale=None):
        return weight_scales is not None and weight.dtype == torch.float8_e4m3fn

    def __init__(self, weight, weight_scales=None, input_scales=None, bias=None, quant_config=None, weight_scale_2=None):
        super().__init__(weight, weight_scales, input_scales, bias, quant_config, weight_scale_2)

    def forward(self, input):
        return input


@pytest.fixture()
def factory():
    _Factory._strategies = [TheirFp8]
    yield _Factory
    _Factory._strategies = []


def _fp8_weight():
    c = model.synth_linear(128, 128, "fp8", "cpu", torch.Generator().manual_seed(0))
    return c.q.view(torch.float8_e4m3fn), c.scales


def test_default_registration_leaves_the_fp8_slot_alone(factory):
    added = reference_plugin.register(factory, linear.LinearBase)
    assert [c.__name__ for c in added] == ["Mi355W8A16Linear", "Mi355W4A16Linear"]       # what it registered before the FP8 strategy existed
    assert factory._strategies == [TheirFp8] + added
    w, s = _fp8_weight()
    assert factory.hits(w, s) == [TheirFp8]
    added = reference_plugin.register(_reset(factory), linear.LinearBase, replace_f16=True)
    assert [c.__name__ for c in added] == ["Mi355F16Linear", "Mi355W8A16Linear", "Mi355W4A16Linear"] and TheirFp8 in factory._strategies


def _reset(factory):
    factory._strategies = [TheirFp8]
    return factory


def test_replace_fp8_takes_the_slot_and_keeps_dispatch_unique(factory):
    added = reference_plugin.register(factory, linear.LinearBase, replace_fp8=True)
    assert [c.__name__ for c in added] == ["Mi355W8A16Linear", "Mi355W4A16Linear", "Mi355Fp8Linear"]
    assert TheirFp8 not in factory._strategies and factory._strategies == added
    w, s = _fp8_weight()
    for scales in (s, s[:, ::128].contiguous()):                                         # per-column and checkpoint block scales
        hits = factory.hits(w, scales)
        assert [h.__name__ for h in hits] == ["Mi355Fp8Linear"]
    lin = hits[0](w, s, None, None, None, None)
    assert isinstance(lin, linear.LinearBase) and lin.packed.wkind == 1 and (lin.in_features, lin.out_features) == (128, 128)
    # the other slots are untouched
    assert [h.__name__ for h in factory.hits(torch.zeros(128, 16, dtype=torch.int8), torch.ones(16).half())] == ["Mi355W8A16Linear"]
    assert factory.hits(torch.zeros(8, 8, dtype=torch.float16), None) == []
