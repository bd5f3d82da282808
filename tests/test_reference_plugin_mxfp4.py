"""reference_plugin.register() and the MXFP4 strategy: by default the FP4 slot is left to the factory's own strategies,
replace_mxfp4=True takes it over and keeps the dispatch unique.  Runs against a stand-in factory with the surface register() uses
(`_strategies`, `register`, unique-match dispatch) and this package's LinearBase, so it needs neither the reference tree nor a GPU."""
import pytest
import torch

from rtp_llm_amd import linear, model, reference_plugin

import mxfp4_util


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


class TheirFp4(linear.LinearBase):                 # stands for the reference's ROCm MXFP4 (W4A4) strategy
    @classmethod
    def can_handle(cls, quant_config, weight, weight_scales, hw_kernel_config=None, weight_scale_2=None, input_scale=None):
        return weight_scales is not None and weight.dtype == torch.uint8 and weight_scales.dtype == torch.uint8

    def __init__(self, weight, weight_scales=None, input_scales=None, bias=None, quant_config=None, weight_scale_2=None):
        super().__init__(weight, weight_scales, input_scales, bias, quant_config, weight_scale_2)

    def forward(self, input):
        return input


@pytest.fixture()
def factory():
    _Factory._strategies = [TheirFp4]
    yield _Factory
    _Factory._strategies = []


def _mxfp4_weight():
    c = model.synth_linear(128, 64, "mxfp4", "cpu", torch.Generator().manual_seed(0))
    return c, mxfp4_util.to_quark(c)


def test_default_registration_leaves_the_fp4_slot_alone(factory):
    added = reference_plugin.register(factory, linear.LinearBase)
    assert [c.__name__ for c in added] == ["Mi355W8A16Linear", "Mi355W4A16Linear"]       # what it registered before the strategy existed
    assert factory._strategies == [TheirFp4] + added
    _, (w, s) = _mxfp4_weight()
    assert factory.hits(w, s) == [TheirFp4]                                               # the W4 strategy does not claim e8m0 scales
    factory._strategies = [TheirFp4]
    added = reference_plugin.register(factory, linear.LinearBase, replace_fp8=True)
    assert "Mi355Mxfp4Linear" not in [c.__name__ for c in added] and TheirFp4 in factory._strategies


def test_replace_mxfp4_takes_the_slot_and_keeps_dispatch_unique(factory):
    added = reference_plugin.register(factory, linear.LinearBase, replace_mxfp4=True)
    assert [c.__name__ for c in added] == ["Mi355W8A16Linear", "Mi355W4A16Linear", "Mi355Mxfp4Linear"]
    assert TheirFp4 not in factory._strategies and factory._strategies == added
    c, (w, s) = _mxfp4_weight()
    hits = factory.hits(w, s)
    assert [h.__name__ for h in hits] == ["Mi355Mxfp4Linear"]
    lin = hits[0](w, s, None, None, None, None)
    assert isinstance(lin, linear.LinearBase) and lin.packed.wkind == 2 and (lin.in_features, lin.out_features) == (128, 64)
    assert torch.equal(lin.packed.qweight, c.pack().qweight) and torch.equal(lin.packed.meta, c.pack().meta)
    # the other slots are untouched
    assert [h.__name__ for h in factory.hits(torch.zeros(128, 16, dtype=torch.int8), torch.ones(16).half())] == ["Mi355W8A16Linear"]
    w4 = model.synth_linear(128, 64, "w4", "cpu", torch.Generator().manual_seed(1))
    assert [h.__name__ for h in factory.hits(w4.q, w4.scales)] == ["Mi355W4A16Linear"]
    assert factory.hits(torch.zeros(8, 8, dtype=torch.float16), None) == []
