"""Bind the MI355 linear strategies and attention impls to the REFERENCE's own plug-in classes.

The reference picks a linear implementation by asking every class registered with its ``LinearFactory`` whether it
``can_handle`` the weight dict (rtp_llm/models_py/modules/factory/linear/factory.py:33-145; registration at import time
in impl/rocm/__init__.py:16-20).  ``register(LinearFactory, LinearBase)`` creates subclasses of the reference's
``LinearBase`` (linear_base.py:16-102) around this package's strategy implementations and registers them, which fills the
W4A16 / W8A16 slot the snapshot leaves empty -- model code such as ``CausalAttention`` / ``DenseMLP`` then
runs unchanged.  The reference-side call is one line in impl/rocm/__init__.py.
"""
from typing import List

from .attention import Mi355PagedDecodeImpl, Mi355PrefillImpl
from .linear import STRATEGY_IMPLS


def make_strategies(ref_linear_base) -> List[type]:
    """Subclasses of the reference's LinearBase, one per MI355 strategy."""
    return [type(name, (impl, ref_linear_base), {"__module__": __name__, "__doc__": impl.__doc__}) for name, impl in STRATEGY_IMPLS]


def register(ref_linear_factory, ref_linear_base, replace_f16: bool = False, replace_fp8: bool = False,
             replace_mxfp4: bool = False) -> List[type]:
    """Register the strategies with the reference's factory.  The fp16 strategy overlaps the reference's own ROCm fp16
    strategies (RocmF16Linear*), and the factory demands a unique match, so it is only registered when asked to replace
    them (``replace_f16``: existing fp16 strategies are removed first).  The same holds for the FP8 block-scale strategy and
    the reference's ROCm FP8 strategies (``replace_fp8``: strategies that claim a float8_e4m3fn weight with 2-D block scales
    are removed first); by default the FP8 slot is left to the reference.  Likewise the MXFP4 strategy (``replace_mxfp4``:
    strategies that claim a uint8 [N, K/2] weight with uint8 e8m0 scales [N, K/32] are removed first) -- note that it is
    weight-only, where the reference's FP4 strategies quantise the activations as well."""
    out = []
    for cls in make_strategies(ref_linear_base):
        if cls.__name__ == "Mi355F16Linear":
            if not replace_f16:
                continue
            import torch
            probe = torch.zeros(8, 8, dtype=torch.float16)
            ref_linear_factory._strategies[:] = [s for s in ref_linear_factory._strategies
                                                 if not _safe_can_handle(s, probe)]
        if cls.__name__ == "Mi355Fp8Linear":
            if not replace_fp8:
                continue
            import torch
            probe, scales = torch.zeros(128, 128, dtype=torch.float8_e4m3fn), torch.ones(1, 1, dtype=torch.float32)
            ref_linear_factory._strategies[:] = [s for s in ref_linear_factory._strategies
                                                 if not _safe_can_handle(s, probe, scales)]
        if cls.__name__ == "Mi355Mxfp4Linear":
            if not replace_mxfp4:
                continue
            import torch
            probe, scales = torch.zeros(16, 64, dtype=torch.uint8), torch.full((16, 4), 127, dtype=torch.uint8)
            ref_linear_factory._strategies[:] = [s for s in ref_linear_factory._strategies
                                                 if not _safe_can_handle(s, probe, scales)]
        ref_linear_factory.register(cls)
        out.append(cls)
    return out


def register_attention(decode_list: list, prefill_list: list, fmha_base) -> List[type]:
    """Bind the two attention impls to the reference's FMHA plug-in lists (factory/attention/__init__.py: DECODE_MHA_IMPS /
    PREFILL_MHA_IMPS, first impl whose support() accepts the inputs wins): subclasses of the reference's FMHAImplBase around
    Mi355PagedDecodeImpl and Mi355PrefillImpl, inserted at the FRONT of the lists.  Registering both keeps writer and reader of the
    cache on one side; registering by hand only the decode one requires AttentionConfigs.kv_layout to name the reference's layout
    (INTEGRATION.md section 1).  Returns [decode class, prefill class]."""
    out = []
    for impl, lst in ((Mi355PagedDecodeImpl, decode_list), (Mi355PrefillImpl, prefill_list)):
        cls = type(impl.__name__, (impl, fmha_base), {"__module__": __name__, "__doc__": impl.__doc__})
        lst.insert(0, cls)
        out.append(cls)
    return out


def _safe_can_handle(strategy, weight, weight_scales=None) -> bool:
    try:
        return bool(strategy.can_handle(None, weight, weight_scales, None, None, None))
    except Exception:  # noqa: BLE001  (a strategy that cannot even inspect the probe weight does not claim it)
        return False
