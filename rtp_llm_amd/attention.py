"""Attention strategies, decode and prefill — the reference's FMHA plug-in surface
(rtp_llm/models_py/modules/factory/attention/{fmha_impl_base.py:99-178, attn_factory.py:100-254}):

    DECODE_MHA_IMPS.append(cls) / PREFILL_MHA_IMPS.append(cls); cls.support(attn_configs, attn_inputs);
    impl = cls(attn_configs, attn_inputs, parallelism_config); impl.forward(qkv, LayerKVCache, layer_idx)

Data-contract mirrors (bindings/OpDefs.h:29-51,281-327; cpp/model_utils/AttentionConfig.h:24-85):
LayerKVCache, PyAttentionInputs, AttentionConfigs — same field names, the fields the two impls use.

Both impls write and read the cache in ``AttentionConfigs.kv_layout`` (kvcache.py).  An integrator who replaces BOTH lists may keep
the native layout; one who keeps the reference's prefill op (or its block reuse / prefix caching) sets the reference layout with the
V form of the decode back-end being replaced, so that both sides see the same bytes.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import ops


@dataclass
class AttentionConfigs:       # cpp/model_utils/AttentionConfig.h:24-85 (per-rank values)
    head_num: int
    kv_head_num: int
    size_per_head: int
    rope_dim: int = 0
    rope_theta: float = 1e6
    max_seq_len: int = 4096
    softmax_extra_scale: float = 1.0
    kernel_tokens_per_block: int = 16
    kv_layout: int = 0             # _C.KV_LAYOUT_*: intra-block layout of the caches (not a field of the reference's struct; native by default)


@dataclass
class LayerKVCache:           # bindings/OpDefs.h:29-51
    kv_cache_base: torch.Tensor                    # [blocks, 2, nkv, page, hd]
    kv_scale_base: Optional[torch.Tensor] = None   # [blocks, 2*nkv*page] fp32 (8-bit caches)
    seq_size_per_block: int = 0
    layer_id: int = -1


@dataclass
class PyAttentionInputs:      # bindings/OpDefs.h:281-327; prefill fields appended
    is_prefill: bool = False
    sequence_lengths: torch.Tensor = None              # int32 [B]: tokens already in the cache
    input_lengths: torch.Tensor = None
    kv_cache_kernel_block_id_device: torch.Tensor = None   # int32 [B, M]
    is_cuda_graph: bool = False
    sequence_lengths_plus_1_device: torch.Tensor = None    # filled by prepare()
    prefix_lengths: torch.Tensor = None                # prefill, int32 [B]: tokens of each sequence already in the cache (None = 0)
    cu_seqlens: torch.Tensor = None                    # prefill, int32 [B + 1]: offsets of the sequences in the packed token order


class FMHAImplBase:
    def forward(self, qkv, kv_cache, layer_idx: int = 0):
        raise NotImplementedError

    @staticmethod
    def support(attn_configs, attn_inputs) -> bool:
        return False

    def support_cuda_graph(self) -> bool:       # fmha_impl_base.py:165-172
        return callable(getattr(self, "prepare_cuda_graph", None))


class Mi355PagedDecodeImpl(FMHAImplBase):
    """RoPE+KV-write op followed by the paged flash-decoding op (the pairing of
    AiterDecodeImpl*, rocm_impl/aiter.py:1960-2031)."""

    def __init__(self, attn_configs: AttentionConfigs, attn_inputs: PyAttentionInputs, parallelism_config=None,
                 cos_sin: Optional[torch.Tensor] = None, qkv_bias: Optional[torch.Tensor] = None):
        self.cfg = attn_configs
        self.cos_sin = cos_sin
        self.prepare(attn_inputs)

    @staticmethod
    def support(attn_configs: AttentionConfigs, attn_inputs: PyAttentionInputs) -> bool:
        return not attn_inputs.is_prefill and _head_shape_ok(attn_configs)

    def prepare(self, attn_inputs: PyAttentionInputs):
        """Host-side prep (FMHAParams, aiter.py:205-209: seq_lens = sequence_lengths + 1 on device)."""
        self.inputs = attn_inputs
        dev = attn_inputs.kv_cache_kernel_block_id_device.device
        self.positions = attn_inputs.sequence_lengths.to(device=dev, dtype=torch.int32).contiguous()
        self.seq_lens = (self.positions + 1).contiguous()
        attn_inputs.sequence_lengths_plus_1_device = self.seq_lens
        self.block_table = attn_inputs.kv_cache_kernel_block_id_device.to(torch.int32).contiguous()

    def prepare_cuda_graph(self, attn_inputs: PyAttentionInputs):
        """In-place refresh of the address-stable device buffers for graph replay (aiter.py:1964-1981)."""
        self.positions.copy_(attn_inputs.sequence_lengths.to(self.positions.device, torch.int32))
        torch.add(self.positions, 1, out=self.seq_lens)
        self.block_table.copy_(attn_inputs.kv_cache_kernel_block_id_device)

    def forward(self, qkv: torch.Tensor, kv_cache: LayerKVCache, layer_idx: int = 0) -> torch.Tensor:
        c = self.cfg
        page = kv_cache.seq_size_per_block or kv_cache.kv_cache_base.shape[3]
        q = ops.rope_kv_write(qkv.contiguous(), None, self.cos_sin, self.positions, self.block_table, kv_cache.kv_cache_base,
                              kv_cache.kv_scale_base, c.head_num, c.kv_head_num, c.size_per_head, page, layout=c.kv_layout)
        return ops.paged_decode_attention(q, kv_cache.kv_cache_base, kv_cache.kv_scale_base, self.block_table, self.seq_lens,
                                          c.kv_head_num, page, c.max_seq_len,
                                          c.softmax_extra_scale / math.sqrt(c.size_per_head), layout=c.kv_layout)


def _head_shape_ok(c: AttentionConfigs) -> bool:
    """what both impls ask of the heads and the rotation"""
    g = c.head_num // max(1, c.kv_head_num)
    return (c.size_per_head in (64, 128) and g <= 16 and c.head_num % c.kv_head_num == 0
            and c.rope_dim in (0, c.size_per_head))


class Mi355PrefillImpl(FMHAImplBase):
    """Prompt ingestion over the paged cache: the rows-mode RoPE + KV writer followed by causal multi-row paged attention (the pairing
    of FusedRopeKVCachePrefillOp + the prefill FMHA, FusedRopeKVCacheOp.cc:216-461 / aiter.py:244-950).

    The reference hands the tokens of a prefill batch PACKED, [sum(input_lengths), ...] in sequence order; the kernels take q_len rows
    per sequence.  prepare() builds that padded row layout on the host: row i of sequence b at b * q_len + i with position
    prefix_lengths[b] + i, -1 for padding rows (never written, output zeros), q_len = max(input_lengths).  forward() scatters the packed
    rows into it, runs the two ops and gathers the real rows back.  A prompt longer than the caller wants in one call comes in chunks:
    prefix_lengths carries what the earlier chunks wrote."""

    def __init__(self, attn_configs: AttentionConfigs, attn_inputs: PyAttentionInputs, parallelism_config=None,
                 cos_sin: Optional[torch.Tensor] = None, qkv_bias: Optional[torch.Tensor] = None):
        self.cfg = attn_configs
        self.cos_sin = cos_sin
        self.prepare(attn_inputs)

    @staticmethod
    def support(attn_configs: AttentionConfigs, attn_inputs: PyAttentionInputs) -> bool:
        return bool(attn_inputs.is_prefill) and _head_shape_ok(attn_configs)

    def prepare(self, attn_inputs: PyAttentionInputs):
        self.inputs = attn_inputs
        if attn_inputs.input_lengths is not None:
            lens = [int(v) for v in attn_inputs.input_lengths.tolist()]
        elif attn_inputs.cu_seqlens is not None:
            cu = [int(v) for v in attn_inputs.cu_seqlens.tolist()]
            lens = [b - a for a, b in zip(cu[:-1], cu[1:])]
        else:
            raise ValueError("Mi355PrefillImpl: attn_inputs needs input_lengths or cu_seqlens")
        B = len(lens)
        prefix = [0] * B if attn_inputs.prefix_lengths is None else [int(v) for v in attn_inputs.prefix_lengths.tolist()]
        if len(prefix) != B or B == 0 or min(lens) < 1 or min(prefix) < 0:
            raise ValueError(f"Mi355PrefillImpl: input_lengths {lens} / prefix_lengths {prefix}")
        if attn_inputs.cu_seqlens is not None and attn_inputs.input_lengths is not None:
            cu = [int(v) for v in attn_inputs.cu_seqlens.tolist()]
            if [b - a for a, b in zip(cu[:-1], cu[1:])] != lens:
                raise ValueError("Mi355PrefillImpl: cu_seqlens does not match input_lengths")
        if max(p + n for p, n in zip(prefix, lens)) > self.cfg.max_seq_len:
            raise ValueError(f"Mi355PrefillImpl: prefix + input length exceeds max_seq_len={self.cfg.max_seq_len}")
        q_len = max(lens)
        positions = torch.full((B * q_len,), -1, dtype=torch.int32)
        token_of_row = torch.full((B * q_len,), -1, dtype=torch.int64)
        row_of_token = torch.empty(sum(lens), dtype=torch.int64)
        t = 0
        for b, (n, p) in enumerate(zip(lens, prefix)):
            positions[b * q_len:b * q_len + n] = torch.arange(p, p + n, dtype=torch.int32)
            token_of_row[b * q_len:b * q_len + n] = torch.arange(t, t + n)
            row_of_token[t:t + n] = torch.arange(b * q_len, b * q_len + n)
            t += n
        bt = attn_inputs.kv_cache_kernel_block_id_device
        dev = bt.device
        self.batch, self.q_len, self.num_tokens = B, q_len, t
        self.positions = positions.to(dev)
        self.row_of_token = row_of_token.to(dev)    # packed token k lives in padded row row_of_token[k]: scatter AND gather index
        self.token_of_row = token_of_row.to(dev)    # the inverse, -1 for padding rows
        self.block_table = bt.to(torch.int32).contiguous()

    def scatter(self, packed: torch.Tensor) -> torch.Tensor:
        """[T, ...] packed -> [B * q_len, ...] padded rows (padding rows zero)"""
        out = packed.new_zeros((self.batch * self.q_len,) + tuple(packed.shape[1:]))
        return out.index_copy_(0, self.row_of_token, packed)

    def gather(self, rows: torch.Tensor) -> torch.Tensor:
        """[B * q_len, ...] padded rows -> [T, ...] packed"""
        return rows.index_select(0, self.row_of_token)

    def forward(self, qkv: torch.Tensor, kv_cache: LayerKVCache, layer_idx: int = 0) -> torch.Tensor:
        c = self.cfg
        if qkv.shape[0] != self.num_tokens:
            raise ValueError(f"Mi355PrefillImpl: {qkv.shape[0]} packed rows, attn_inputs describe {self.num_tokens}")
        page = kv_cache.seq_size_per_block or kv_cache.kv_cache_base.shape[3]
        q = ops.rope_kv_write_rows(self.scatter(qkv.contiguous()), None, self.cos_sin, self.positions, self.block_table,
                                   kv_cache.kv_cache_base, kv_cache.kv_scale_base, c.head_num, c.kv_head_num, c.size_per_head, page,
                                   self.q_len, layout=c.kv_layout)
        out = ops.paged_attention_rows(q, kv_cache.kv_cache_base, kv_cache.kv_scale_base, self.block_table, self.positions,
                                       c.kv_head_num, page, self.q_len, c.max_seq_len,
                                       c.softmax_extra_scale / math.sqrt(c.size_per_head), layout=c.kv_layout)
        return self.gather(out)


DECODE_MHA_IMPS: List[type] = [Mi355PagedDecodeImpl]   # attention/__init__.py:47-49 registration lists
PREFILL_MHA_IMPS: List[type] = [Mi355PrefillImpl]


class AttnImplFactory:
    """attn_factory.py:226-254: first impl of the list for the phase (is_prefill) whose support() accepts the inputs."""

    @staticmethod
    def get_fmha_impl(attn_configs, attn_inputs, parallelism_config=None, **kw) -> FMHAImplBase:
        for impl in (PREFILL_MHA_IMPS if attn_inputs.is_prefill else DECODE_MHA_IMPS):
            if impl.support(attn_configs, attn_inputs):
                inst = impl(attn_configs, attn_inputs, parallelism_config, **kw)
                if attn_inputs.is_cuda_graph and not inst.support_cuda_graph():
                    continue
                return inst
        raise RuntimeError(f"no {'prefill' if attn_inputs.is_prefill else 'decode'} FMHA implementation supports these inputs")
