"""HF checkpoint -> canonical weights -> (TP split) -> MI355-native packed weights.

The decode-path slice of the reference's loader stack:
  * HF names -> W-names: rtp_llm/models/qwen_v2.py:43-335 (Qwen2), rtp_llm/models/llama_weight.py (Llama);
  * QKV merge [q | k | v] along the output dim (merge_qkv_hf, rtp_llm/utils/model_weight.py) and gate/up merge
    into ffn_w13 (model_loader/group_wise_quant_weight.py:211-260);
  * GPTQ / AWQ tensors `.qweight/.qzeros/.scales` (model_loader/group_wise_quant_weight.py:35-301), canonicalised
    by rtp_llm_amd.quant (device_impl.py:148-171,242-300); like the reference loader, `g_idx` (act-order) is not
    supported — the reference never reads it — and a non-trivial g_idx is rejected here;
  * FP8 block-quantised checkpoints (`quant_method: "fp8"`, the published form of the Qwen3 dense family): `.weight` float8_e4m3fn
    [out, in] with `.weight_scale_inv` fp32 [ceil(out/128), ceil(in/128)]; the codes are kept as they are and the block scale is
    expanded per output column (_linear_fp8), so splits and merges are plain column / 128-row operations;
  * MXFP4 checkpoints in the Quark form (`quant_method: "quark"`, weight dtype "fp4", per_group 32, scale_format "e8m0"): `.weight`
    uint8 [out, in/2] (low nibble = even input index) with `.weight_scale` uint8 [out, in/32]; weight-only here, the declared
    activation quantisation is ignored (_check_quark_config, _linear_mxfp4);
  * `--quantization int8`: load-time per-channel autoquant of the fp16 linears (weight_only_quant_weight.py:94-105).

With quantization="int8" the per-channel scales are computed on the full [K, N] weight BEFORE the row-parallel TP split
(the reference autoquantises each rank's shard; both are valid per-channel quantisations, this one makes every rank's
codes a slice of the tp = 1 codes).  bf16 / fp32 checkpoint tensors are converted to fp16 at load time.

Pure host code (safetensors + torch on CPU); the result feeds model.DecoderEngine / Qwen2DecoderModel unchanged.
"""
import fnmatch
import json
import logging
import os
from typing import Dict, Optional, Tuple

import torch

from . import quant
from .model import CanonLinear, ModelConfig, split_layer_tp


class _Shards:
    """Tensor lookup over one or several safetensors files (model.safetensors.index.json aware)."""

    def __init__(self, path: str):
        from safetensors import safe_open
        self.path = path
        idx = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(idx):
            self.map = json.load(open(idx))["weight_map"]
        else:
            files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
            if not files:
                raise FileNotFoundError(f"no .safetensors files under {path}")
            self.map = {}
            for f in files:
                with safe_open(os.path.join(path, f), "pt") as sf:
                    for k in sf.keys():
                        self.map[k] = f
        self._open = {}
        self._safe_open = safe_open

    def has(self, name: str) -> bool:
        return name in self.map

    def get(self, name: str) -> torch.Tensor:
        f = self.map[name]
        if f not in self._open:
            self._open[f] = self._safe_open(os.path.join(self.path, f), "pt")
        return self._open[f].get_tensor(name)


def config_from_hf(cfg: dict, name: str = "hf-model") -> Tuple[ModelConfig, dict]:
    """config.json -> (ModelConfig, quantization dict) — the fields models/qwen_v2.py:338-399 reads."""
    nh = cfg["num_attention_heads"]
    # newer transformers write RoPE settings as `rope_parameters` ({"rope_theta", "rope_type", ...}) instead of rope_theta / rope_scaling
    rp = cfg.get("rope_parameters") or {}
    theta = cfg.get("rope_theta", rp.get("rope_theta", 10000.0))
    mc = ModelConfig(name=name, num_layers=cfg["num_hidden_layers"], hidden=cfg["hidden_size"], nh=nh,
                     nkv=cfg.get("num_key_value_heads", nh), hd=cfg.get("head_dim", cfg["hidden_size"] // nh),
                     inter=cfg["intermediate_size"], vocab=cfg["vocab_size"], rope_theta=float(theta),
                     rms_eps=float(cfg.get("rms_norm_eps", 1e-6)), qkv_bias=False,
                     max_pos=int(cfg.get("max_position_embeddings", 8192)),
                     qk_norm=cfg.get("model_type") == "qwen3")   # Qwen3 dense: per-head q_norm / k_norm (also set when the tensors are found)
    if cfg.get("model_type") == "qwen3_moe":
        raise NotImplementedError("mixture-of-experts models (Qwen3-MoE) are not on this decode path")
    rs = cfg.get("rope_scaling") or {k: v for k, v in rp.items() if k != "rope_theta"}
    kind = rs.get("rope_type", rs.get("type", "default")) if rs else "default"
    if kind not in ("default", None):
        # linear / llama3 / yarn fold into the position-indexed cos/sin table (model.rope_frequencies); "dynamic" (models/llama.py:95-96,
        # gpt_neox.py:128-134: RopeStyle::DynamicNTK, scale = factor, original context = max_position_embeddings) gets one base per position
        if kind not in ("linear", "llama3", "yarn", "dynamic"):
            raise NotImplementedError(f"rope_scaling={rs}: only base / linear / llama3 / yarn / dynamic RoPE are on this decode path")
        mc.rope_scaling = dict(rs)
        if kind == "dynamic":
            mc.rope_scaling.setdefault("original_max_position_embeddings", int(cfg.get("max_position_embeddings", 2048)))
    if cfg.get("use_dynamic_ntk"):   # Qwen-1 (models/qwen.py:293-295): RopeStyle::QwenDynamicNTK over seq_length
        mc.rope_scaling = {"rope_type": "qwen_dynamic", "original_max_position_embeddings": int(cfg.get("seq_length", 8192))}
    if cfg.get("use_sliding_window"):
        raise NotImplementedError("sliding-window attention is not on this decode path")
    q = cfg.get("quantization_config") or {}
    qc = {"method": q.get("quant_method", "none"), "bits": int(q.get("bits", 16)), "group_size": int(q.get("group_size", 0)),
          "desc_act": bool(q.get("desc_act", False))}
    return mc, qc


def _f16(t: torch.Tensor, name: str, dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """Checkpoint tensor -> the activation dtype of the model.  fp16 (default): bf16 / fp32 checkpoints (Qwen2 ships bf16) are
    converted once at load time; a value outside the fp16 range would become inf silently, so it is an error.  bf16
    (DecoderEngine(dtype=torch.bfloat16)): bf16 tensors stay as they are, fp16 / fp32 ones are rounded to bf16.  Quantisation
    scales are always fp16 (the meta image of the W4 / W8 kernels)."""
    if t.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise TypeError(f"{name}: unsupported tensor dtype {t.dtype}")
    if dtype == torch.bfloat16:
        return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)
    if t.dtype == torch.float16:
        return t
    if t.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{name}: unsupported tensor dtype {t.dtype}")
    o = t.to(torch.float16)
    if not bool(torch.isfinite(o).all()):
        raise ValueError(f"{name}: {t.dtype} values exceed the fp16 range")
    return o


def _from_fp16_tensor(t: torch.Tensor, prefix: str, dtype: torch.dtype = torch.float16) -> CanonLinear:
    w = _f16(t, prefix, dtype)                              # HF stores [out, in]
    return CanonLinear("fp16", w.shape[1], w.shape[0], w=w.t().contiguous())


def _linear_fp16(sh: _Shards, prefix: str, dtype: torch.dtype = torch.float16) -> CanonLinear:
    return _from_fp16_tensor(sh.get(prefix + ".weight"), prefix, dtype)


def _linear_quant(sh: _Shards, prefix: str, method: str, group_size: int) -> CanonLinear:
    qw, qz, sc = sh.get(prefix + ".qweight"), sh.get(prefix + ".qzeros"), _f16(sh.get(prefix + ".scales"), prefix + ".scales")
    if sh.has(prefix + ".g_idx"):
        gidx = sh.get(prefix + ".g_idx")
        K = gidx.numel()
        if not torch.equal(gidx.to(torch.int64), torch.arange(K) // group_size):
            raise NotImplementedError(f"{prefix}: act-order (non-trivial g_idx) checkpoints are not supported")
    q, z = (quant.unpack_gptq if method == "gptq" else quant.unpack_awq)(qw, qz)
    return CanonLinear("w4", q.shape[0], q.shape[1], q=q, scales=sc, z_eff=z, group_size=group_size)


def _check_fp8_config(q: dict) -> set:
    """The FP8 scheme this decode path serves: e4m3 weights, dynamic activations (the weight-only path ignores them), one scale per
    128 x 128 block.  Everything else is refused by the name of the field.  Returns modules_to_not_convert as a set of names."""
    fmt = q.get("fmt", q.get("format"))
    if fmt not in (None, "e4m3"):
        raise NotImplementedError(f"quantization_config.fmt={fmt!r}: only e4m3 FP8 weights are on this decode path")
    if q.get("activation_scheme", "dynamic") != "dynamic":
        raise NotImplementedError(f"quantization_config.activation_scheme={q.get('activation_scheme')!r}: static activation scales are not supported")
    wbs = q.get("weight_block_size")
    if wbs is None:
        raise NotImplementedError("quantization_config.weight_block_size is absent: per-tensor / per-channel FP8 scales are not supported (128 x 128 blocks only)")
    if list(wbs) != [quant.FP8_BLOCK, quant.FP8_BLOCK]:
        raise NotImplementedError(f"quantization_config.weight_block_size={wbs}: only [128, 128] is supported")
    return set(q.get("modules_to_not_convert") or [])


def _linear_fp8(sh: _Shards, prefix: str, w: torch.Tensor) -> CanonLinear:
    """w: the module's `.weight` as read from the checkpoint, float8_e4m3fn [out, in]."""
    if not sh.has(prefix + ".weight_scale_inv"):
        raise NotImplementedError(f"{prefix}: FP8 weight without weight_scale_inv (per-tensor weight_scale checkpoints are not supported)")
    s = sh.get(prefix + ".weight_scale_inv")
    N, K = w.shape
    B = quant.FP8_BLOCK
    if s.dim() != 2 or tuple(s.shape) != ((N + B - 1) // B, (K + B - 1) // B):
        raise NotImplementedError(f"{prefix}.weight_scale_inv: shape {tuple(s.shape)}, expected one scale per 128 x 128 block of [{N}, {K}]")
    codes = w.view(torch.uint8).t().contiguous()            # [K, N]
    if bool(((codes & 0x7F) == 0x7F).any()):
        raise ValueError(f"{prefix}.weight holds an FP8 NaN code (byte & 0x7f == 0x7f)")
    scales = quant.expand_fp8_block_scales(s.float().t().contiguous(), N)
    return CanonLinear("fp8", K, N, q=codes, scales=scales, group_size=B)


def _check_quark_config(q: dict) -> list:
    """The Quark scheme this decode path serves: MXFP4 weights -- dtype "fp4", qscheme "per_group", group_size 32, scale_format "e8m0",
    static, grouped along the input dimension.  Activation entries (input_tensors) must be dynamic and are ignored: weight-only.
    Everything else is refused by the name of the field.  Returns the `exclude` patterns."""
    g = q.get("global_quant_config")
    if not isinstance(g, dict) or not isinstance(g.get("weight"), dict):
        raise NotImplementedError("quantization_config.global_quant_config.weight is absent: not a Quark MXFP4 checkpoint this decode path serves")
    w = g["weight"]
    if w.get("dtype") != "fp4":
        raise NotImplementedError(f"quantization_config.global_quant_config.weight.dtype={w.get('dtype')!r}: only 'fp4' (MXFP4) Quark weights are supported")
    if w.get("qscheme") != "per_group":
        raise NotImplementedError(f"quantization_config.global_quant_config.weight.qscheme={w.get('qscheme')!r}: only 'per_group' is supported")
    if w.get("group_size") != quant.MXFP4_GROUP:
        raise NotImplementedError(f"quantization_config.global_quant_config.weight.group_size={w.get('group_size')!r}: MXFP4 groups are 32 weights")
    if w.get("scale_format") != "e8m0":
        raise NotImplementedError(f"quantization_config.global_quant_config.weight.scale_format={w.get('scale_format')!r}: only 'e8m0' scales are supported (NVFP4 and float scales are not)")
    if w.get("is_dynamic", False):
        raise NotImplementedError("quantization_config.global_quant_config.weight.is_dynamic=True: weights must be quantised ahead of time")
    if w.get("ch_axis", -1) not in (-1, 1):
        raise NotImplementedError(f"quantization_config.global_quant_config.weight.ch_axis={w.get('ch_axis')!r}: groups must run along the input dimension (axis 1 / -1 of [out, in])")
    it = g.get("input_tensors")
    if it is not None and not (isinstance(it, dict) and it.get("is_dynamic", False)):
        raise NotImplementedError("quantization_config.global_quant_config.input_tensors is not dynamic: static activation scales are not supported")
    for k in ("desc_act", "desc"):
        if q.get(k) or w.get(k):
            raise NotImplementedError(f"quantization_config {k}: act-order extras are not supported with MXFP4")
    if q.get("layer_quant_config") or q.get("layer_type_quant_config"):
        which = "layer_quant_config" if q.get("layer_quant_config") else "layer_type_quant_config"
        raise NotImplementedError(f"quantization_config.{which} is not empty: per-layer overrides to another scheme are not supported")
    return list(q.get("exclude") or [])


def _linear_mxfp4(sh: _Shards, prefix: str, w: torch.Tensor, flushed: list) -> CanonLinear:
    """w: the module's `.weight` as read from the checkpoint, uint8 [out, in/2].  flushed: running [groups, weights] totals of the
    exponent rule (quant.mxfp4_apply_range)."""
    if not sh.has(prefix + ".weight_scale"):
        raise NotImplementedError(f"{prefix}.weight_scale is missing: an MXFP4 weight needs its e8m0 group scales")
    s = sh.get(prefix + ".weight_scale")
    if s.dtype != torch.uint8:
        raise NotImplementedError(f"{prefix}.weight_scale: dtype {s.dtype}, expected uint8 e8m0 bytes (float scales are not supported)")
    N, K = w.shape[0], w.shape[1] * 2
    if w.dim() != 2 or K % quant.MXFP4_GROUP or tuple(s.shape) != (N, K // quant.MXFP4_GROUP):
        raise ValueError(f"{prefix}.weight_scale: shape {tuple(s.shape)}, expected ({N}, {K // quant.MXFP4_GROUP}): one byte per 32 inputs of "
                         f"{prefix}.weight {tuple(w.shape)}")
    try:
        codes, sb, g, n = quant.mxfp4_apply_range(*quant.mxfp4_from_checkpoint(w, s))
    except ValueError as e:
        raise ValueError(f"{prefix}.weight_scale: {e}") from None
    flushed[0] += g
    flushed[1] += n
    return CanonLinear("mxfp4", K, N, q=codes, scales=sb, group_size=quant.MXFP4_GROUP)


def _cat_same_kind(parts, what: str) -> CanonLinear:
    if len({p.kind for p in parts}) != 1:
        raise NotImplementedError(f"{what}: the merged projections are stored in different formats {[p.kind for p in parts]}")
    return CanonLinear.cat_cols(parts)


def load_hf_checkpoint(path: str, quantization: Optional[str] = None, tp: int = 1, rank: int = 0,
                       max_layers: Optional[int] = None, split_embedding: bool = False,
                       dtype: torch.dtype = torch.float16) -> Tuple[ModelConfig, Dict]:
    """Read an HF Qwen2/Llama/Qwen3 checkpoint (fp16, GPTQ-4bit, AWQ-4bit, FP8 e4m3 with 128 x 128 block scales or Quark MXFP4) into the canonical weight dict of
    rtp_llm_amd.model (per-rank tensors when tp > 1).  quantization="int8" autoquantises fp16 linears at load time.
    split_embedding (tp > 1): the embedding table comes back as this rank's [vocab, hidden / tp] column slice, the reference's TP
    layout (utils/model_weight.py:1490 sp_neg1) -- pair it with DecoderEngine.set_embedding_split(); default: replicated table
    (no collective in the lookup).  dtype: activation dtype the model will run in (see _f16); bf16 excludes quantization="int8"."""
    if dtype not in (torch.float16, torch.bfloat16) or (dtype == torch.bfloat16 and quantization == "int8"):
        raise NotImplementedError(f"load_hf_checkpoint: dtype {dtype} with quantization {quantization}")
    cfg_json = json.load(open(os.path.join(path, "config.json")))
    mc, qc = config_from_hf(cfg_json, os.path.basename(os.path.normpath(path)))
    fp8 = qc["method"] == "fp8"
    fp8_skip = _check_fp8_config(cfg_json.get("quantization_config") or {}) if fp8 else set()
    if fp8 and quantization == "int8":
        raise NotImplementedError("load_hf_checkpoint: quantization='int8' on an FP8 checkpoint")
    mx = qc["method"] == "quark"
    mx_skip = _check_quark_config(cfg_json.get("quantization_config") or {}) if mx else []
    mx_flushed = [0, 0]
    if mx and quantization == "int8":
        raise NotImplementedError("load_hf_checkpoint: quantization='int8' on an MXFP4 checkpoint")
    if not fp8 and not mx and (qc["method"] not in ("none", "gptq", "awq") or (qc["method"] != "none" and qc["bits"] != 4)):
        raise NotImplementedError(f"quantization_config {qc} is outside the decode path of this build (4-bit GPTQ/AWQ, FP8 128 x 128 blocks, "
                                  "Quark MXFP4: fp4 per_group 32 with e8m0 scales)")
    if qc["desc_act"]:
        raise NotImplementedError("desc_act=True (act-order) GPTQ checkpoints are not supported (the reference ignores g_idx too)")
    sh = _Shards(path)
    pre = "model." if sh.has("model.embed_tokens.weight") else ""
    L = mc.num_layers if max_layers is None else min(mc.num_layers, max_layers)
    quantised = qc["method"] in ("gptq", "awq")

    def not_converted(name):   # listed in modules_to_not_convert: by full name, without the "model." prefix, or by a trailing component
        names = {name, name[len(pre):] if pre and name.startswith(pre) else name}
        return any(n in fp8_skip or any(n.endswith("." + m) for m in fp8_skip) for n in names)

    def excluded(name):        # Quark `exclude`: module names or glob patterns, with or without the "model." prefix
        names = {name, name[len(pre):] if pre and name.startswith(pre) else name}
        return any(n == m or n.endswith("." + m) or fnmatch.fnmatchcase(n, m) for n in names for m in mx_skip)

    def lin(name):
        if mx:
            w = sh.get(name + ".weight")
            if excluded(name):
                if w.dtype == torch.uint8:
                    raise ValueError(f"{name}.weight is uint8 but the module is listed in quantization_config.exclude")
                return _from_fp16_tensor(w, name, dtype)
            if w.dtype != torch.uint8:
                raise NotImplementedError(f"{name}.weight: dtype {w.dtype} in an MXFP4 checkpoint and the module is not in quantization_config.exclude")
            return _linear_mxfp4(sh, name, w, mx_flushed)
        if fp8 and not not_converted(name):
            w = sh.get(name + ".weight")                      # read once: a module stored 16-bit falls through to _linear_fp16
            if w.dtype == torch.float8_e4m3fn:
                return _linear_fp8(sh, name, w)
            return _from_fp16_tensor(w, name, dtype)
        c = _linear_quant(sh, name, qc["method"], qc["group_size"]) if quantised and sh.has(name + ".qweight") else _linear_fp16(sh, name, dtype)
        if c.kind == "fp16" and quantization == "int8":
            q, s = quant.symmetric_quantize_int8(c.w)
            c = CanonLinear("int8", c.K, c.N, q=q, scales=s)
        return c

    def bias(name):
        return _f16(sh.get(name + ".bias"), name + ".bias", dtype) if sh.has(name + ".bias") else None

    layers = []
    has_bias = False
    # Qwen3: self_attn.{q,k}_norm.weight [hd] per layer.  Either every layer has both or the checkpoint is refused: a norm tensor the
    # step would not apply must never be skipped silently (the logits would be wrong without an error)
    qkn = [(sh.has(f"{pre}layers.{i}.self_attn.q_norm.weight"), sh.has(f"{pre}layers.{i}.self_attn.k_norm.weight")) for i in range(mc.num_layers)]
    if any(a or b for a, b in qkn):
        if not all(a and b for a, b in qkn):
            raise ValueError("checkpoint has per-head q_norm / k_norm tensors on some layers only: not a model this decode path serves")
        mc.qk_norm = True
    elif mc.qk_norm:
        raise ValueError("config.json says model_type 'qwen3' but the checkpoint has no self_attn.q_norm / k_norm tensors")
    for i in range(L):
        p = f"{pre}layers.{i}."
        qkv = _cat_same_kind([lin(p + "self_attn.q_proj"), lin(p + "self_attn.k_proj"), lin(p + "self_attn.v_proj")], p + "self_attn qkv")
        b = [bias(p + "self_attn.q_proj"), bias(p + "self_attn.k_proj"), bias(p + "self_attn.v_proj")]
        has_bias = has_bias or b[0] is not None
        layer = {
            "qkv": qkv, "o": lin(p + "self_attn.o_proj"),
            "gate_up": _cat_same_kind([lin(p + "mlp.gate_proj"), lin(p + "mlp.up_proj")], p + "mlp gate_up"),
            "down": lin(p + "mlp.down_proj"),
            "qkv_bias": torch.cat(b).contiguous() if b[0] is not None else None,
            "input_norm": _f16(sh.get(p + "input_layernorm.weight"), p + "input_layernorm", dtype),
            "post_norm": _f16(sh.get(p + "post_attention_layernorm.weight"), p + "post_attention_layernorm", dtype),
        }
        if mc.qk_norm:
            for k in ("q_norm", "k_norm"):
                w = _f16(sh.get(p + f"self_attn.{k}.weight"), p + f"self_attn.{k}", dtype)
                if w.shape != (mc.hd,):
                    raise ValueError(f"{p}self_attn.{k}.weight: shape {tuple(w.shape)}, expected ({mc.hd},) (one weight per head channel)")
                layer[k] = w
        layers.append(split_layer_tp(layer, mc, tp, rank))
    if mx_flushed[0]:
        logging.getLogger(__name__).warning(
            "MXFP4: %d groups (%d nonzero weights, each below 6 * 2^-14) had a scale below 2^-13 and were flushed to zero", *mx_flushed)
    emb = _f16(sh.get(pre + "embed_tokens.weight"), "embed_tokens", dtype)
    if sh.has("lm_head.weight"):
        head = _f16(sh.get("lm_head.weight"), "lm_head", dtype)
    else:                                                   # tie_word_embeddings (e.g. Qwen2-0.5B)
        head = emb
    V = head.shape[0]                                       # padded-vocab checkpoints: the tensor, not config.json, decides
    if V < mc.vocab or emb.shape[0] < mc.vocab:
        raise ValueError(f"lm_head / embedding rows ({V}, {emb.shape[0]}) < vocab_size {mc.vocab}")
    if tp > 1:                                              # vocab-split lm_head (PyWrappedModel.cc:915-936)
        if V % tp:
            raise ValueError(f"lm_head rows {V} not divisible by tp={tp}")
        head = head[rank * (V // tp):(rank + 1) * (V // tp)]
    mc = ModelConfig(**{**mc.__dict__, "num_layers": L, "qkv_bias": has_bias, "vocab": V})
    if split_embedding and tp > 1:
        from .model import split_embedding_tp
        emb = split_embedding_tp(emb, tp, rank)
    weights = {"layers": layers, "embedding": emb, "final_norm": _f16(sh.get(pre + "norm.weight"), "norm", dtype),
               "lm_head": CanonLinear("fp16", head.shape[1], head.shape[0], w=head.t().contiguous())}
    return (mc.per_rank(tp) if tp > 1 else mc), weights
