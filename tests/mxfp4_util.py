"""MXFP4 (e2m1 codes, one e8m0 scale byte per 32 rows of a column) helpers for the tests: the reference weights, an independent
index computation of the tile image and of the meta plane, and a writer of synthetic checkpoints in the Quark on-disk form
(`quant_method: "quark"`: `.weight` uint8 [out, in/2], low nibble = even input index, + `.weight_scale` uint8 [out, in/32])."""
import json
import os

import torch
from safetensors.torch import save_file

from rtp_llm_amd.model import CanonLinear
from rtp_llm_amd.quant import E2M1_VALUES


def w_ref(codes: torch.Tensor, scale_bytes: torch.Tensor) -> torch.Tensor:
    """fp64 [K, N]: E2M1_VALUES[code].double() * 2.0 ** (byte - 127) -- the reference of every MXFP4 test."""
    sc = (2.0 ** (scale_bytes.double() - 127)).repeat_interleave(32, dim=0)
    return E2M1_VALUES[codes.long()].double() * sc


def dense_canonical(w: dict, dtype=torch.float32) -> dict:
    """Canonical weight dict with every 'mxfp4' linear replaced by its dequantised weights (kind 'fp16', w = W_ref): what the
    reference decoders (oracle.OracleDecoder, qwen3_ref.from_canonical) take, since they only read `.w.float()` of such a linear."""
    def conv(v):
        if isinstance(v, CanonLinear) and v.kind == "mxfp4":
            return CanonLinear("fp16", v.K, v.N, w=w_ref(v.q, v.scales).to(dtype))
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, list):
            return [conv(x) for x in v]
        return v
    return conv(w)


def image_position(k: int, n: int, K_pad: int):
    """(dword index, bit offset) of the code of weight (k, n) in the MXFP4 tile image, from the header comment of
    include/mi355_decode.h: tile (nt, c) is 1024 bytes at (nt * K_pad/128 + c) * 1024; lane l = i + 16 q owns column 16 nt + i and
    rows 128 c + 32 s + 8 q + e; dword s of the lane's 16 bytes is k-step s; code e sits at bit 4 e."""
    nt, i = divmod(n, 16)
    c, r = divmod(k, 128)
    s, r = divmod(r, 32)
    q, e = divmod(r, 8)
    lane = q * 16 + i
    return ((nt * (K_pad // 128) + c) * 64 + lane) * 4 + s, 4 * e


def meta_position(k: int, n: int, N_pad: int):
    """(dword index, bit offset) of the scale byte of weight (k, n): meta[c * N_pad + n], byte s = the group of rows 128 c + 32 s .. + 31."""
    c, r = divmod(k, 128)
    return c * N_pad + n, 8 * (r // 32)


def to_quark(c: CanonLinear):
    """(weight uint8 [N, K/2], weight_scale uint8 [N, K/32]) of a canonical mxfp4 linear, written out here independently of the
    package: byte j of row n holds input 2 j in its low nibble and input 2 j + 1 in its high nibble."""
    q = c.q.t().contiguous()                                  # [N, K]
    return (q[:, 0::2] | (q[:, 1::2] << 4)).contiguous(), c.scales.t().contiguous()


QUARK_CFG = {
    "quant_method": "quark",
    "global_quant_config": {
        "weight": {"dtype": "fp4", "qscheme": "per_group", "group_size": 32, "scale_format": "e8m0", "is_dynamic": False, "ch_axis": -1,
                   "observer_cls": "PerBlockMXObserver", "round_method": "half_even", "scale_type": "float", "symmetric": None},
        "input_tensors": {"dtype": "fp4", "qscheme": "per_group", "group_size": 32, "scale_format": "e8m0", "is_dynamic": True, "ch_axis": -1},
        "output_tensors": None, "bias": None, "target_device": None,
    },
    "layer_quant_config": {}, "layer_type_quant_config": {}, "exclude": ["lm_head"], "export": {"pack_method": "reorder", "weight_format": "real_quantized"},
}


def quark_cfg(**weight_changes):
    cfg = json.loads(json.dumps(QUARK_CFG))
    cfg["global_quant_config"]["weight"].update(weight_changes)
    return cfg


def write_mxfp4_ckpt(tmp, cfg, canon, excluded=(), quant_cfg=None, model_type="qwen3"):
    """canon: synth_model(kind='mxfp4') layout.  Modules whose HF name ends with an entry of `excluded` are stored as fp16 tensors
    of their dequantised weights and listed in `exclude` (as glob patterns "*<suffix>").  Returns the dict of tensors written."""
    t = {}
    hd, nh, nkv, I = cfg.hd, cfg.nh, cfg.nkv, cfg.inter

    def put(name, c):
        if any(name.endswith(m) for m in excluded):
            t[name + ".weight"] = w_ref(c.q, c.scales).t().contiguous().half()
            return
        t[name + ".weight"], t[name + ".weight_scale"] = to_quark(c)

    for i, L in enumerate(canon["layers"]):
        p = f"model.layers.{i}."
        qkv, gu = L["qkv"], L["gate_up"]
        put(p + "self_attn.q_proj", qkv.cols(0, nh * hd))
        put(p + "self_attn.k_proj", qkv.cols(nh * hd, (nh + nkv) * hd))
        put(p + "self_attn.v_proj", qkv.cols((nh + nkv) * hd, (nh + 2 * nkv) * hd))
        if L.get("qkv_bias") is not None:
            b = L["qkv_bias"]
            t[p + "self_attn.q_proj.bias"], t[p + "self_attn.k_proj.bias"], t[p + "self_attn.v_proj.bias"] = \
                b[: nh * hd].clone(), b[nh * hd:(nh + nkv) * hd].clone(), b[(nh + nkv) * hd:].clone()
        put(p + "self_attn.o_proj", L["o"])
        put(p + "mlp.gate_proj", gu.cols(0, I)); put(p + "mlp.up_proj", gu.cols(I, 2 * I))
        put(p + "mlp.down_proj", L["down"])
        t[p + "input_layernorm.weight"], t[p + "post_attention_layernorm.weight"] = L["input_norm"], L["post_norm"]
        for k in ("q_norm", "k_norm"):
            if L.get(k) is not None:
                t[p + f"self_attn.{k}.weight"] = L[k]
    t["model.embed_tokens.weight"], t["model.norm.weight"] = canon["embedding"], canon["final_norm"]
    t["lm_head.weight"] = canon["lm_head"].w.t().contiguous()
    save_file({k: v.contiguous() for k, v in t.items()}, os.path.join(tmp, "model.safetensors"))
    qc = quark_cfg() if quant_cfg is None else quant_cfg
    if quant_cfg is None and excluded:
        qc["exclude"] = ["lm_head"] + ["*" + m for m in excluded]
    hf = {"model_type": model_type, "hidden_size": cfg.hidden, "num_hidden_layers": cfg.num_layers, "num_attention_heads": nh,
          "num_key_value_heads": nkv, "intermediate_size": I, "vocab_size": cfg.vocab, "rope_theta": cfg.rope_theta,
          "rms_norm_eps": cfg.rms_eps, "max_position_embeddings": cfg.max_pos, "head_dim": hd, "quantization_config": qc}
    json.dump(hf, open(os.path.join(tmp, "config.json"), "w"))
    return t
