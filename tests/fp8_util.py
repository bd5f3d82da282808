"""FP8 (e4m3, 128 x 128 block scales) helpers for the tests: the reference weights, an independent index computation of the tile
image, and a writer of synthetic checkpoints in the published on-disk form (`quant_method: "fp8"`: `.weight` float8_e4m3fn
[out, in] + `.weight_scale_inv` fp32 [ceil(out/128), ceil(in/128)])."""
import json
import os

import torch
from safetensors.torch import save_file

from rtp_llm_amd.model import CanonLinear


def w_ref(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp64 [K, N]: codes.view(float8_e4m3fn).double() * scale[k // 128][n] -- the reference of every FP8 test."""
    K = codes.shape[0]
    return codes.view(torch.float8_e4m3fn).double() * scales.double().repeat_interleave(128, dim=0)[:K]


def dense_canonical(w: dict, dtype=torch.float32) -> dict:
    """Canonical weight dict with every 'fp8' linear replaced by its dequantised weights (kind 'fp16', w = W_ref): what the
    reference decoders (oracle.OracleDecoder, qwen3_ref.from_canonical) take, since they only read `.w.float()` of such a linear."""
    def conv(v):
        if isinstance(v, CanonLinear) and v.kind == "fp8":
            return CanonLinear("fp16", v.K, v.N, w=w_ref(v.q, v.scales).to(dtype))
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, list):
            return [conv(x) for x in v]
        return v
    return conv(w)


def image_offset(k: int, n: int, K_pad: int) -> int:
    """Byte offset of weight (k, n) in the W8 tile image, from the header comment of include/mi355_decode.h: tile (nt, c) at
    ((nt * K_pad/128 + c) * 2) * 1024; wave-load p holds k-steps 2p and 2p + 1; lane l = i + 16 q owns column 16 nt + i and rows
    128 c + 32 s + 8 q + e; a lane's 16 bytes are step 2p (8 bytes, e = 0..7) then step 2p + 1."""
    nt, i = divmod(n, 16)
    c, r = divmod(k, 128)
    s, r = divmod(r, 32)
    q, e = divmod(r, 8)
    p, h = divmod(s, 2)
    lane = q * 16 + i
    return ((nt * (K_pad // 128) + c) * 2 + p) * 1024 + lane * 16 + h * 8 + e


def block_scales_of(c: CanonLinear) -> torch.Tensor:
    """[ceil(N/128), ceil(K/128)] (the checkpoint's [out, in] orientation) of a canonical fp8 linear whose per-column scales are
    constant inside every 128-column block starting at column 0."""
    s = c.scales
    bs = s[:, ::128]
    assert torch.equal(bs.repeat_interleave(128, dim=1)[:, : c.N], s), "scales are not 128-column block constant"
    return bs.t().contiguous()


def write_fp8_ckpt(tmp, cfg, canon, not_converted=(), quant_cfg=None, model_type="qwen3"):
    """canon: synth_model(kind='fp8') layout.  Modules whose HF name ends with an entry of `not_converted` are stored as fp16
    tensors of their dequantised weights and listed in modules_to_not_convert.  Returns the dict of tensors written."""
    t = {}
    hd, nh, nkv, I = cfg.hd, cfg.nh, cfg.nkv, cfg.inter

    def put(name, c):
        if any(name.endswith(m) for m in not_converted):
            t[name + ".weight"] = w_ref(c.q, c.scales).t().contiguous().half()
            return
        t[name + ".weight"] = c.q.t().contiguous().view(torch.float8_e4m3fn)
        t[name + ".weight_scale_inv"] = block_scales_of(c).float()

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
    qc = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
    if not_converted:
        qc["modules_to_not_convert"] = sorted({n[: -len(".weight")] for n in t if n.endswith(".weight") and any(n[: -len(".weight")].endswith(m) for m in not_converted)})
    if quant_cfg is not None:
        qc = quant_cfg
    hf = {"model_type": model_type, "hidden_size": cfg.hidden, "num_hidden_layers": cfg.num_layers, "num_attention_heads": nh,
          "num_key_value_heads": nkv, "intermediate_size": I, "vocab_size": cfg.vocab, "rope_theta": cfg.rope_theta,
          "rms_norm_eps": cfg.rms_eps, "max_position_embeddings": cfg.max_pos, "head_dim": hd, "quantization_config": qc}
    json.dump(hf, open(os.path.join(tmp, "config.json"), "w"))
    return t
