"""CPU reference of a Qwen3 dense decoder, built from the oracle primitives (oracle.oracle: rmsnorm, linear, apply_rope,
attention_decode, OracleKV).  It is OracleDecoder.forward_tokens with one step inserted: the per-head RMSNorm of every Q and K
head between the QKV projection and RoPE (Qwen3Attention: q_norm / k_norm over head_dim; the reference's FusedQKRMSNorm).

Weights as for OracleDecoder (dense [K, N] fp32 linears), plus per layer "q_norm" / "k_norm" [hd]."""
import math
from typing import List, Optional

import torch

from oracle import oracle


def qk_norm(qkv: torch.Tensor, q_norm: torch.Tensor, k_norm: torch.Tensor, nh: int, nkv: int, hd: int, eps: float) -> torch.Tensor:
    """Packed rows [T, (nh + 2 nkv) hd] -> the same with every Q head oracle.rmsnorm'ed by q_norm and every K head by k_norm."""
    T = qkv.shape[0]
    q = oracle.rmsnorm(qkv[:, : nh * hd].reshape(T, nh, hd), q_norm, eps).reshape(T, nh * hd)
    k = oracle.rmsnorm(qkv[:, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd), k_norm, eps).reshape(T, nkv * hd)
    return torch.cat([q.to(qkv.dtype), k.to(qkv.dtype), qkv[:, (nh + nkv) * hd:]], dim=1)


class Qwen3RefDecoder(oracle.OracleDecoder):
    """Qwen3 dense: embedding -> N x [RMSNorm, QKV(+bias), per-head QK RMSNorm, RoPE, KV append, attention, O, +res, RMSNorm,
    gate_up, SiLU*mul, down, +res] -> RMSNorm -> lm_head."""

    def forward_tokens(self, token_ids: torch.Tensor, positions: torch.Tensor, kv: oracle.OracleKV, seq_idx: List[int],
                       trace: Optional[list] = None):
        c, w = self.cfg, self.w
        nh, nkv, hd, eps = c["nh"], c["nkv"], c["hd"], c["rms_eps"]
        h = w["embedding"][token_ids.long()]
        T = h.shape[0]
        for l in range(c["num_layers"]):
            L = w["layers"][l]
            x = oracle.rmsnorm(h, L["input_norm"], eps)
            qkv = oracle.linear(x, L["qkv"], L.get("qkv_bias"))
            qkv = qk_norm(qkv, L["q_norm"], L["k_norm"], nh, nkv, hd, eps)
            qh = qkv[:, : nh * hd].reshape(T, nh, hd)
            kh = qkv[:, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd)
            vh = qkv[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
            qh, kh = oracle.apply_rope(qh, positions, self.cos_sin), oracle.apply_rope(kh, positions, self.cos_sin)
            attn = torch.empty(T, nh * hd, dtype=h.dtype)
            for t in range(T):
                b = seq_idx[t]
                kv.append(l, b, kh[t], vh[t])
                K, V, ks, vs = kv.get(l, b)
                attn[t] = oracle.attention_decode(qh[t], K, V, 1.0 / math.sqrt(hd), ks, vs).reshape(-1)
            h = h + oracle.linear(attn, L["o"])
            if trace is not None:
                trace.append((l, "attn", h.clone()))
            x = oracle.rmsnorm(h, L["post_norm"], eps)
            h = h + oracle.linear(oracle.silu_mul(oracle.linear(x, L["gate_up"])), L["down"])
            if trace is not None:
                trace.append((l, "mlp", h.clone()))
        hn = oracle.rmsnorm(h, w["final_norm"], eps)
        return hn, oracle.linear(hn, w["lm_head"], out_f32=True)


def dense(c) -> torch.Tensor:
    """CanonLinear -> fp32 [K, N] (what the oracle's linear takes)."""
    if c.kind == "fp16":
        return c.w.float()
    if c.kind == "int8":
        return oracle.dequant_int8(c.q, c.scales)
    return oracle.dequant_groupwise(c.q, c.z_eff, c.scales, c.group_size)


def from_canonical(cfg, w) -> Qwen3RefDecoder:
    """Reference decoder over a canonical weight dict (model.synth_model / loader.load_hf_checkpoint layout, tp = 1)."""
    ow = {"embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": dense(w["lm_head"]),
          "layers": [{"input_norm": L["input_norm"], "post_norm": L["post_norm"], "qkv_bias": L["qkv_bias"], "q_norm": L["q_norm"],
                      "k_norm": L["k_norm"], **{k: dense(L[k]) for k in ("qkv", "o", "gate_up", "down")}} for L in w["layers"]]}
    return Qwen3RefDecoder({**cfg.__dict__}, ow)


def from_hf(hf_model, max_pos: int) -> Qwen3RefDecoder:
    """Reference decoder over the weights of a transformers Qwen3ForCausalLM (fp32 copies; HF linears are [out, in])."""
    hc = hf_model.config
    sd = {k: v.detach().float().clone() for k, v in hf_model.state_dict().items()}
    layers = []
    for i in range(hc.num_hidden_layers):
        p = f"model.layers.{i}."
        qkv = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0).t().contiguous()
        bias = torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"]) if (p + "self_attn.q_proj.bias") in sd else None
        layers.append({"qkv": qkv, "qkv_bias": bias, "o": sd[p + "self_attn.o_proj.weight"].t().contiguous(),
                       "gate_up": torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], dim=0).t().contiguous(),
                       "down": sd[p + "mlp.down_proj.weight"].t().contiguous(),
                       "input_norm": sd[p + "input_layernorm.weight"], "post_norm": sd[p + "post_attention_layernorm.weight"],
                       "q_norm": sd[p + "self_attn.q_norm.weight"], "k_norm": sd[p + "self_attn.k_norm.weight"]})
    head = sd["lm_head.weight"] if "lm_head.weight" in sd else sd["model.embed_tokens.weight"]
    cfg = {"num_layers": hc.num_hidden_layers, "nh": hc.num_attention_heads, "nkv": hc.num_key_value_heads, "hd": hc.head_dim,
           "rms_eps": hc.rms_norm_eps, "rope_theta": _rope_theta(hc), "max_pos": max_pos, "rope_scaling": None}
    return Qwen3RefDecoder(cfg, {"embedding": sd["model.embed_tokens.weight"], "final_norm": sd["model.norm.weight"],
                                 "lm_head": head.t().contiguous(), "layers": layers})


def _rope_theta(hc) -> float:
    rp = getattr(hc, "rope_parameters", None)   # newer transformers keep it there
    if isinstance(rp, dict) and "rope_theta" in rp:
        return float(rp["rope_theta"])
    return float(hc.rope_theta)


def hf_tiny_config(**over):
    """A small transformers Qwen3Config (fp32, eager attention, untied head); nh * hd != hidden on purpose."""
    from transformers import Qwen3Config
    kw = dict(vocab_size=256, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
              head_dim=64, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=256, tie_word_embeddings=False,
              attention_bias=False, use_sliding_window=False)
    kw.update(over)
    cfg = Qwen3Config(**kw)
    cfg._attn_implementation = "eager"
    return cfg


def hf_tiny_model(seed: int = 0, **over):
    """Qwen3ForCausalLM at hf_tiny_config, fp32, with every norm weight (q_norm / k_norm included) randomised around 1."""
    from transformers import Qwen3ForCausalLM
    torch.manual_seed(seed)
    m = Qwen3ForCausalLM(hf_tiny_config(**over)).float().eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
    return m
