"""Qwen3 dense models without a GPU: the CPU reference (tests/qwen3_ref.py) against transformers' own Qwen3ForCausalLM, the
loader on synthetic Qwen3 checkpoints (per-head q_norm / k_norm), and the native entry points of the per-head QK norm."""
import json
import os

import pytest
import torch

from oracle import oracle
from rtp_llm_amd import _C, loader, model

import qwen3_ref
from ckpt_util import write_ckpt


# ------------------------------------------------------------------ (a) the reference against transformers
@pytest.mark.parametrize("over", [{}, {"attention_bias": True}, {"head_dim": 32, "num_attention_heads": 8, "num_key_value_heads": 4}])
def test_reference_matches_transformers_qwen3(over):
    hf = qwen3_ref.hf_tiny_model(seed=3, **over)
    if over.get("attention_bias"):
        with torch.no_grad():   # transformers initialises biases to zero: give them values so that the order bias -> norm is seen
            g = torch.Generator().manual_seed(9)
            for name, p in hf.named_parameters():
                if name.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias")):   # (o_proj's stays zero: no O bias on this path)
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
    ref = qwen3_ref.from_hf(hf, max_pos=64)
    ids = torch.tensor([5, 77, 201, 3, 150, 9, 42], dtype=torch.int32)
    with torch.no_grad():
        want = hf(ids.long().unsqueeze(0)).logits[0].float()
    kv = oracle.OracleKV(hf.config.num_hidden_layers, 1, False)
    got = torch.cat([ref.forward_tokens(ids[t:t + 1], torch.tensor([t], dtype=torch.int32), kv, [0])[1] for t in range(len(ids))])
    assert torch.allclose(got, want, atol=1e-4, rtol=0), float((got - want).abs().max())


def test_reference_differs_without_the_norm():
    """The QK norm matters: the same weights through the Qwen2 decoder (no norm) give other logits."""
    hf = qwen3_ref.hf_tiny_model(seed=4)
    ref = qwen3_ref.from_hf(hf, max_pos=64)
    ids = torch.tensor([1, 2, 3], dtype=torch.int32)
    plain = oracle.OracleDecoder(ref.cfg, ref.w)
    kv1, kv2 = oracle.OracleKV(2, 1, False), oracle.OracleKV(2, 1, False)
    pos = torch.arange(3, dtype=torch.int32)
    a = ref.forward_tokens(ids, pos, kv1, [0, 0, 0])[1]
    b = plain.forward_tokens(ids, pos, kv2, [0, 0, 0])[1]
    assert (a - b).abs().max() > 1e-2


# ------------------------------------------------------------------ (b) the loader
def _synth_qwen3(cfg, kind, seed=0):
    w = model.synth_model(cfg, "fp16" if kind == "fp16" else "w4", "cpu", seed=seed, method="awq" if kind == "awq" else "gptq",
                          zeros="centered")
    return w


def _write_qwen3(tmp, kind, cfg, w, layers_with_norm=None, model_type="qwen3", q_only=False):
    """write_ckpt + the two norm tensors per layer in a third shard (listed in the index)."""
    write_ckpt(str(tmp), kind, cfg, w, extra_cfg={"model_type": model_type} if model_type else None)
    extra = {}
    for i, L in enumerate(w["layers"]):
        if layers_with_norm is not None and i not in layers_with_norm:
            continue
        extra[f"model.layers.{i}.self_attn.q_norm.weight"] = L["q_norm"].clone()
        if not q_only:
            extra[f"model.layers.{i}.self_attn.k_norm.weight"] = L["k_norm"].clone()
    if extra:
        from safetensors.torch import save_file
        save_file(extra, os.path.join(str(tmp), "model-qk-norm.safetensors"))
        idx_path = os.path.join(str(tmp), "model.safetensors.index.json")
        idx = json.load(open(idx_path))
        idx["weight_map"].update({k: "model-qk-norm.safetensors" for k in extra})
        json.dump(idx, open(idx_path, "w"))


# nh * hd != hidden (512 vs 256): the Qwen3-0.6B / 4B situation
CFG = model.ModelConfig("tiny-qwen3", 2, 256, 8, 2, 64, 384, 512, max_pos=128, qk_norm=True)


@pytest.mark.parametrize("kind", ["fp16", "gptq", "awq"])
def test_loader_reads_qwen3_norms(tmp_path, kind):
    w = _synth_qwen3(CFG, kind, seed=1)
    _write_qwen3(tmp_path, kind, CFG, w)
    mc, lw = loader.load_hf_checkpoint(str(tmp_path))
    assert mc.qk_norm and mc.hd == 64 and mc.nh * mc.hd != mc.hidden
    for L, S in zip(lw["layers"], w["layers"]):
        assert torch.equal(L["q_norm"], S["q_norm"]) and torch.equal(L["k_norm"], S["k_norm"])
        assert L["q_norm"].dtype == torch.float16 and L["q_norm"].shape == (CFG.hd,)
        if kind != "fp16":
            assert torch.equal(L["qkv"].q, S["qkv"].q)
        else:
            assert torch.equal(L["qkv"].w, S["qkv"].w)


def test_loader_qwen3_int8_autoquant_and_bf16(tmp_path):
    w = _synth_qwen3(CFG, "fp16", seed=2)
    _write_qwen3(tmp_path, "fp16", CFG, w)
    mc, lw = loader.load_hf_checkpoint(str(tmp_path), quantization="int8")
    assert mc.qk_norm and lw["layers"][0]["qkv"].kind == "int8"
    assert torch.equal(lw["layers"][1]["k_norm"], w["layers"][1]["k_norm"])
    mc, lw = loader.load_hf_checkpoint(str(tmp_path), dtype=torch.bfloat16)
    assert lw["layers"][0]["q_norm"].dtype == torch.bfloat16
    assert torch.equal(lw["layers"][0]["q_norm"], w["layers"][0]["q_norm"].to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["fp16", "gptq"])
def test_loader_qwen3_tp_split_replicates_the_norms(tmp_path, kind):
    w = _synth_qwen3(CFG, kind, seed=3)
    _write_qwen3(tmp_path, kind, CFG, w)
    for rank in range(2):
        mc, lw = loader.load_hf_checkpoint(str(tmp_path), tp=2, rank=rank)
        assert mc.qk_norm and mc.nh == CFG.nh // 2
        for L, S in zip(lw["layers"], w["layers"]):
            assert torch.equal(L["q_norm"], S["q_norm"]) and torch.equal(L["k_norm"], S["k_norm"])
    S = model.split_layer_tp(w["layers"][0], CFG, 2, 1)
    assert S["q_norm"] is w["layers"][0]["q_norm"] and S["k_norm"] is w["layers"][0]["k_norm"]


def test_loader_found_norms_without_model_type(tmp_path):
    """The tensors decide: a config.json without model_type but with q_norm / k_norm tensors loads as Qwen3."""
    w = _synth_qwen3(CFG, "fp16", seed=4)
    _write_qwen3(tmp_path, "fp16", CFG, w, model_type=None)
    mc, lw = loader.load_hf_checkpoint(str(tmp_path))
    assert mc.qk_norm and "q_norm" in lw["layers"][0]


@pytest.mark.parametrize("case", ["some_layers", "q_only", "no_tensors", "wrong_shape"])
def test_loader_refuses_norms_it_cannot_serve(tmp_path, case):
    w = _synth_qwen3(CFG, "fp16", seed=5)
    if case == "some_layers":
        _write_qwen3(tmp_path, "fp16", CFG, w, layers_with_norm={0})
    elif case == "q_only":
        _write_qwen3(tmp_path, "fp16", CFG, w, q_only=True)
    elif case == "no_tensors":
        _write_qwen3(tmp_path, "fp16", CFG, w, layers_with_norm=set())
    else:
        for L in w["layers"]:
            L["q_norm"] = torch.ones(CFG.hd * 2, dtype=torch.float16)
        _write_qwen3(tmp_path, "fp16", CFG, w)
    with pytest.raises(ValueError):
        loader.load_hf_checkpoint(str(tmp_path))


def test_loader_refuses_qwen3_moe():
    with pytest.raises(NotImplementedError):
        loader.config_from_hf({"model_type": "qwen3_moe", "num_attention_heads": 4, "num_hidden_layers": 1, "hidden_size": 64,
                               "intermediate_size": 64, "vocab_size": 64})


def test_config_from_hf_qwen3_head_dim():
    mc, _ = loader.config_from_hf({"model_type": "qwen3", "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128,
                                   "num_hidden_layers": 28, "hidden_size": 1024, "intermediate_size": 3072, "vocab_size": 151936})
    assert mc.qk_norm and mc.hd == 128 and mc.nh * mc.hd == 2048 != mc.hidden


def test_synth_and_preset():
    q = model.QWEN3_8B
    assert (q.num_layers, q.hidden, q.nh, q.nkv, q.hd, q.inter, q.vocab, q.rope_theta, q.qkv_bias, q.qk_norm) == \
        (36, 4096, 32, 8, 128, 12288, 151936, 1e6, False, True)
    w = model.synth_model(CFG, "w4", "cpu", seed=0)
    qn = w["layers"][0]["q_norm"]
    assert qn.shape == (CFG.hd,) and not torch.all(qn == 1) and (qn.float() - 1).abs().max() < 2
    # a config without the norm keeps its weights exactly (the norms are drawn last)
    from dataclasses import replace
    a = model.synth_model(replace(CFG, qk_norm=False, num_layers=1), "w4", "cpu", seed=0)
    b = model.synth_model(replace(CFG, num_layers=1), "w4", "cpu", seed=0)
    assert "q_norm" not in a["layers"][0] and torch.equal(a["layers"][0]["qkv"].q, b["layers"][0]["qkv"].q)


# ------------------------------------------------------------------ (c) native entry points
def test_native_library_exports_the_qk_norm_entry_points():
    import ctypes
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ("mi355_rope_kv_write_rows_qk_norm", "mi355_qk_rmsnorm", "mi355_decoder_set_qk_norm"):
        assert hasattr(lib, name), name
    assert hasattr(_C.lib(), "mi355_decoder_set_qk_norm")


def test_qk_norm_entry_points_check_arguments_without_a_gpu():
    l = _C.lib()
    assert l.mi355_qk_rmsnorm(None, 1, 384, 4, 1, 64, None, None, 1e-6, _C.ACT_F16, None) == -1
    assert b"qk_rmsnorm" in l.mi355_last_error()
    assert l.mi355_decoder_set_qk_norm(None, None, None) == -1
    kv = _C.KVLayer(0, 0, _C.KV_FP16, 16, 1, 64, 1, _C.ACT_F16)
    assert l.mi355_rope_kv_write_rows_qk_norm(None, None, 0, 384, None, None, None, 1e-6, None, 64, 64, None, None, 1, 1, 1, 4,
                                              ctypes_byref(kv), None, None, None) == -1


def ctypes_byref(x):
    import ctypes
    return ctypes.byref(x)
