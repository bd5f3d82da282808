"""FP8 (e4m3, 128 x 128 block scales) weights on the host: the packer against an independent index computation of the tile image,
the fp32 meta plane, the loader on a synthetic `quant_method: "fp8"` checkpoint (merges, tp shards, modules_to_not_convert, the
refusals), and the strategy dispatch.  No GPU."""
import ctypes
import json
import os

import pytest
import torch

from rtp_llm_amd import _C, loader, model, quant
from rtp_llm_amd.linear import LinearFactory, Mi355Fp8Linear

import fp8_util

TOY = model.ModelConfig("toy-qwen3-fp8", 2, 256, 4, 2, 64, 512, 384, max_pos=128, qkv_bias=False, qk_norm=True)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _codes(K, N, seed):
    c = torch.randint(0, 256, (K, N), generator=_gen(seed), dtype=torch.uint8)
    return torch.where((c & 0x7F) == 0x7F, c & 0xF8, c)      # no NaN codes


def test_every_finite_code_is_exact_in_fp16_and_bf16():
    """The numerics contract: the byte enters the MFMA as the exact 16-bit image of its value."""
    c = torch.arange(256, dtype=torch.uint8)
    fin = (c & 0x7F) != 0x7F
    v = c.view(torch.float8_e4m3fn).float()[fin]
    assert int(fin.sum()) == 254
    assert torch.equal(v.half().float(), v) and torch.equal(v.bfloat16().float(), v)


def test_weight_struct_has_wkind_and_keeps_its_size():
    assert ctypes.sizeof(_C.Weight) == 48 and _C.Weight.wkind.offset == 44
    assert _C.ABI_VERSION == 5 and (_C.WKIND_INT, _C.WKIND_FP8_E4M3) == (0, 1)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355_decode.h")).read()
    assert "#define MI355_ABI_VERSION 5" in hdr and "MI355_WKIND_FP8_E4M3 = 1" in hdr


def test_pack_fp8_block_tile_image_and_meta():
    K, N = 256, 48
    codes = _codes(K, N, 1)
    scales = torch.rand(K // 128, N, generator=_gen(2)) * 1e-3 + 1e-6
    p = quant.pack_fp8_block(codes, scales)
    assert (p.wbits, p.group_size, p.wkind, p.K, p.N, p.K_pad, p.N_pad) == (8, 128, 1, K, N, 256, 48)
    img = p.qweight.view(torch.uint8)
    assert img.numel() == K * N
    want = torch.empty(K * N, dtype=torch.uint8)
    for k in range(K):
        for n in range(N):
            want[fp8_util.image_offset(k, n, 256)] = codes[k, n]
    assert torch.equal(img, want)
    # the raw bytes in pack_w8's tile order (which stores q + 128)
    assert torch.equal(img, quant.pack_w8((codes.to(torch.int16) - 128).to(torch.int8)))
    meta = p.meta.view(torch.float32)
    assert meta.shape == (2, 48) and torch.equal(meta, scales)


def test_pack_fp8_block_padding():
    K, N = 200, 40                                           # K padded to 256 with code 0, N to 48 with code 0 / scale 0
    codes, scales = _codes(K, N, 3), torch.rand(2, N, generator=_gen(4)) + 0.5
    p = quant.pack_fp8_block(codes, scales)
    assert (p.K_pad, p.N_pad) == (256, 48)
    img, meta = p.qweight.view(torch.uint8), p.meta.view(torch.float32)
    for k, n in ((199, 39), (0, 0), (128, 17)):
        assert img[fp8_util.image_offset(k, n, 256)] == codes[k, n]
    for k, n in ((200, 0), (255, 39), (0, 40), (255, 47)):
        assert img[fp8_util.image_offset(k, n, 256)] == 0
    assert torch.equal(meta[:, :N], scales) and bool((meta[:, N:] == 0).all())
    with pytest.raises(ValueError):
        quant.pack_fp8_block(torch.full((128, 16), 0x7F, dtype=torch.uint8), torch.ones(1, 16))


def test_quant_fp8_block_round_trip():
    w = torch.randn(256, 200, generator=_gen(5)) * 0.05
    w[:128, :128] = 0                                       # an all-zero block: scale 1, codes 0
    codes, scales = quant.quant_fp8_block(w)
    assert codes.dtype == torch.uint8 and scales.shape == (2, 200) and scales.dtype == torch.float32
    assert bool((scales[0, :128] == 1).all()) and bool((codes[:128, :128] == 0).all())
    amax = w[128:, 128:].abs().max()
    assert torch.allclose(scales[1, 128:], (amax / 448).expand(72))
    assert not bool(((codes & 0x7F) == 0x7F).any())
    err = (fp8_util.w_ref(codes, scales).float() - w).abs()
    assert float(err.max()) <= float(w.abs().max()) * 2 ** -4   # 3 mantissa bits: half an ulp is 2^-4 relative
    assert torch.equal(quant.dequant_fp8(codes, scales), fp8_util.w_ref(codes, scales).float())


def test_canon_linear_fp8_ops():
    c = model.synth_linear(256, 384, "fp8", "cpu", _gen(6))
    assert c.kind == "fp8" and c.group_size == 128 and c.q.dtype == torch.uint8 and c.scales.shape == (2, 384) and c.z_eff is None
    W = fp8_util.w_ref(c.q, c.scales)
    assert torch.equal(fp8_util.w_ref(c.cols(64, 200).q, c.cols(64, 200).scales), W[:, 64:200])
    r = c.rows(128, 256)
    assert r.K == 128 and torch.equal(fp8_util.w_ref(r.q, r.scales), W[128:])
    with pytest.raises(AssertionError):
        c.rows(64, 256)
    pc, pr = c.pad_cols(16), c.pad_rows(128)
    assert pc.N == 400 and bool((fp8_util.w_ref(pc.q, pc.scales)[:, 384:] == 0).all())
    assert pr.K == 384 and bool((fp8_util.w_ref(pr.q, pr.scales)[256:] == 0).all())
    cat = model.CanonLinear.cat_cols([c.cols(0, 128), c.cols(128, 384)])
    assert torch.equal(cat.q, c.q) and torch.equal(cat.scales, c.scales) and cat.kind == "fp8"
    p = c.pack()
    assert p.wkind == 1 and p.wbits == 8 and p.group_size == 128
    gu = c.pack(gate_up=True)                                 # interleaved (gate, up) columns: codes and scales move together
    assert torch.equal(gu.meta.view(torch.float32), quant.interleave_gate_up(c.scales))


def _toy(seed=7):
    return model.synth_model(TOY, "fp8", "cpu", seed=seed)


def test_loader_round_trip(tmp_path):
    w = _toy()
    fp8_util.write_fp8_ckpt(str(tmp_path), TOY, w)
    cfg, lw = loader.load_hf_checkpoint(str(tmp_path))
    assert cfg.qk_norm and cfg.num_layers == 2 and not cfg.qkv_bias
    assert lw["lm_head"].kind == "fp16"
    for L, R in zip(lw["layers"], w["layers"]):
        for k in ("qkv", "o", "gate_up", "down"):
            assert L[k].kind == "fp8" and L[k].group_size == 128 and (L[k].K, L[k].N) == (R[k].K, R[k].N)
            assert L[k].q.dtype == torch.uint8 and torch.equal(L[k].q, R[k].q), k
            assert L[k].scales.dtype == torch.float32 and torch.equal(L[k].scales, R[k].scales), k
        assert torch.equal(L["q_norm"], R["q_norm"])
    # the merged tensors equal their parts
    L, R = lw["layers"][0], w["layers"][0]
    nq, nk = TOY.nh * TOY.hd, TOY.nkv * TOY.hd
    for lo, hi in ((0, nq), (nq, nq + nk), (nq + nk, nq + 2 * nk)):
        assert torch.equal(L["qkv"].cols(lo, hi).q, R["qkv"].q[:, lo:hi])
    assert torch.equal(L["gate_up"].cols(TOY.inter, 2 * TOY.inter).scales, R["gate_up"].scales[:, TOY.inter:])
    # max_layers and bf16 activations: codes and scales are untouched, the 16-bit tensors follow the dtype
    cfg1, lw1 = loader.load_hf_checkpoint(str(tmp_path), max_layers=1, dtype=torch.bfloat16)
    assert cfg1.num_layers == 1 and len(lw1["layers"]) == 1 and lw1["layers"][0]["input_norm"].dtype == torch.bfloat16
    assert torch.equal(lw1["layers"][0]["down"].q, w["layers"][0]["down"].q) and lw1["layers"][0]["down"].scales.dtype == torch.float32


def test_loader_tp2_shards_reassemble(tmp_path):
    w = _toy(8)
    fp8_util.write_fp8_ckpt(str(tmp_path), TOY, w)
    shards = [loader.load_hf_checkpoint(str(tmp_path), tp=2, rank=r)[1] for r in range(2)]
    R = w["layers"][1]
    W = {k: fp8_util.w_ref(R[k].q, R[k].scales) for k in ("qkv", "o", "gate_up", "down")}
    S = [{k: fp8_util.w_ref(s["layers"][1][k].q, s["layers"][1][k].scales) for k in W} for s in shards]
    hd, nh, nkv, I = TOY.hd, TOY.nh, TOY.nkv, TOY.inter
    nq, nk = nh * hd, nkv * hd
    q = torch.cat([s["qkv"][:, : nq // 2] for s in S], dim=1)
    k = torch.cat([s["qkv"][:, nq // 2: nq // 2 + nk // 2] for s in S], dim=1)
    v = torch.cat([s["qkv"][:, nq // 2 + nk // 2:] for s in S], dim=1)
    assert torch.equal(torch.cat([q, k, v], dim=1), W["qkv"])
    assert torch.equal(torch.cat([s["o"] for s in S], dim=0), W["o"])
    assert torch.equal(torch.cat([s["down"] for s in S], dim=0), W["down"])
    g = torch.cat([s["gate_up"][:, : I // 2] for s in S], dim=1)
    u = torch.cat([s["gate_up"][:, I // 2:] for s in S], dim=1)
    assert torch.equal(torch.cat([g, u], dim=1), W["gate_up"])
    assert all(s["layers"][1]["o"].kind == "fp8" and s["layers"][1]["o"].K == nq // 2 for s in shards)


def test_loader_modules_to_not_convert(tmp_path):
    w = _toy(9)
    fp8_util.write_fp8_ckpt(str(tmp_path), TOY, w, not_converted=("self_attn.o_proj", "mlp.down_proj"))
    _, lw = loader.load_hf_checkpoint(str(tmp_path))
    for L, R in zip(lw["layers"], w["layers"]):
        assert L["o"].kind == "fp16" and L["down"].kind == "fp16" and L["qkv"].kind == "fp8" and L["gate_up"].kind == "fp8"
        assert torch.equal(L["o"].w, fp8_util.w_ref(R["o"].q, R["o"].scales).half())


def _rewrite_config(tmp, **changes):
    p = os.path.join(tmp, "config.json")
    cfg = json.load(open(p))
    qc = cfg["quantization_config"]
    for k, v in changes.items():
        if v is None:
            qc.pop(k, None)
        else:
            qc[k] = v
    json.dump(cfg, open(p, "w"))


def test_loader_refusals(tmp_path):
    w = _toy(10)
    t = fp8_util.write_fp8_ckpt(str(tmp_path), TOY, w)
    for field, value in (("fmt", "e5m2"), ("weight_block_size", [64, 64]), ("weight_block_size", None), ("activation_scheme", "static")):
        _rewrite_config(str(tmp_path), **{field: value})
        with pytest.raises(NotImplementedError, match=field):
            loader.load_hf_checkpoint(str(tmp_path))
        _rewrite_config(str(tmp_path), fmt="e4m3", weight_block_size=[128, 128], activation_scheme="dynamic")
    _rewrite_config(str(tmp_path), fmt=None)                 # fmt absent: accepted
    loader.load_hf_checkpoint(str(tmp_path), max_layers=1)
    # a NaN code in a weight
    from safetensors.torch import save_file
    name = "model.layers.0.mlp.down_proj.weight"
    bad = t[name].view(torch.uint8).clone()
    bad[3, 5] = 0xFF
    save_file({**{k: v.contiguous() for k, v in t.items()}, name: bad.view(torch.float8_e4m3fn)}, os.path.join(str(tmp_path), "model.safetensors"))
    with pytest.raises(ValueError, match="NaN"):
        loader.load_hf_checkpoint(str(tmp_path))
    # per-tensor scales (no weight_scale_inv)
    t2 = {k: v.contiguous() for k, v in t.items() if k != "model.layers.0.mlp.down_proj.weight_scale_inv"}
    save_file(t2, os.path.join(str(tmp_path), "model.safetensors"))
    with pytest.raises(NotImplementedError, match="weight_scale_inv"):
        loader.load_hf_checkpoint(str(tmp_path))


def test_fp8_strategy_is_the_only_match():
    c = model.synth_linear(256, 256, "fp8", "cpu", _gen(11))
    w8 = c.q.view(torch.float8_e4m3fn)
    for scales in (c.scales, c.scales[:, ::128].contiguous()):
        hits = [s.__name__ for s in LinearFactory._strategies if s.can_handle(None, w8, scales)]
        assert hits == ["Mi355Fp8Linear"], hits
    assert not Mi355Fp8Linear.can_handle(None, w8, None) and not Mi355Fp8Linear.can_handle(None, c.q, c.scales)
    assert not Mi355Fp8Linear.can_handle(None, w8, torch.ones(256))
    # both scale forms pack to the same image
    a = LinearFactory.create_linear(w8, None, c.scales)
    b = LinearFactory.create_linear(w8, None, c.scales[:, ::128].contiguous())
    assert isinstance(a, Mi355Fp8Linear) and torch.equal(a.packed.meta, b.packed.meta) and torch.equal(a.packed.qweight, b.packed.qweight)
    assert a.packed.wkind == 1
    from rtp_llm_amd.linear import STRATEGY_IMPLS, QuantConfig
    assert "Mi355Fp8Linear" in [n for n, _ in STRATEGY_IMPLS] and QuantConfig(method="fp8").is_quanted()


def test_predicates_and_argument_checks_refuse_the_kind():
    """No image / fused launch takes wkind = 1 (an FP8 image must never be decoded as INT8 g128), and the kind only goes with
    wbits 8 / group_size 128.  Host code of the library: no GPU needed."""
    import ctypes as C
    lib = _C.lib()
    mk = lambda K, N, wbits, gs, kind: _C.Weight(1 << 20, 1 << 21, wbits, K, N, K, N, gs, _C.ACT_F16, kind)   # pointers are never read here
    for name, extra in (("mi355_fullk_weight_ok", ()), ("mi355_fullk64_weight_ok", ()), ("mi355_gemm_wide_direct_ok", ()),
                        ("mi355_fullk64_publish_ok", ()), ("mi355_fullk64_qkv_ok", (128,))):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, [C.POINTER(_C.Weight)] + [C.c_int] * len(extra)
        for wbits, gs in ((8, 128), (8, 0), (4, 128)):       # whatever else the struct says, the kind decides
            assert f(C.byref(mk(3584, 37888, wbits, gs, _C.WKIND_FP8_E4M3)), *extra) == 0, (name, wbits, gs)
    assert lib.mi355_fullk64_weight_ok(C.byref(mk(3584, 4608, 8, 0, _C.WKIND_INT))) == 1      # the integer kinds are untouched
    plan = lib.mi355_gemm_splitk64_plan
    plan.restype, plan.argtypes = C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)]
    assert plan(64, 224, 148, 0x108, 128, 16, None) < 0      # the library's format code of an FP8 weight
    dplan = lib.mi355_gemm_splitk64_direct_plan
    dplan.restype, dplan.argtypes = C.c_int, [C.c_int] * 5
    assert dplan(64, 592, 28, 0x108, 128) < 0
    for wbits, gs in ((4, 128), (8, 0), (8, 64), (16, 0)):
        bad = mk(256, 64, wbits, gs, _C.WKIND_FP8_E4M3)
        assert lib.mi355_linear_partial(1, 4, C.byref(bad), 1, 4, None) == _C.ERR_ARG and b"FP8" in lib.mi355_last_error()
    assert lib.mi355_linear_partial(1, 4, C.byref(mk(256, 64, 8, 128, 7)), 1, 4, None) == _C.ERR_ARG and b"wkind" in lib.mi355_last_error()
