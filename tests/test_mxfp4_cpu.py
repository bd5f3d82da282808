"""MXFP4 (e2m1 codes, e8m0 scale per 32 rows) weights on the host: the quantiser against a brute-force grid search, the packer
against an independent index computation of the tile image and the meta plane, the exponent-range rule, the TP split and merges,
the loader on synthetic Quark-form checkpoints with its refusals, the strategy dispatch, and the library's argument checks and
predicates for the kind.  No GPU."""
import ctypes as C
import json
import logging
import os

import pytest
import torch
from safetensors.torch import save_file

from rtp_llm_amd import _C, loader, model, quant
from rtp_llm_amd.linear import LinearFactory, Mi355Mxfp4Linear

import mxfp4_util

TOY = model.ModelConfig("toy-qwen3-mxfp4", 2, 256, 4, 2, 64, 512, 384, max_pos=128, qkv_bias=False, qk_norm=True)
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _codes(K, N, seed):
    return torch.randint(0, 16, (K, N), generator=_gen(seed), dtype=torch.uint8)


def _bytes(G, N, seed, lo=114, hi=140):
    return torch.randint(lo, hi + 1, (G, N), generator=_gen(seed), dtype=torch.uint8)


# ------------------------------------------------------------------ the format
def test_enum_struct_and_abi():
    assert _C.WKIND_MXFP4 == 2 and quant.WKIND_MXFP4 == 2
    assert C.sizeof(_C.Weight) == 48 and _C.Weight.wkind.offset == 44 and _C.ABI_VERSION == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mi355_decode.h")).read()
    assert "#define MI355_ABI_VERSION 5" in hdr and "MI355_WKIND_MXFP4 = 2" in hdr and "MXFP4 weights (wkind = MI355_WKIND_MXFP4" in hdr
    assert "MI355_WFMT_MXFP4" in open(os.path.join(root, "rtp_llm_amd", "csrc", "internal.h")).read()
    assert quant.E2M1_VALUES.tolist() == GRID + [-v for v in GRID]


def test_operand_is_exact_and_normal_inside_the_exponent_range():
    """The numerics contract: fp16(2^E * e2m1) and its bf16 twin are exact normal numbers for E in [-13, 13], and E = 14 / -14 are
    the first exponents at which fp16 is not (overflow of 6 * 2^14 / a subnormal 0.5 * 2^-14)."""
    v = torch.tensor(GRID[1:], dtype=torch.float64)
    for E in range(-13, 14):
        p = v * 2.0 ** E
        assert torch.equal(p.half().double(), p) and torch.equal(p.bfloat16().double(), p)
        assert float(p.min()) >= 2.0 ** -14 and float(p.max()) <= 49152
    assert torch.isinf((v * 2.0 ** 14).half()).any() and float(v[0] * 2.0 ** -14) < 2.0 ** -14


def test_quant_mxfp4_against_brute_force():
    """OCP rule: E = floor(log2(amax)) - 2, nearest grid value with ties to the even code, saturation at 6."""
    w = torch.randn(96, 24, generator=_gen(1), dtype=torch.float64) * 0.3
    w[:32, 0] = 0                                                                    # an all-zero group: E = 0
    w[32:64, 1] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0] * 4) * 0.125   # every tie, amax 5 -> E = 0 - 3
    w[32, 1] = -w[32, 1]
    w[64:96, 2] = torch.tensor([7.9, -7.5, 6.1, 0.1] * 8)                            # amax 7.9: E = 0, 7.9 / 7.5 / 6.1 saturate at 6
    w[0:32, 3] = 2.0 ** -20 * torch.arange(32)                                       # small magnitudes
    codes, sb = quant.quant_mxfp4(w)
    assert codes.dtype == torch.uint8 and sb.dtype == torch.uint8 and codes.shape == (96, 24) and sb.shape == (3, 24)
    assert int(codes.max()) <= 15
    for g in range(3):
        for n in range(24):
            col = w[32 * g: 32 * g + 32, n]
            amax = float(col.abs().max())
            E = 0
            if amax > 0:
                E = 0
                while 2.0 ** (E + 1) <= amax:
                    E += 1
                while 2.0 ** E > amax:
                    E -= 1
                E -= 2
            assert int(sb[g, n]) == E + 127, (g, n, amax)
            for r in range(32):
                a = abs(float(col[r])) / 2.0 ** E
                d = [abs(a - v) for v in GRID]
                best = min(d)
                cands = [i for i in range(8) if d[i] == best]
                idx = [i for i in cands if i % 2 == 0][0] if len(cands) > 1 else cands[0]   # a tie: the even code
                sign = 8 if (float(col[r]) < 0 and idx > 0) else 0
                assert int(codes[32 * g + r, n]) == idx + sign, (g, n, r, float(col[r]), E)
    assert int(sb[0, 0]) == 127 and bool((codes[:32, 0] == 0).all())
    assert codes[32:40, 1].tolist() == [0, 2, 2, 4, 4, 6, 6, 6] and int(sb[1, 1]) == 127 - 3   # -0.25 * 2^-3 rounds to +0
    assert codes[64:68, 2].tolist() == [7, 15, 7, 0] and int(sb[2, 2]) == 127
    assert torch.equal(quant.dequant_mxfp4(codes, sb).double(), mxfp4_util.w_ref(codes, sb))
    with pytest.raises(AssertionError):
        quant.quant_mxfp4(torch.zeros(48, 8))


@pytest.mark.parametrize("K,N", [(160, 40), (256, 48)])
def test_pack_mxfp4_image_and_meta(K, N):
    """Every code and every scale byte at the place the header gives it; padding in both directions (160 x 40: a ragged last chunk
    of one 32-row group, 8 padding columns) holds code 0 / byte 127."""
    codes, sb = _codes(K, N, K), _bytes(K // 32, N, N)
    p, flushed = quant.pack_mxfp4(codes, sb)
    K_pad, N_pad = (K + 127) // 128 * 128, (N + 15) // 16 * 16
    assert (p.wbits, p.group_size, p.wkind, p.K, p.N, p.K_pad, p.N_pad) == (4, 32, 2, K, N, K_pad, N_pad) and flushed == (0, 0)
    img = p.qweight.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    meta = p.meta.view(torch.int32).to(torch.int64).reshape(-1) & 0xFFFFFFFF
    assert img.numel() == K_pad * N_pad // 8 and meta.numel() == (K_pad // 128) * N_pad
    live = (codes & 7) != 0
    group_live = live.reshape(K // 32, 32, N).any(dim=1)
    want_img, want_meta = torch.zeros_like(img), torch.zeros_like(meta)
    for k in range(K_pad):
        for n in range(N_pad):
            inside = k < K and n < N
            d, b = mxfp4_util.image_position(k, n, K_pad)
            want_img[d] |= (int(codes[k, n]) if inside and bool(group_live[k // 32, n]) else 0) << b
            if k % 32 == 0:
                d, b = mxfp4_util.meta_position(k, n, N_pad)
                want_meta[d] |= (int(sb[k // 32, n]) if inside and bool(group_live[k // 32, n]) else 127) << b
    assert torch.equal(img, want_img)
    assert torch.equal(meta, want_meta)
    assert bool(group_live.all())                                  # (random codes: no group is all zero, so nothing was rewritten)


def test_exponent_range_rule():
    K, N = 64, 16
    codes = torch.full((K, N), 3, dtype=torch.uint8)              # 1.5 everywhere
    sb = torch.full((2, N), 127, dtype=torch.uint8)
    sb[0, 0], sb[1, 1], sb[0, 2] = 127 - 13, 127 + 13, 127 - 14   # the two ends stay, E = -14 is flushed
    sb[1, 3] = 5                                                  # far below: flushed
    codes[:32, 4] = 0; sb[0, 4] = 255 - 1                         # an all-zero group with a huge scale: rewritten, not refused
    codes[32:, 5] = 8; sb[1, 5] = 3                               # only -0 codes: zero group, rewritten, not counted as flushed
    codes[32:, 3] = torch.tensor([0, 8, 1, 9] * 8, dtype=torch.uint8)   # 16 nonzero weights in the flushed group
    c2, s2, groups, weights = quant.mxfp4_apply_range(codes, sb)
    assert (groups, weights) == (2, 32 + 16)
    assert int(s2[0, 0]) == 114 and int(s2[1, 1]) == 140 and bool((c2[:32, 0] == 3).all())
    for g, n in ((0, 2), (1, 3), (0, 4), (1, 5)):
        assert int(s2[g, n]) == 127 and bool((c2[32 * g: 32 * g + 32, n] == 0).all()), (g, n)
    # what was flushed is below 6 * 2^-14
    lost = mxfp4_util.w_ref(codes, sb).abs()[(c2 == 0) & ((codes & 7) != 0)]
    assert lost.numel() == 48 and float(lost.max()) < 6 * 2.0 ** -14
    # after the rule W = e2m1 * 2^(byte - 127) holds with every exponent inside [-13, 13]
    assert int(s2.min()) >= 114 and int(s2.max()) <= 140
    p, fl = quant.pack_mxfp4(codes, sb)
    assert fl == (2, 48)
    assert quant.mxfp4_apply_range(c2, s2)[2:] == (0, 0)          # idempotent
    for bad_byte, msg in ((127 + 14, r"\[-13, 13\]"), (255, r"\[-13, 13\]")):
        sb2 = sb.clone(); sb2[0, 7] = bad_byte
        with pytest.raises(ValueError, match=msg):
            quant.pack_mxfp4(codes, sb2)
    sb2 = sb.clone(); sb2[0, 4] = 255                             # NaN byte even on an all-zero group
    with pytest.raises(ValueError, match="255"):
        quant.pack_mxfp4(codes, sb2)
    with pytest.raises(ValueError, match="0..15"):
        quant.pack_mxfp4(torch.full((32, 16), 16, dtype=torch.uint8), sb[:1])
    with pytest.raises(AssertionError):
        quant.pack_mxfp4(codes, sb[:1])


# ------------------------------------------------------------------ canonical linears
def test_canon_linear_mxfp4_ops():
    c = model.synth_linear(256, 384, "mxfp4", "cpu", _gen(6))
    assert c.kind == "mxfp4" and c.group_size == 32 and c.q.dtype == torch.uint8 and c.scales.dtype == torch.uint8
    assert c.scales.shape == (8, 384) and c.z_eff is None and int(c.q.max()) <= 15
    assert int(c.scales.min()) >= 114 and int(c.scales.max()) <= 140    # xavier weights sit well inside the range
    W = mxfp4_util.w_ref(c.q, c.scales)
    assert torch.equal(mxfp4_util.w_ref(c.cols(64, 200).q, c.cols(64, 200).scales), W[:, 64:200])
    r = c.rows(96, 256)                                               # rows in multiples of 32
    assert r.K == 160 and torch.equal(mxfp4_util.w_ref(r.q, r.scales), W[96:])
    with pytest.raises(AssertionError):
        c.rows(16, 256)
    pc, pr = c.pad_cols(16), c.pad_rows(64)
    assert pc.N == 400 and bool((mxfp4_util.w_ref(pc.q, pc.scales)[:, 384:] == 0).all())
    assert pr.K == 320 and bool((mxfp4_util.w_ref(pr.q, pr.scales)[256:] == 0).all())
    assert pc.pack().wkind == 2 and pr.pack().K_pad == 384            # the zero groups (byte 0) are rewritten to 127, not refused
    cat = model.CanonLinear.cat_cols([c.cols(0, 128), c.cols(128, 256), c.cols(256, 384)])   # q / k / v merge
    assert torch.equal(cat.q, c.q) and torch.equal(cat.scales, c.scales) and cat.kind == "mxfp4"
    p = c.pack()
    assert (p.wkind, p.wbits, p.group_size) == (2, 4, 32)
    gu = c.pack(gate_up=True)                                         # interleaved (gate, up) columns: codes and bytes move together
    ref, _ = quant.pack_mxfp4(quant.interleave_gate_up(c.q), quant.interleave_gate_up(c.scales))
    assert torch.equal(gu.qweight, ref.qweight) and torch.equal(gu.meta, ref.meta)
    w8, s8 = c.factory_weight(), c.factory_scales()
    qw, qs = mxfp4_util.to_quark(c)
    assert torch.equal(w8, qw) and torch.equal(s8, qs) and w8.shape == (384, 128) and s8.shape == (384, 8)


def test_split_layer_tp_equals_slices_of_w_ref():
    cfg = TOY
    w = model.synth_model(cfg, "mxfp4", "cpu", seed=8)
    R = w["layers"][1]
    W = {k: mxfp4_util.w_ref(R[k].q, R[k].scales) for k in ("qkv", "o", "gate_up", "down")}
    S = []
    for rank in range(2):
        L = model.split_layer_tp(R, cfg, 2, rank)
        S.append({k: mxfp4_util.w_ref(L[k].q, L[k].scales) for k in W})
        assert L["o"].kind == "mxfp4" and L["o"].K == cfg.nh * cfg.hd // 2 and L["down"].group_size == 32
    hd, nh, nkv, I = cfg.hd, cfg.nh, cfg.nkv, cfg.inter
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


# ------------------------------------------------------------------ the loader
def _toy(seed=7):
    return model.synth_model(TOY, "mxfp4", "cpu", seed=seed)


def test_loader_round_trip_with_an_excluded_module(tmp_path):
    w = _toy()
    mxfp4_util.write_mxfp4_ckpt(str(tmp_path), TOY, w, excluded=("self_attn.o_proj",))
    cfg, lw = loader.load_hf_checkpoint(str(tmp_path))
    assert cfg.qk_norm and cfg.num_layers == 2 and not cfg.qkv_bias
    assert lw["lm_head"].kind == "fp16"
    for L, R in zip(lw["layers"], w["layers"]):
        for k in ("qkv", "gate_up", "down"):
            assert L[k].kind == "mxfp4" and L[k].group_size == 32 and (L[k].K, L[k].N) == (R[k].K, R[k].N)
            assert L[k].q.dtype == torch.uint8 and torch.equal(L[k].q, R[k].q), k
            assert L[k].scales.dtype == torch.uint8 and torch.equal(L[k].scales, R[k].scales), k
        assert L["o"].kind == "fp16" and torch.equal(L["o"].w, mxfp4_util.w_ref(R["o"].q, R["o"].scales).half())
        assert torch.equal(L["q_norm"], R["q_norm"])
    L, R = lw["layers"][0], w["layers"][0]
    nq, nk = TOY.nh * TOY.hd, TOY.nkv * TOY.hd
    for lo, hi in ((0, nq), (nq, nq + nk), (nq + nk, nq + 2 * nk)):
        assert torch.equal(mxfp4_util.w_ref(L["qkv"].cols(lo, hi).q, L["qkv"].cols(lo, hi).scales), mxfp4_util.w_ref(R["qkv"].q, R["qkv"].scales)[:, lo:hi])
    cfg1, lw1 = loader.load_hf_checkpoint(str(tmp_path), max_layers=1, dtype=torch.bfloat16)
    assert cfg1.num_layers == 1 and lw1["layers"][0]["input_norm"].dtype == torch.bfloat16 and lw1["layers"][0]["o"].w.dtype == torch.bfloat16
    assert torch.equal(lw1["layers"][0]["down"].q, w["layers"][0]["down"].q)
    # tp = 2 shards reassemble
    shards = [loader.load_hf_checkpoint(str(tmp_path), tp=2, rank=r)[1] for r in range(2)]
    down = torch.cat([mxfp4_util.w_ref(s["layers"][1]["down"].q, s["layers"][1]["down"].scales) for s in shards], dim=0)
    assert torch.equal(down, mxfp4_util.w_ref(w["layers"][1]["down"].q, w["layers"][1]["down"].scales))


def test_loader_flushes_and_warns_once(tmp_path, caplog):
    w = _toy(9)
    for i in (0, 1):
        w["layers"][i]["down"].scales[0, :3] = 100                 # E = -27: three groups per layer
    t = mxfp4_util.write_mxfp4_ckpt(str(tmp_path), TOY, w)
    with caplog.at_level(logging.WARNING, logger="rtp_llm_amd.loader"):
        _, lw = loader.load_hf_checkpoint(str(tmp_path))
    msgs = [r.getMessage() for r in caplog.records if "MXFP4" in r.getMessage()]
    nz = sum(int(((w["layers"][i]["down"].q[:32, :3] & 7) != 0).sum()) for i in (0, 1))
    assert len(msgs) == 1 and msgs[0].startswith(f"MXFP4: 6 groups ({nz} nonzero weights")
    d = lw["layers"][0]["down"]
    assert bool((d.q[:32, :3] == 0).all()) and bool((d.scales[0, :3] == 127).all()) and torch.equal(d.q[32:], w["layers"][0]["down"].q[32:])
    assert t["model.layers.0.mlp.down_proj.weight_scale"][0, 0] == 100


def _set_config(tmp, qc):
    p = os.path.join(tmp, "config.json")
    cfg = json.load(open(p))
    cfg["quantization_config"] = qc
    json.dump(cfg, open(p, "w"))


def test_loader_refusals(tmp_path):
    tmp = str(tmp_path)
    w = _toy(10)
    t = mxfp4_util.write_mxfp4_ckpt(tmp, TOY, w)
    loader.load_hf_checkpoint(tmp, max_layers=1)                   # the form itself is accepted
    for field, value in (("dtype", "fp6"), ("dtype", "fp8"), ("dtype", "int4"), ("group_size", 16), ("group_size", 128),
                         ("qscheme", "per_channel"), ("scale_format", "float32"), ("scale_format", None), ("is_dynamic", True), ("ch_axis", 0)):
        _set_config(tmp, mxfp4_util.quark_cfg(**{field: value}))
        with pytest.raises(NotImplementedError, match=field):
            loader.load_hf_checkpoint(tmp)
    qc = mxfp4_util.quark_cfg(); qc["global_quant_config"]["input_tensors"]["is_dynamic"] = False
    _set_config(tmp, qc)
    with pytest.raises(NotImplementedError, match="input_tensors"):
        loader.load_hf_checkpoint(tmp)
    qc = mxfp4_util.quark_cfg(); qc["global_quant_config"]["input_tensors"] = None     # weight-only export: accepted
    _set_config(tmp, qc)
    loader.load_hf_checkpoint(tmp, max_layers=1)
    qc = mxfp4_util.quark_cfg(); qc["layer_quant_config"] = {"*down_proj": {"weight": {"dtype": "fp8_e4m3"}}}
    _set_config(tmp, qc)
    with pytest.raises(NotImplementedError, match="layer_quant_config"):
        loader.load_hf_checkpoint(tmp)
    qc = mxfp4_util.quark_cfg(); qc["desc_act"] = True
    _set_config(tmp, qc)
    with pytest.raises(NotImplementedError, match="desc"):
        loader.load_hf_checkpoint(tmp)
    qc = mxfp4_util.quark_cfg(); del qc["global_quant_config"]
    _set_config(tmp, qc)
    with pytest.raises(NotImplementedError, match="global_quant_config"):
        loader.load_hf_checkpoint(tmp)
    _set_config(tmp, mxfp4_util.quark_cfg())
    with pytest.raises(NotImplementedError, match="int8"):
        loader.load_hf_checkpoint(tmp, quantization="int8")
    _set_config(tmp, {"quant_method": "nvfp4"})                    # the general message lists the new form
    with pytest.raises(NotImplementedError, match="Quark MXFP4"):
        loader.load_hf_checkpoint(tmp)
    _set_config(tmp, mxfp4_util.quark_cfg())
    # tensors: a missing scale, float scales, a wrong shape, an exponent outside the range, a NaN byte, an unlisted 16-bit module
    name = "model.layers.0.mlp.down_proj"
    base = {k: v.contiguous() for k, v in t.items()}
    sc = base[name + ".weight_scale"]

    def rewrite(**changes):
        d = {**base, **{k: v for k, v in changes.items() if v is not None}}
        for k, v in changes.items():
            if v is None:
                d.pop(k)
        save_file(d, os.path.join(tmp, "model.safetensors"))

    rewrite(**{name + ".weight_scale": None})
    with pytest.raises(NotImplementedError, match=r"down_proj\.weight_scale"):
        loader.load_hf_checkpoint(tmp)
    rewrite(**{name + ".weight_scale": torch.ones_like(sc, dtype=torch.float16)})
    with pytest.raises(NotImplementedError, match=r"down_proj\.weight_scale.*float16"):
        loader.load_hf_checkpoint(tmp)
    rewrite(**{name + ".weight_scale": sc[:, :-1].contiguous()})
    with pytest.raises(ValueError, match=r"down_proj\.weight_scale: shape"):
        loader.load_hf_checkpoint(tmp)
    bad = sc.clone(); bad[1, 2] = 127 + 14
    rewrite(**{name + ".weight_scale": bad})
    with pytest.raises(ValueError, match=r"down_proj\.weight_scale.*\[-13, 13\]"):
        loader.load_hf_checkpoint(tmp)
    bad = sc.clone(); bad[1, 2] = 255
    rewrite(**{name + ".weight_scale": bad})
    with pytest.raises(ValueError, match=r"down_proj\.weight_scale.*255"):
        loader.load_hf_checkpoint(tmp)
    rewrite(**{name + ".weight": torch.zeros(TOY.hidden, TOY.inter, dtype=torch.float16)})
    with pytest.raises(NotImplementedError, match=r"down_proj\.weight.*exclude"):
        loader.load_hf_checkpoint(tmp)


# ------------------------------------------------------------------ strategies
def test_mxfp4_strategy_is_the_only_match():
    c = model.synth_linear(256, 128, "mxfp4", "cpu", _gen(11))
    w8, s8 = mxfp4_util.to_quark(c)
    hits = [s.__name__ for s in LinearFactory._strategies if s.can_handle(None, w8, s8)]
    assert hits == ["Mi355Mxfp4Linear"], hits
    assert not Mi355Mxfp4Linear.can_handle(None, w8, None) and not Mi355Mxfp4Linear.can_handle(None, w8, s8.half())
    assert not Mi355Mxfp4Linear.can_handle(None, w8, s8[:, :-1]) and not Mi355Mxfp4Linear.can_handle(None, w8.view(torch.int8), s8)
    # canonical W4 tensors (uint8 codes, fp16 scales) still go to the W4 strategy alone
    w4 = model.synth_linear(256, 128, "w4", "cpu", _gen(12))
    assert [s.__name__ for s in LinearFactory._strategies if s.can_handle(None, w4.q, w4.scales)] == ["Mi355W4A16Linear"]
    a = LinearFactory.create_linear(w8, None, s8)
    ref = c.pack()
    assert isinstance(a, Mi355Mxfp4Linear) and torch.equal(a.packed.qweight, ref.qweight) and torch.equal(a.packed.meta, ref.meta)
    assert a.packed.wkind == 2 and (a.in_features, a.out_features) == (256, 128) and a.flushed == (0, 0)
    from rtp_llm_amd.linear import STRATEGY_IMPLS, QuantConfig
    assert "Mi355Mxfp4Linear" in [n for n, _ in STRATEGY_IMPLS] and QuantConfig(method="mxfp4").is_quanted()


# ------------------------------------------------------------------ the library, host side
def test_library_refuses_the_kind_on_every_fused_and_image_entry():
    """No image / fused launch or predicate takes wkind = 2 (an e2m1 image must never be decoded as integer W4 g32), and the kind
    only goes with wbits 4 / group_size 32.  Host code of the library: every call returns before it touches a device pointer."""
    lib = C.CDLL(_C.lib()._name)                                   # an own handle: argtypes set here stay here
    W = C.POINTER(_C.Weight)
    vp, i32 = C.c_void_p, C.c_int32
    mk = lambda K, N, wbits, gs, kind: _C.Weight(1 << 20, 1 << 21, wbits, K, N, K, N, gs, _C.ACT_F16, kind)   # pointers are never read here
    MX = _C.WKIND_MXFP4
    lib.mi355_last_error.restype = C.c_char_p
    for name, extra, int_gs in (("mi355_fullk_weight_ok", (), 32), ("mi355_fullk64_weight_ok", (), 32), ("mi355_gemm_wide_direct_ok", (), None),
                                ("mi355_fullk64_publish_ok", (), 128), ("mi355_fullk64_qkv_ok", (128,), 32)):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, [W] + [C.c_int] * len(extra)
        for wbits, gs in ((4, 32), (4, 128), (8, 0)):              # whatever else the struct says, the kind decides
            assert f(C.byref(mk(4096, 4096, wbits, gs, MX)), *extra) == 0, (name, wbits, gs)
        if int_gs is not None:                                     # the same struct with integer codes is served: the kind alone refused it
            assert f(C.byref(mk(4096, 4096, 4, int_gs, _C.WKIND_INT)), *extra) == 1, name
    plan = lib.mi355_gemm_splitk64_plan
    plan.restype, plan.argtypes = C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int)]
    assert plan(64, 224, 148, 0x204, 32, 16, None) < 0 and plan(64, 224, 148, 4, 32, 16, None) > 0   # the library's format code of the kind
    dplan = lib.mi355_gemm_splitk64_direct_plan
    dplan.restype, dplan.argtypes = C.c_int, [C.c_int] * 5
    assert dplan(64, 592, 28, 0x204, 32) < 0
    w = mk(4096, 4096, 4, 32, MX)
    P = 1 << 22                                                   # a non-null dummy for every pointer argument
    entries = {
        "mi355_linear_residual": ([vp, i32, W, vp, vp, vp, vp, i32, vp], (P, 8, C.byref(w), None, P, P, None, 0, None)),
        "mi355_linear_residual_img": ([vp, i32, W, vp, vp, vp, vp, i32, vp], (P, 8, C.byref(w), None, P, P, None, 0, None)),
        "mi355_linear_publish_img": ([vp, i32, W, vp, vp, vp], (P, 8, C.byref(w), None, P, None)),
        "mi355_linear_residual_prenorm_img": ([vp, i32, W, vp, vp, vp, vp, i32, vp, vp, i32, vp], (P, 8, C.byref(w), None, P, P, P, 0, P, P, 256, None)),
        "mi355_linear_deferred_norm_img": ([vp, i32, vp, W, vp, vp, i32, vp], (P, 8, None, C.byref(w), None, P, 0, None)),
        "mi355_linear_direct_img": ([vp, i32, W, vp, vp, i32, vp], (P, 8, C.byref(w), None, P, 0, None)),
        "mi355_linear_partial_img": ([vp, i32, W, vp, i32, vp], (P, 8, C.byref(w), P, 4, None)),
        "mi355_qkv_touch_plan": ([W, i32, vp, vp], (C.byref(w), 128, P, P)),
    }
    for name, (argtypes, args) in entries.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, argtypes
        assert f(*args) == _C.ERR_UNSUPPORTED, (name, lib.mi355_last_error())
    part = lib.mi355_linear_partial
    part.restype, part.argtypes = C.c_int, [vp, i32, W, vp, i32, vp]
    for wbits, gs in ((4, 128), (4, 64), (4, 0), (8, 32), (8, 128), (16, 32)):
        bad = mk(256, 64, wbits, gs, MX)
        assert part(1, 4, C.byref(bad), 1, 4, None) == _C.ERR_ARG and b"wkind" in lib.mi355_last_error(), (wbits, gs)
    assert part(1, 4, C.byref(mk(256, 64, 4, 32, 3)), 1, 4, None) == _C.ERR_ARG and b"wkind" in lib.mi355_last_error()
