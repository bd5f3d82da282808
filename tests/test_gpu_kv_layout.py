"""The reference's KV block layouts on the GPU, through the C ABI (include/mi355_decode.h: MI355_KV_LAYOUT_REF / _REF_VVEC).

  * reader against the reference's OWN attention result on the reference's layout (golden vectors, oracle/gen_golden.py);
  * layout invariance of reader and writers, BIT-EXACT: a layout only changes addresses -- every MFMA sees the same operands in the
    same order -- so the result on convert_layout(native cache) equals the result on the native cache without any tolerance, and a
    writer leaves convert_layout(what the native writer leaves) in the WHOLE cache tensor (no stray bytes);
  * the step driver (prefill, eager steps, captured graph) per layout;
  * the hand-over the layouts exist for, in both directions: somebody else's prefill -> our decode, our prefill -> somebody else's reader;
  * the reference-shaped module graph, prefill to decode through the plug-in lists only, against the oracle.
"""
import glob
import math
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from rtp_llm_amd import _C, attention, kvcache, model, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-2, rtol=1e-2)          # the project's attention tolerance (tests/test_gpu_parity.py, the reference's own)
NATIVE, REF, VVEC = _C.KV_LAYOUT_NATIVE, _C.KV_LAYOUT_REF, _C.KV_LAYOUT_REF_VVEC
REF_LAYOUTS = [REF, VVEC]
ids = {REF: "ref", VVEC: "ref_vvec"}
layouts = pytest.mark.parametrize("layout", REF_LAYOUTS, ids=[ids[l] for l in REF_LAYOUTS])


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _C.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dense(c):
    if c.kind == "fp16":
        return c.w.float()
    if c.kind == "int8":
        return oracle.dequant_int8(c.q, c.scales)
    return oracle.dequant_groupwise(c.q, c.z_eff, c.scales, c.group_size)


def _oracle_weights(w):
    return {"embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": _dense(w["lm_head"]),
            "layers": [{"input_norm": L["input_norm"], "post_norm": L["post_norm"], "qkv_bias": L["qkv_bias"],
                        **{k: _dense(L[k]) for k in ("qkv", "o", "gate_up", "down")}} for L in w["layers"]]}


def _to(cache, layout):
    return kvcache.convert_layout(cache, NATIVE, layout)


# ------------------------------------------------------------------ 6. reader against the reference's own result
def _golden(golden_dir, stem):
    parts = sorted(glob.glob(os.path.join(golden_dir, stem + ".*.npz")))
    assert parts
    return {k: v for p in parts for k, v in np.load(p).items()}


def _ref_cache(Kn, Vn, nblk, block, nkv, hd, layout):
    """the caches gen_golden.py hands to the reference's run_native, as one [blocks, 2, nkv, page, hd] pool tensor"""
    x = 8
    k = Kn.view(nblk, block, nkv, hd // x, x).permute(0, 2, 3, 1, 4).reshape(nblk, -1)
    if layout == REF:
        v = Vn.view(nblk, block, nkv, hd).permute(0, 2, 3, 1).reshape(nblk, -1)
    else:
        v = Vn.view(nblk, block // x, x, nkv, hd).permute(0, 3, 1, 4, 2).reshape(nblk, -1)
    return torch.stack([k, v], dim=1).reshape(nblk, 2, nkv, block, hd).contiguous()


@layouts
@pytest.mark.parametrize("stem,case", [("ref_layers", 0), ("ref_layers", 1), ("ref_layers", 2), ("ref_layers_bf16", 0), ("ref_layers_bf16", 1)])
def test_reader_matches_the_references_result_on_the_references_layout(golden_dir, stem, case, layout):
    r = _golden(golden_dir, stem)
    bf = stem.endswith("bf16")
    t = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).view(torch.bfloat16)) if bf else (lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    nh, nkv, hd, block = (int(v) for v in r[f"attn{case}_cfg"][:4])
    assert bf or int(r[f"attn{case}_cfg"][4]) == 0
    ctx, bt = r[f"attn{case}_ctx"].tolist(), torch.from_numpy(np.ascontiguousarray(r[f"attn{case}_bt"])).to(torch.int32)
    q, Kn, Vn, want = t(r[f"attn{case}_q"]), t(r[f"attn{case}_k"]), t(r[f"attn{case}_v"]), t(r[f"attn{case}_out"])
    nblk = Kn.shape[0] // block
    cache = _ref_cache(Kn, Vn, nblk, block, nkv, hd, layout).to(DEV)
    out = ops.paged_decode_attention(q.to(DEV), cache, None, bt.to(DEV), torch.tensor(ctx, dtype=torch.int32, device=DEV), nkv, block, max(ctx),
                                     layout=layout)
    torch.cuda.synchronize()
    got, want = out.cpu().float().reshape(len(ctx), -1), want.float().reshape(len(ctx), -1)
    err = float((got - want).abs().max())
    print(f"golden {stem} attn{case} layout {ids[layout]}: max |err| {err:.3e}")
    assert torch.allclose(got, want, **TOL), err
    # the codec reads the reference's cache back as the natural K / V it was built from
    K0, V0, _, _ = kvcache.read_tokens(cache, None, bt[0].to(DEV), ctx[0], layout=layout)
    slots = (bt[0].long()[torch.arange(ctx[0]) // block] * block + torch.arange(ctx[0]) % block)
    assert torch.equal(K0.cpu(), Kn[slots]) and torch.equal(V0.cpu(), Vn[slots])


# ------------------------------------------------------------------ 7. layout invariance of the reader, bit-exact
def _fill_cache(B, ctx_lens, nkv, hd, page, nblk, seed, dtype=torch.float16):
    g = _gen(seed)
    max_blocks = (max(ctx_lens) + page - 1) // page
    bt = torch.randperm(nblk, generator=g)[: B * max_blocks].reshape(B, max_blocks).to(torch.int32)
    kv, _ = kvcache.alloc_layer_cache(nblk, nkv, page, hd, False, DEV, dtype)
    kv.copy_(torch.randn(kv.shape, generator=g).to(dtype))      # pages nobody wrote hold junk, as in a recycled pool
    for b in range(B):
        K, V = torch.randn(ctx_lens[b], nkv, hd, generator=g).to(dtype), torch.randn(ctx_lens[b], nkv, hd, generator=g).to(dtype)
        kvcache.write_tokens(kv, None, bt[b], 0, K, V)
    return kv, bt


@pytest.mark.parametrize("nh,nkv,hd,page,dtype", [(28, 4, 128, 16, torch.float16), (32, 8, 128, 16, torch.float16), (14, 2, 64, 64, torch.float16),
                                                  (8, 1, 128, 64, torch.float16), (16, 16, 128, 16, torch.float16), (28, 4, 128, 32, torch.bfloat16)])
def test_decode_attention_is_bit_equal_across_layouts(nh, nkv, hd, page, dtype):
    ctx = [1, 7, 8, 15, 16, 17, 31, 33, 127, 128, 129, 500, 1024, 1500]       # the context list of test_paged_attention
    B = len(ctx)
    nblk = sum((c + page - 1) // page for c in ctx) + B * ((max(ctx) + page - 1) // page)
    kv, bt = _fill_cache(B, ctx, nkv, hd, page, nblk, 21, dtype)
    q = torch.randn(B, nh, hd, generator=_gen(4)).to(dtype).to(DEV)
    sl = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    want = ops.paged_decode_attention(q, kv, None, bt.to(DEV), sl, nkv, page, max(ctx))
    assert bool(torch.isfinite(want.float()).all())
    for layout in REF_LAYOUTS:
        got = ops.paged_decode_attention(q, _to(kv, layout), None, bt.to(DEV), sl, nkv, page, max(ctx), layout=layout)
        assert torch.equal(got, want), (ids[layout], float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("nh,nkv,hd,page,q_len,dtype", [(28, 4, 128, 16, 5, torch.float16), (32, 8, 128, 16, 9, torch.float16), (14, 2, 64, 64, 3, torch.float16),
                                                        (8, 1, 128, 16, 2, torch.float16), (16, 16, 128, 16, 33, torch.float16),
                                                        (28, 4, 128, 16, 5, torch.bfloat16)])
def test_rows_attention_and_image_output_are_bit_equal_across_layouts(nh, nkv, hd, page, q_len, dtype):
    base = [0, 7, 130, 1000]                                   # the sequences of test_paged_attention_rows_causal
    B = len(base)
    ctx = [b + q_len for b in base]
    nblk = sum((c + page - 1) // page for c in ctx) + B * ((max(ctx) + page - 1) // page)
    kv, bt = _fill_cache(B, ctx, nkv, hd, page, nblk, 33, dtype)
    q = torch.randn(B * q_len, nh, hd, generator=_gen(5)).to(dtype).to(DEV)
    pos = torch.tensor([[b + i for i in range(q_len)] for b in base], dtype=torch.int32)
    pos[1, q_len - 1] = -1                                     # padding row
    pos = pos.reshape(-1).contiguous().to(DEV)
    want = ops.paged_attention_rows(q, kv, None, bt.to(DEV), pos, nkv, page, q_len, max(ctx))
    img = B * q_len <= 64
    want_img = ops.paged_attention_rows_img(q, kv, None, bt.to(DEV), pos, nkv, page, q_len, max(ctx)) if img else None
    for layout in REF_LAYOUTS:
        c = _to(kv, layout)
        got = ops.paged_attention_rows(q, c, None, bt.to(DEV), pos, nkv, page, q_len, max(ctx), layout=layout)
        assert torch.equal(got, want), (ids[layout], float((got.float() - want.float()).abs().max()))
        if img:
            got_img = ops.paged_attention_rows_img(q, c, None, bt.to(DEV), pos, nkv, page, q_len, max(ctx), layout=layout)
            assert torch.equal(got_img.unpack(), want_img.unpack()), ids[layout]


# ------------------------------------------------------------------ 8. writers, bit-exact, whole cache
def _same_as_native(run, nblk, nkv, page, hd, dtype):
    """run(kv, oob, layout) -> q; every layout must leave convert_layout(native cache), the same q and the same oob count"""
    res = {}
    for layout in [NATIVE] + REF_LAYOUTS:
        kv, _ = kvcache.alloc_layer_cache(nblk, nkv, page, hd, False, DEV, dtype)
        oob = torch.zeros(1, dtype=torch.int32, device=DEV)
        q = run(kv, oob, layout)
        assert q is not None
        torch.cuda.synchronize()
        res[layout] = (q, kv, int(oob.item()))
    q0, kv0, oob0 = res[NATIVE]
    assert bool((kv0 != 0).any())
    for layout in REF_LAYOUTS:
        q, kv, oob = res[layout]
        assert torch.equal(q, q0), ids[layout]
        assert oob == oob0, (ids[layout], oob, oob0)
        assert torch.equal(kv, _to(kv0, layout)), ids[layout]         # the WHOLE tensor: nothing written anywhere else
        assert not torch.equal(kv, kv0)
    return oob0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("nh,nkv,hd,page", [(28, 4, 128, 16), (14, 2, 64, 64), (8, 1, 128, 16)])
def test_standalone_writers_leave_the_converted_native_cache(nh, nkv, hd, page, dtype):
    T, max_blocks, nblk = 6, 8, 64                              # the shapes of test_rope_kv_write
    cfg = model.ModelConfig("t", 1, nh * hd, nh, nkv, hd, 64, 128, max_pos=max_blocks * page)
    cs = model.rope_table(cfg, DEV)
    W = (nh + 2 * nkv) * hd
    qkv = (torch.randn(T, W, generator=_gen(11)) * 0.5).to(dtype).to(DEV)
    bias = (torch.randn(W, generator=_gen(12)) * 0.1).to(dtype).to(DEV)
    pos = torch.tensor([0, 1, 15, 16, 37, max_blocks * page - 1], dtype=torch.int32, device=DEV)
    bt = torch.randperm(nblk, generator=_gen(2))[: T * max_blocks].reshape(T, max_blocks).to(torch.int32).to(DEV)
    args = (nblk, nkv, page, hd, dtype)
    assert _same_as_native(lambda kv, oob, lay: ops.rope_kv_write(qkv, bias, cs, pos, bt, kv, None, nh, nkv, hd, page, oob, layout=lay), *args) == 0
    # rows mode: 2 sequences x 3 rows, a padding row and a position past the table
    rpos = torch.tensor([14, 15, 16, 30, max_blocks * page + 3, -1], dtype=torch.int32, device=DEV)
    rbt = bt[:2].contiguous()
    assert _same_as_native(lambda kv, oob, lay: ops.rope_kv_write_rows(qkv, None, cs, rpos, rbt, kv, None, nh, nkv, hd, page, 3, oob, layout=lay), *args) == 1
    qn = (1 + 0.1 * torch.randn(hd, generator=_gen(13))).to(dtype).to(DEV)
    kn = (1 + 0.1 * torch.randn(hd, generator=_gen(14))).to(dtype).to(DEV)
    assert _same_as_native(lambda kv, oob, lay: ops.rope_kv_write_rows_qk_norm(qkv, bias, qn, kn, 1e-6, cs, rpos, rbt, kv, None, nh, nkv, hd, page, 3,
                                                                             oob, layout=lay), *args) == 1


@pytest.fixture(scope="module")
def qwen2_7b_qkv():
    nh, nkv, hd, K = 28, 4, 128, 3584
    N = (nh + 2 * nkv) * hd
    packed = model.synth_linear(K, N, "w4", DEV, torch.Generator(device=DEV).manual_seed(K + N), zeros="centered").pack()
    return nh, nkv, hd, K, N, packed


@pytest.mark.parametrize("M", [1, 4, 16])
def test_fused_qkv_writer_leaves_the_converted_native_cache(qwen2_7b_qkv, M):
    nh, nkv, hd, K, N, packed = qwen2_7b_qkv
    page, max_blocks = 16, 4
    nblk = M * max_blocks
    cfg = model.ModelConfig("t", 1, K, nh, nkv, hd, 64, 128, max_pos=max_blocks * page)
    cs = model.rope_table(cfg, DEV)
    g = _gen(M)
    x = (torch.randn(M, K, generator=g) * 0.5).half().to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).half().to(DEV)
    pos = torch.randint(0, max_blocks * page, (M,), generator=g).to(torch.int32)
    if M > 1:
        pos[M - 1] = max_blocks * page + 1                      # one stale row
    pos = pos.to(DEV)
    bt = torch.randperm(nblk, generator=g).reshape(M, max_blocks).to(torch.int32).to(DEV)
    run = lambda kv, oob, lay: ops.qkv_rope_kv_write(x, packed, bias, cs, pos, bt, kv, None, nh, nkv, hd, page, 1, oob, layout=lay)
    assert _same_as_native(run, nblk, nkv, page, hd, torch.float16) == (1 if M > 1 else 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M", [5, 33, 64])
def test_fused_qkv_image_writer_leaves_the_converted_native_cache(qwen2_7b_qkv, M, dtype):
    nh, nkv, hd, K, N, packed = qwen2_7b_qkv
    page, max_blocks = 16, 4
    nblk = M * max_blocks
    cfg = model.ModelConfig("t", 1, K, nh, nkv, hd, 64, 128, max_pos=max_blocks * page)
    cs = model.rope_table(cfg, DEV)
    g = _gen(100 + M)
    x = ops.act_image_pack((torch.randn(M, K, generator=g) * 0.5).to(dtype).to(DEV))
    bias = (torch.randn(N, generator=g) * 0.1).to(dtype).to(DEV)
    pos = torch.randint(0, max_blocks * page, (M,), generator=g).to(torch.int32)
    pos[2], pos[M - 1] = -1, max_blocks * page + 1              # a padding row and a stale one
    pos = pos.to(DEV)
    bt = torch.randperm(nblk, generator=g).reshape(M, max_blocks).to(torch.int32).to(DEV)
    run = lambda kv, oob, lay: ops.qkv_rope_kv_write_img(x, packed, bias, cs, pos, bt, kv, None, nh, nkv, hd, page, 1, oob, layout=lay)
    assert _same_as_native(run, nblk, nkv, page, hd, dtype) == 1


def test_int8_caches_refuse_the_reference_layouts_before_any_launch():
    nh, nkv, hd, page, nblk = 8, 2, 64, 16, 8
    kv8, sc8 = kvcache.alloc_layer_cache(nblk, nkv, page, hd, True, DEV)
    before = kv8.clone()
    cfg = model.ModelConfig("t", 1, nh * hd, nh, nkv, hd, 64, 128, max_pos=64)
    cs = model.rope_table(cfg, DEV)
    qkv = torch.zeros(2, (nh + 2 * nkv) * hd, dtype=torch.float16, device=DEV)
    pos, bt = torch.tensor([0, 1], dtype=torch.int32, device=DEV), torch.arange(8, dtype=torch.int32, device=DEV).reshape(2, 4)
    for layout in REF_LAYOUTS + [7]:
        with pytest.raises(_C.Mi355Error):
            ops.rope_kv_write(qkv, None, cs, pos, bt, kv8, sc8, nh, nkv, hd, page, layout=layout)
        with pytest.raises(_C.Mi355Error):
            ops.paged_decode_attention(qkv[:, : nh * hd].reshape(2, nh, hd).contiguous(), kv8, sc8, bt, pos + 1, nkv, page, 64, layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(kv8, before)


# ------------------------------------------------------------------ 9. the step driver
def _tiny_prefill_case():
    """config, weights, prompts and block table of test_prefill_ragged_prompts_multi_chunk_matches_oracle"""
    cfg = model.ModelConfig("tiny-prefill", 2, 512, 8, 2, 64, 1024, 2048, max_pos=512)
    w = model.synth_model(cfg, "w4", "cpu", seed=29, zeros="centered")
    lens, page = [150, 97, 201], 16
    B = len(lens)
    g = _gen(31)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=g, dtype=torch.int32).tolist() for n in lens]
    bt = torch.randperm(B * 16, generator=g).reshape(B, 16).to(torch.int32)
    return cfg, w, lens, page, B, prompts, bt


def _engine_run(cfg, w_dev, lens, page, B, prompts, bt, layout, graph):
    eng = model.DecoderEngine(cfg, w_dev, kv_int8=False, page=page, num_blocks=B * 16, max_batch=4, max_seq_len=256, device=DEV, kv_layout=layout)
    assert eng.kv_layout == layout
    trace = [eng.prefill(prompts, bt, chunk=64).clone()]
    eng.set_inputs(ops.argmax(trace[0]).tolist(), lens, bt)
    if graph:
        eng.capture(B)
    for _ in range(3):
        if graph:
            eng.replay(B, 1)
        else:
            eng.step(B)
        torch.cuda.synchronize()
        trace.append(eng.logits[:B].clone()); trace.append(eng.token_ids[:B].clone())
    assert eng.oob_count() == 0
    return eng, trace


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_engine_per_layout_is_bit_equal_to_the_native_engine(graph):
    cfg, w, lens, page, B, prompts, bt = _tiny_prefill_case()
    w_dev = model.weights_to(w, DEV)
    eng0, want = _engine_run(cfg, w_dev, lens, page, B, prompts, bt, NATIVE, graph)
    for layout in REF_LAYOUTS:
        eng, got = _engine_run(cfg, w_dev, lens, page, B, prompts, bt, layout, graph)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (ids[layout], i)
        for l in range(cfg.num_layers):
            assert torch.equal(eng.kv[l], _to(eng0.kv[l], layout)), (ids[layout], l)
        with pytest.raises(_C.Mi355Error):                      # the layout is fixed once something was enqueued
            eng.set_kv_layout(NATIVE)
        assert eng.kv_layout == layout
    with pytest.raises(_C.Mi355Error):
        eng0.set_kv_layout(REF)


def test_engine_refuses_a_reference_layout_on_an_int8_cache_and_unknown_values():
    cfg, w, lens, page, B, prompts, bt = _tiny_prefill_case()
    w_dev = model.weights_to(w, DEV)
    kw = dict(page=page, num_blocks=B * 16, max_batch=4, max_seq_len=256, device=DEV)
    for layout in REF_LAYOUTS:
        with pytest.raises(_C.Mi355Error):
            model.DecoderEngine(cfg, w_dev, kv_int8=True, kv_layout=layout, **kw)
    with pytest.raises(_C.Mi355Error):
        model.DecoderEngine(cfg, w_dev, kv_int8=False, kv_layout=7, **kw)
    eng = model.DecoderEngine(cfg, w_dev, kv_int8=True, **kw)   # native on INT8 stays what it was
    eng.set_kv_layout(NATIVE)
    with pytest.raises(_C.Mi355Error):
        eng.set_kv_layout(VVEC)


# ------------------------------------------------------------------ 10. hand-over in both directions
@layouts
def test_decode_impl_on_top_of_a_cache_somebody_else_prefilled(layout):
    """(a) the host codec stands in for the reference's prefill op: it writes a 3-sequence prompt's K/V into a cache in the reference's layout;
    one Mi355PagedDecodeImpl step on top of it (its own KV write included) matches the oracle's attention over prompt + new token."""
    nh, nkv, hd, page, ctx = 8, 2, 64, 16, [37, 5, 100]
    B, mb = len(ctx), 8
    g = _gen(51)
    cfg = model.ModelConfig("t", 1, nh * hd, nh, nkv, hd, 64, 128, max_pos=mb * page)
    cs = oracle.rope_cos_sin(hd, cfg.rope_theta, cfg.max_pos)
    bt = torch.randperm(B * mb, generator=g).reshape(B, mb).to(torch.int32)
    kv, _ = kvcache.alloc_layer_cache(B * mb, nkv, page, hd, False, DEV)
    nat = []
    for b in range(B):
        K, V = torch.randn(ctx[b], nkv, hd, generator=g).half(), torch.randn(ctx[b], nkv, hd, generator=g).half()
        kvcache.write_tokens(kv, None, bt[b], 0, K, V, layout=layout)
        nat.append((K, V))
    qkv = (torch.randn(B, (nh + 2 * nkv) * hd, generator=g) * 0.5).half()
    acfg = attention.AttentionConfigs(nh, nkv, hd, hd, cfg.rope_theta, mb * page, 1.0, page, kv_layout=layout)
    ai = attention.PyAttentionInputs(False, torch.tensor(ctx, dtype=torch.int32), None, bt.to(DEV))
    impl = attention.AttnImplFactory.get_fmha_impl(acfg, ai, None, cos_sin=cs.to(DEV))
    assert type(impl) is attention.Mi355PagedDecodeImpl
    out = impl.forward(qkv.to(DEV), attention.LayerKVCache(kv, None, page, 0)).cpu()
    pos = torch.tensor(ctx, dtype=torch.int32)
    qh = oracle.apply_rope(qkv[:, : nh * hd].reshape(B, nh, hd), pos, cs)
    kh = oracle.apply_rope(qkv[:, nh * hd: (nh + nkv) * hd].reshape(B, nkv, hd), pos, cs)
    vh = qkv[:, (nh + nkv) * hd:].reshape(B, nkv, hd)
    for b in range(B):
        K, V = torch.cat([nat[b][0], kh[b:b + 1]]), torch.cat([nat[b][1], vh[b:b + 1]])
        ref = oracle.attention_decode(qh[b], K, V, 1 / math.sqrt(hd)).reshape(-1)
        assert torch.allclose(out[b].float(), ref.float(), **TOL), (b, float((out[b].float() - ref.float()).abs().max()))


@layouts
def test_prefill_impl_leaves_a_cache_somebody_else_can_read(layout):
    """(b) Mi355PrefillImpl writes the prompt; the host codec (standing in for the reference's reader) returns the oracle's rotated K and V
    from the reference's layout; the rows' outputs are the oracle's causal attention."""
    nh, nkv, hd, page, lens = 8, 2, 64, 16, [37, 5, 100]
    B, mb = len(lens), 8
    g = _gen(52)
    cfg = model.ModelConfig("t", 1, nh * hd, nh, nkv, hd, 64, 128, max_pos=mb * page)
    cs = oracle.rope_cos_sin(hd, cfg.rope_theta, cfg.max_pos)
    bt = torch.randperm(B * mb, generator=g).reshape(B, mb).to(torch.int32)
    kv, _ = kvcache.alloc_layer_cache(B * mb, nkv, page, hd, False, DEV)
    T = sum(lens)
    qkv = (torch.randn(T, (nh + 2 * nkv) * hd, generator=g) * 0.5).half()
    acfg = attention.AttentionConfigs(nh, nkv, hd, hd, cfg.rope_theta, mb * page, 1.0, page, kv_layout=layout)
    ai = attention.PyAttentionInputs(True, None, torch.tensor(lens, dtype=torch.int32), bt.to(DEV))
    impl = attention.AttnImplFactory.get_fmha_impl(acfg, ai, None, cos_sin=cs.to(DEV))
    assert type(impl) is attention.Mi355PrefillImpl
    out = impl.forward(qkv.to(DEV), attention.LayerKVCache(kv, None, page, 0)).cpu()
    assert out.shape == (T, nh * hd)
    t0 = 0
    for b, n in enumerate(lens):
        rows = qkv[t0:t0 + n]
        pos = torch.arange(n, dtype=torch.int32)
        qh = oracle.apply_rope(rows[:, : nh * hd].reshape(n, nh, hd), pos, cs)
        kh = oracle.apply_rope(rows[:, nh * hd: (nh + nkv) * hd].reshape(n, nkv, hd), pos, cs)
        vh = rows[:, (nh + nkv) * hd:].reshape(n, nkv, hd)
        K, V, _, _ = kvcache.read_tokens(kv, None, bt[b], n, layout=layout)
        assert torch.allclose(K.cpu().float(), kh.float(), **TOL)
        assert torch.equal(V.cpu(), vh)                          # V is a pure copy: bit exact
        for i in range(n):
            ref = oracle.attention_decode(qh[i], kh[: i + 1], vh[: i + 1], 1 / math.sqrt(hd)).reshape(-1)
            assert torch.allclose(out[t0 + i].float(), ref.float(), **TOL), (b, i, float((out[t0 + i].float() - ref.float()).abs().max()))
        t0 += n


# ------------------------------------------------------------------ 11. module graph, prefill to decode through the plug-in lists
def test_module_graph_prefill_then_decode_matches_oracle():
    """Qwen2DecoderModel with prepare_fmha_impl choosing Mi355PrefillImpl, then Mi355PagedDecodeImpl: the prompts of
    test_prefill_ragged_prompts_multi_chunk_matches_oracle (150 / 97 / 201 tokens) in two prefill calls of at most 128 tokens per sequence
    (the second one without the sequence that is done, prefix_lengths = 128), native layout and REF; logits of every last prompt token
    and of three further teacher-forced steps against OracleDecoder at that test's tolerance (1e-2)."""
    cfg, w, lens, page, B, prompts, bt = _tiny_prefill_case()
    odec = oracle.OracleDecoder({**cfg.__dict__}, _oracle_weights(w))
    okv = oracle.OracleKV(cfg.num_layers, B, False)
    ref_last = []
    for b, pr in enumerate(prompts):
        for pos, tok in enumerate(pr):
            _, lg = odec.forward_tokens(torch.tensor([tok], dtype=torch.int32), torch.tensor([pos], dtype=torch.int32), okv, [b])
        ref_last.append(lg[0])
    ref_steps, toks = [torch.stack(ref_last)], []
    tok = oracle.greedy(ref_steps[0])
    for step in range(3):
        toks.append(tok)
        _, ref = odec.forward_tokens(tok, torch.tensor([n + step for n in lens], dtype=torch.int32), okv, list(range(B)))
        ref_steps.append(ref)
        tok = oracle.greedy(ref)
    w_dev = model.weights_to(w, DEV)
    CH = 128
    for layout in (NATIVE, REF):
        pym = model.Qwen2DecoderModel(cfg, w_dev, page, 256, kv_layout=layout)
        kvs = [model.LayerKVCache(*kvcache.alloc_layer_cache(B * 16, cfg.nkv, page, cfg.hd, False, DEV), page, i) for i in range(cfg.num_layers)]
        last = [None] * B
        for c0 in (0, CH):
            seqs = [b for b in range(B) if lens[b] > c0]
            n = [min(CH, lens[b] - c0) for b in seqs]
            ids_ = torch.tensor([t for b, k in zip(seqs, n) for t in prompts[b][c0:c0 + k]], dtype=torch.int32)
            cu = torch.tensor([0] + list(np.cumsum(n)), dtype=torch.int32)
            ai = model.PyAttentionInputs(True, None, torch.tensor(n, dtype=torch.int32), bt[seqs].to(DEV),
                                         prefix_lengths=torch.tensor([c0] * len(seqs), dtype=torch.int32), cu_seqlens=cu)
            impl = pym.prepare_fmha_impl(ai)
            assert type(impl) is attention.Mi355PrefillImpl
            hid = pym(ids_.to(DEV), impl, kvs)
            assert hid.shape == (int(cu[-1]), cfg.hidden)
            for j, b in enumerate(seqs):
                if c0 + n[j] == lens[b]:
                    last[b] = int(cu[j + 1]) - 1
            done = [b for b in seqs if c0 + min(CH, lens[b] - c0) == lens[b]]
            rows = torch.tensor([last[b] for b in done], device=DEV)
            lg = pym.logits(hid.index_select(0, rows)).cpu()
            for j, b in enumerate(done):
                err = float((lg[j] - ref_steps[0][b]).abs().max())
                print(f"module prefill layout {layout} seq {b}: max |logit err| {err:.3e}")
                assert torch.allclose(lg[j], ref_steps[0][b], **TOL), (layout, b, err)
        for step in range(3):
            ai = model.PyAttentionInputs(False, torch.tensor([n + step for n in lens], dtype=torch.int32), None, bt.to(DEV))
            impl = pym.prepare_fmha_impl(ai)
            assert type(impl) is attention.Mi355PagedDecodeImpl
            lg = pym.logits(pym(toks[step].to(DEV), impl, kvs)).cpu()
            err = float((lg - ref_steps[step + 1]).abs().max())
            print(f"module decode layout {layout} step {step}: max |logit err| {err:.3e}")
            assert torch.allclose(lg, ref_steps[step + 1], **TOL), (layout, step, err)
