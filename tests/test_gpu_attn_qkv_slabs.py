"""Decode attention that folds the QKV projection's split-K slabs in its prologue (ops.paged_attention_qkv_slabs_img): bias + RoPE +
KV write inside the attention launch, the new token attended to from registers.  Against the CPU oracle and against the composed pair
it replaces (qkv_rope_kv_write_img, then paged_attention_rows_img), at every seam of the page walk; refusals; the step driver on the new
QKV selector, eager and captured.  TOL is the project's 1e-2 (test_gpu_fused_linear.py)."""
import ctypes as C
import math

import pytest
import torch

from oracle import oracle
from rtp_llm_amd import _C, kvcache, model, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-2, rtol=1e-2)
PAGE, MAX_BLOCKS = 16, 24
# positions of the new token: nothing cached | inside the first requested group | last / first slot of a page (the block id comes from
# the next table entry) | group and partition boundary | a later partition (P > 1 at 5 and 17 rows) | the last slot of the table
SEAMS = [0, 5, PAGE - 1, PAGE, 127, 128, 300, MAX_BLOCKS * PAGE - 1]


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _C.lib()


def _w4(K, N, seed):
    """(packed W4 g128 weight, dense fp32 reference)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    c_dev = model.synth_linear(K, N, "w4", DEV, gen, group_size=128, zeros="centered")
    c = model.weights_to({"w": c_dev}, "cpu")["w"]
    return c_dev.pack(), oracle.dequant_groupwise(c.q, c.z_eff, c.scales, c.group_size)


def _slabs(x_dev, packed):
    """fp32 split-K slabs [n, T, N_pad] of x W.  ops.linear_partial_img where its plan takes the shape (Qwen2-7B's QKV); hidden 512 is
    too shallow for that launch's eight K slices (test_linear_partial_img_refuses_shapes_outside_its_plan pins the refusal), so there the
    slabs come from the row-major split-K launch -- the producer the step driver uses at such widths."""
    s = ops.linear_partial_img(ops.act_image_pack(x_dev), packed)
    if s is not None:
        return s
    T = x_dev.shape[0]
    slabs = torch.empty(16, T, packed.N_pad, dtype=torch.float32, device=DEV)
    ws = ops.weight_struct(packed, x_dev.dtype)
    n = _C.check(_C.lib().mi355_linear_partial(x_dev.data_ptr(), T, C.byref(ws), slabs.data_ptr(), 16, torch.cuda.current_stream().cuda_stream),
                 "linear_partial")
    return slabs[:n]


_WEIGHTS = {}


def _weights(hidden, N):
    if (hidden, N) not in _WEIGHTS:
        _WEIGHTS[(hidden, N)] = _w4(hidden, N, hidden + N)
    return _WEIGHTS[(hidden, N)]


def _run_case(nh, nkv, hd, hidden, T, dtype, off):
    N = (nh + 2 * nkv) * hd
    packed, W = _weights(hidden, N)
    max_seq, nblk = MAX_BLOCKS * PAGE, T * MAX_BLOCKS
    cfg = model.ModelConfig("t", 1, hidden, nh, nkv, hd, 64, 128, max_pos=max_seq)
    cs = oracle.rope_cos_sin(hd, cfg.rope_theta, cfg.max_pos)
    g = torch.Generator().manual_seed(1000 * T + off + nh)
    x = (torch.randn(T, hidden, generator=g) * 0.5).to(dtype)
    bias = (torch.randn(N, generator=g) * 0.1).to(dtype)
    pos = torch.tensor([SEAMS[(t + off) % len(SEAMS)] for t in range(T)], dtype=torch.int32)
    bt = torch.randperm(nblk, generator=g)[: T * MAX_BLOCKS].reshape(T, MAX_BLOCKS).to(torch.int32)
    kv, _ = kvcache.alloc_layer_cache(nblk, nkv, PAGE, hd, False, DEV, dtype)
    kv.copy_(torch.randn(kv.shape, generator=g).to(dtype))
    before = kv.clone()
    xd, bd, csd, pd, btd = x.to(DEV), bias.to(DEV), cs.to(DEV), pos.to(DEV), bt.to(DEV)
    slabs = _slabs(xd, packed)
    out = ops.paged_attention_qkv_slabs_img(slabs, bd, csd, pd, btd, kv, None, nh, nkv, hd, PAGE, max_seq)
    assert out is not None
    torch.cuda.synchronize()
    got = out.unpack().cpu().float()
    # ---- oracle: attention over (cache + the oracle's rotated k, v of the new token)
    qkv = oracle.linear(x, W, bias)
    qh = qkv[:, : nh * hd].reshape(T, nh, hd)
    kh = qkv[:, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd)
    vh = qkv[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    q_ref, k_ref = oracle.apply_rope(qh, pos, cs), oracle.apply_rope(kh, pos, cs)
    expected = before.clone()
    worst = [0.0, 0.0, 0.0]
    for t in range(T):
        p = int(pos[t])
        Kc, Vc, _, _ = kvcache.read_tokens(before, None, bt[t], p)
        ref = oracle.attention_decode(q_ref[t], torch.cat((Kc.cpu(), k_ref[t][None])), torch.cat((Vc.cpu(), vh[t][None])), 1 / math.sqrt(hd)).reshape(-1).float()
        worst[0] = max(worst[0], float((got[t] - ref).abs().max()))
        assert torch.allclose(got[t], ref, **TOL), (t, p, float((got[t] - ref).abs().max()))
        Kn, Vn, _, _ = kvcache.read_tokens(kv, None, bt[t], p + 1)
        worst[1] = max(worst[1], float((Kn[-1].cpu().float() - k_ref[t].float()).abs().max()))
        worst[2] = max(worst[2], float((Vn[-1].cpu().float() - vh[t].float()).abs().max()))
        assert torch.allclose(Kn[-1].cpu().float(), k_ref[t].float(), **TOL), (t, p)
        assert torch.allclose(Vn[-1].cpu().float(), vh[t].float(), **TOL), (t, p)
        kvcache.write_tokens(expected, None, bt[t], p, Kn[-1:], Vn[-1:])
    print(f"nh={nh} hd={hd} T={T} {dtype} off={off} slabs={slabs.shape[0]}: max |out - oracle| {worst[0]:.2e}, |k - oracle| {worst[1]:.2e}, |v - oracle| {worst[2]:.2e}")
    # every element of the pool except the T new slots is bit-identical to before
    assert torch.equal(kv, expected)
    # ---- the composed pair it replaces leaves the same cache image and the same output (same tolerance)
    kv2 = before.clone()
    q2 = ops.qkv_rope_kv_write_img(ops.act_image_pack(xd), packed, bd, csd, pd, btd, kv2, None, nh, nkv, hd, PAGE, 1)
    assert q2 is not None
    out2 = ops.paged_attention_rows_img(q2, kv2, None, btd, pd, nkv, PAGE, 1, max_seq).unpack().cpu().float()
    assert torch.allclose(got, out2, **TOL), float((got - out2).abs().max())
    assert torch.allclose(kv.float(), kv2.float(), **TOL)
    assert torch.equal((kv != before).reshape(nblk, -1).any(1), (kv2 != before).reshape(nblk, -1).any(1))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T", [5, 17, 64])
@pytest.mark.parametrize("nh,nkv,hd", [(14, 2, 128), (4, 2, 64)], ids=["g7-hd128", "g2-hd64"])
def test_attn_qkv_slabs_vs_oracle_and_composed_pair(nh, nkv, hd, T, dtype):
    """hidden 512; rows 5 / 17 / 64; every seam position in every case (5 rows: two launches), P > 1 at 5 and 17 rows."""
    for off in range(0, len(SEAMS), T):
        _run_case(nh, nkv, hd, 512, T, dtype, off)


def test_attn_qkv_slabs_from_the_image_launch_qwen2_7b_heads():
    """Qwen2-7B's QKV (K 3584, 28 / 4 heads of 128): the slabs come from linear_partial_img, 64 rows x 4 kv heads = one partition."""
    packed, _ = _weights(3584, 4608)
    x = torch.zeros(64, 3584, dtype=torch.float16, device=DEV)
    assert ops.linear_partial_img(ops.act_image_pack(x), packed) is not None
    _run_case(28, 4, 128, 3584, 64, torch.float16, 0)


def test_attn_qkv_slabs_stale_rows_and_refusals():
    nh, nkv, hd, hidden, page = 4, 2, 64, 512, 16             # (the writer's test uses page 8; the attention launch takes pages from 16)
    N = (nh + 2 * nkv) * hd
    packed, _ = _weights(hidden, N)
    max_blocks, nblk, T = 4, 256, 20
    cfg = model.ModelConfig("t", 1, hidden, nh, nkv, hd, 64, 128, max_pos=max_blocks * page)
    cs = oracle.rope_cos_sin(hd, cfg.rope_theta, cfg.max_pos).to(DEV)
    x = (torch.randn(T, hidden, generator=torch.Generator().manual_seed(1)) * 0.5).half().to(DEV)
    pos = torch.full((T,), 3, dtype=torch.int32, device=DEV)
    pos[1] = -1; pos[2] = max_blocks * page + 7                                            # padding row, past the table
    bt = torch.arange(T * max_blocks, dtype=torch.int32, device=DEV).reshape(T, max_blocks)
    bt[3, 0] = nblk + 5                                                                      # stale block id
    kv, sc = kvcache.alloc_layer_cache(nblk, nkv, page, hd, False, DEV)
    oob = torch.zeros(1, dtype=torch.int32, device=DEV)
    before = kv.clone()
    slabs = _slabs(x, packed)
    out = ops.paged_attention_qkv_slabs_img(slabs, None, cs, pos, bt, kv, sc, nh, nkv, hd, page, max_blocks * page, 1, oob)
    torch.cuda.synchronize()
    assert out is not None and int(oob.item()) == 2          # rows 2 and 3 refused, row 1 is padding (not an error)
    changed = (kv != before).reshape(nblk, -1).any(dim=1).nonzero().flatten().tolist()
    assert changed == [t * max_blocks for t in range(T) if t not in (1, 2, 3)]
    o = out.unpack()
    assert torch.equal(o[1], torch.zeros_like(o[1])) and torch.isfinite(o).all()
    kv8, sc8 = kvcache.alloc_layer_cache(nblk, nkv, page, hd, True, DEV)
    assert ops.paged_attention_qkv_slabs_img(slabs, None, cs, pos, bt, kv8, sc8, nh, nkv, hd, page, max_blocks * page) is None      # INT8 cache
    assert ops.paged_attention_qkv_slabs_img(slabs, None, cs, pos[: T // 2].contiguous(), bt[: T // 2].contiguous(), kv, sc, nh, nkv, hd, page, max_blocks * page, 2) is None   # q_len > 1
    for lay in (_C.KV_LAYOUT_REF, _C.KV_LAYOUT_REF_VVEC):                                   # a reference layout
        assert ops.paged_attention_qkv_slabs_img(slabs, None, cs, pos, bt, kv, None, nh, nkv, hd, page, max_blocks * page, layout=lay) is None
    torch.cuda.synchronize()
    assert torch.equal((kv != before).reshape(nblk, -1).any(dim=1).nonzero().flatten().cpu(), torch.tensor(changed))   # the refused calls launched nothing


def _dense(c):
    return c.w.float() if c.kind == "fp16" else oracle.dequant_groupwise(c.q, c.z_eff, c.scales, c.group_size)


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("B", [5, 64])
def test_engine_takes_the_slab_selector_and_matches_oracle(B, mode, parity):
    """2-layer toy-width step driver at 5 and 64 rows: every step on the slab selector (asserted), greedy steps from position 0 across the
    page boundary at 16; the four steps 14..17 around it and all steps before them against OracleDecoder by test_gpu_parity's rule
    (logits within TOL, ids on safe rows)."""
    cfg = model.ModelConfig("tiny-qwen2", 2, 512, 8, 2, 64, 1024, 2048, max_pos=512)
    w = model.synth_model(cfg, "w4", "cpu", seed=3, zeros="centered")
    ow = {"embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": _dense(w["lm_head"]),
          "layers": [{"input_norm": L["input_norm"], "post_norm": L["post_norm"], "qkv_bias": L["qkv_bias"],
                      **{k: _dense(L[k]) for k in ("qkv", "o", "gate_up", "down")}} for L in w["layers"]]}
    odec = oracle.OracleDecoder({**cfg.__dict__}, ow)
    okv = oracle.OracleKV(cfg.num_layers, B, False)
    eng = model.DecoderEngine(cfg, model.weights_to(w, DEV), kv_int8=False, page=PAGE, num_blocks=B * 2, max_batch=B, max_seq_len=32, device=DEV)
    bt = torch.randperm(B * 2, generator=torch.Generator().manual_seed(1)).reshape(B, 2).to(torch.int32)
    tok = torch.randint(0, cfg.vocab, (B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    eng.set_inputs(tok.tolist(), [0] * B, bt)
    eng.set_qkv_slab_rows(5)           # the path is opt-in (its sums run in another order than the fused launch's): taken from its first row count
    if mode == "graph":
        eng.capture(B)
    for step in range(PAGE + 2):
        pos = torch.full((B,), step, dtype=torch.int32)
        eng.step(B) if mode == "eager" else eng.replay(B, 1)
        torch.cuda.synchronize()
        assert eng.qkv_launch() == 3
        _, ref = odec.forward_tokens(tok, pos, okv, list(range(B)))
        got = eng.logits[:B].cpu()
        assert torch.allclose(got, ref, **TOL), (step, float((got - ref).abs().max()))
        nxt = oracle.greedy(ref)
        parity.step(got_ids=eng.token_ids[:B].cpu(), ref_ids=nxt, ref_logits=ref, got_logits=got, tol=1e-2, label=f"step {step}")
        assert torch.equal(eng.positions[:B].cpu(), pos + 1)
        tok = nxt
        eng.token_ids[:B].copy_(tok)
    assert eng.oob_count() == 0
