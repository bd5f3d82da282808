"""Launch heads (kernarg preload): gemm_fullk64_kernel, paged_attn_kernel / attn_reduce_kernel and gemm_splitk64_kernel take the
fields they need first as leading scalar kernel parameters and the parameter struct behind them.  What can go wrong is a head field bound to the
wrong slot, truncated, or stale from the launch before -- so every test drives one of these entry points through the Python / ctypes path of the
existing kernel tests as call A, call B (every head field that the entry point lets a caller vary takes another value), call A again:
A's two results are bit-equal, and A and B sit inside the reference tolerance of the existing tests of that entry point (tests/test_gpu_fused_linear.py,
tests/test_gpu_native_ops.py, tests/test_gpu_kv_layout.py: fp32 torch / oracle reference, atol = rtol = 1e-2).  Nothing here depends on whether the
machine's firmware honours the preload: the results are the same either way.

gemm_wide_kernel keeps its struct (its head needs 17 dwords, the budget is 14: DESIGN.md §9), so it has no test here."""
import math

import pytest
import torch

from oracle import oracle
from rtp_llm_amd import kvcache, model, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-2, rtol=1e-2)


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    from rtp_llm_amd import _C
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _C.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _w4(K, N, seed):
    """(packed W4 g128 weight, dense fp32 reference): the helper of tests/test_gpu_fused_linear.py"""
    c_dev = model.synth_linear(K, N, "w4", DEV, torch.Generator(device=DEV).manual_seed(seed), group_size=128, zeros="centered")
    c = model.weights_to({"w": c_dev}, "cpu")["w"]
    return c_dev.pack(), oracle.dequant_groupwise(c.q, c.z_eff, c.scales, c.group_size)


def _aba(call_a, call_b):
    """A, B, A in one process; returns (A's first result, B's result) after checking that A's second result has the same bits."""
    a1 = call_a()
    b = call_b()
    a2 = call_a()
    torch.cuda.synchronize()
    for x, y in zip(a1, a2):
        assert torch.equal(x, y), "call A after call B does not repeat call A: a head field is stale"
    return a1, b


# ------------------------------------------------------------------ full-K image launches (gemm_fullk64.hip)
HIDDEN, NH, NKV, HD, PAGE = 512, 4, 2, 128, 16           # N = (4 + 2 * 2) * 128 = 1024


@pytest.fixture(scope="module")
def qkv_case():
    N = (NH + 2 * NKV) * HD
    cfg = model.ModelConfig("t", 1, HIDDEN, NH, NKV, HD, 64, 128, max_pos=3 * PAGE)
    return {"N": N, "w": [_w4(HIDDEN, N, 11), _w4(HIDDEN, N, 12)], "cs": oracle.rope_cos_sin(HD, cfg.rope_theta, cfg.max_pos),
            "bias": (torch.randn(N, generator=_gen(4)) * 0.1).half()}


def _qkv_call(case, wi, M, max_blocks, seed):
    """One QKV + RoPE + KV write launch on its own cache; positions 15 and 16 alternate (last slot of page 0, first of page 1)."""
    packed, W = case["w"][wi]
    nblk = 64 * 3
    g = _gen(seed)
    x = (torch.randn(M, HIDDEN, generator=g) * 0.5).half()
    pos = torch.tensor([15 + (m & 1) for m in range(M)], dtype=torch.int32)
    bt = torch.randperm(nblk, generator=g)[: M * max_blocks].reshape(M, max_blocks).to(torch.int32)
    kv, sc = kvcache.alloc_layer_cache(nblk, NKV, PAGE, HD, False, DEV)
    q = ops.qkv_rope_kv_write_img(ops.act_image_pack(x.to(DEV)), packed, case["bias"].to(DEV), case["cs"].to(DEV), pos.to(DEV), bt.to(DEV), kv, sc,
                                  NH, NKV, HD, PAGE, 1)
    assert q is not None, "W4 g128, 1-64 rows, K = 512: the image kernel must take it"
    return (q, kv), (x, W, pos, bt, sc)


def _qkv_check(case, got, inputs):
    (q, kv), (x, W, pos, bt, sc) = got, inputs
    M = x.shape[0]
    qkv = oracle.linear(x, W, case["bias"])
    qh = qkv[:, : NH * HD].reshape(M, NH, HD)
    kh = qkv[:, NH * HD: (NH + NKV) * HD].reshape(M, NKV, HD)
    vh = qkv[:, (NH + NKV) * HD:].reshape(M, NKV, HD)
    q_ref, k_ref = oracle.apply_rope(qh, pos, case["cs"]), oracle.apply_rope(kh, pos, case["cs"])
    assert torch.allclose(q.cpu().float(), q_ref.float(), **TOL), f"M={M}: q max err {(q.cpu().float() - q_ref.float()).abs().max()}"
    written = set()
    for t in range(M):
        K, V, _, _ = kvcache.read_tokens(kv, sc, bt[t], int(pos[t]) + 1)
        assert torch.allclose(K[-1].cpu().float(), k_ref[t].float(), **TOL), t
        assert torch.allclose(V[-1].cpu().float(), vh[t].float(), **TOL), t
        written.add(int(bt[t, int(pos[t]) // PAGE]))
    changed = (kv != 0).reshape(kv.shape[0], -1).any(1).nonzero().flatten().tolist()     # alloc_layer_cache hands out zeros
    assert set(changed) == written, "pages other than the rows' own were written (or theirs were not)"


def test_fullk64_qkv_rope_head(qkv_case):
    """rows 5 / 64 (one / four row blocks), two weight tensors, table widths 2 / 3, positions 15 and 16 (two table slots, two pages)."""
    keep = {}
    def call(tag, wi, M, max_blocks, seed):
        def run():
            got, inputs = _qkv_call(qkv_case, wi, M, max_blocks, seed)
            keep[tag] = inputs
            return got
        return run
    a, b = _aba(call("a", 0, 5, 2, 1), call("b", 1, 64, 3, 2))
    _qkv_check(qkv_case, a, keep["a"])
    _qkv_check(qkv_case, b, keep["b"])


def test_fullk64_o_residual_head():
    """O + residual (+ per-tile sums of squares): K = nh * hd = 512, N = hidden = 512; rows 5 / 64, two weight tensors, with / without bias."""
    K = N = 512
    ws = [_w4(K, N, 21), _w4(K, N, 22)]
    x = (torch.randn(64, K, generator=_gen(3)) * 0.5).half()
    res = (torch.randn(64, N, generator=_gen(5)) * 2.0).half()
    bias = (torch.randn(N, generator=_gen(4)) * 0.1).half()
    def call(wi, M, b):
        def run():
            ssq = torch.zeros(M, (N // 16 + 3) & ~3, dtype=torch.float32, device=DEV)
            out = ops.linear_residual_img(ops.act_image_pack(x[:M].contiguous().to(DEV)), ws[wi][0], res[:M].contiguous().to(DEV),
                                          b.to(DEV) if b is not None else None, tile_sumsq=ssq)
            assert out is not None
            return out, ssq
        return run
    (oa, sa), (ob, sb) = _aba(call(0, 5, bias), call(1, 64, None))
    for out, ssq, wi, M, b in ((oa, sa, 0, 5, bias), (ob, sb, 1, 64, None)):
        ref = (oracle.linear(x[:M], ws[wi][1], b).float() + res[:M].float()).half()
        assert torch.allclose(out.cpu().float(), ref.float(), **TOL), f"M={M}: max err {(out.cpu().float() - ref.float()).abs().max()}"
        assert torch.allclose(ssq[:, : N // 16].sum(1).cpu(), (out.cpu().float() ** 2).sum(1), rtol=1e-5)


# ------------------------------------------------------------------ attention (attention.hip)
def _attn_cache(ctx, page, max_blocks, seed):
    """2 sequences x 2 kv heads of 128 on a junk-filled pool (tests/test_gpu_kv_layout.py _fill_cache); returns cache, table, per-sequence K / V"""
    B, nblk = len(ctx), 16
    g = _gen(seed)
    bt = torch.randperm(nblk, generator=g)[: B * max_blocks].reshape(B, max_blocks).to(torch.int32)
    kv, _ = kvcache.alloc_layer_cache(nblk, NKV, page, HD, False, DEV)
    kv.copy_(torch.randn(kv.shape, generator=g).half())
    KV = []
    for b in range(B):
        K, V = torch.randn(ctx[b], NKV, HD, generator=g).half(), torch.randn(ctx[b], NKV, HD, generator=g).half()
        kvcache.write_tokens(kv, None, bt[b], 0, K, V)
        KV.append((K, V))
    return kv, bt, KV


def test_attention_heads():
    """G = 2 (4 query heads on 2 kv heads), hd 128.
    A: decode rows (seq_lens, seq_add 0, q_len 1, one row tile), contexts 1 and 17, page 16, table width 8, max_seq_len 128: one partition, no reduce launch.
    B: 17 rows per sequence (positions, seq_add 1, q_len 17: two row tiles of 2 x 8 rows), contexts 17..33 and 1..17, page 64, table width 3,
       max_seq_len 129: the smallest at which two sequences take a second partition, so attn_reduce_kernel runs (A's 128 is the largest below it)."""
    nh = NKV * 2
    kva, bta, KVa = _attn_cache([1, 17], 16, 8, 41)
    qa = torch.randn(2, nh, HD, generator=_gen(6)).half().to(DEV)
    sla = torch.tensor([1, 17], dtype=torch.int32, device=DEV)
    q_len = 17
    kvb, btb, KVb = _attn_cache([33, 17], 64, 3, 42)
    qb = torch.randn(2 * q_len, nh, HD, generator=_gen(7)).half().to(DEV)
    posb = torch.tensor([[16 + i for i in range(q_len)], [i for i in range(q_len)]], dtype=torch.int32).reshape(-1)
    (oa,), (ob,) = _aba(lambda: (ops.paged_decode_attention(qa, kva, None, bta.to(DEV), sla, NKV, 16, 128),),
                        lambda: (ops.paged_attention_rows(qb, kvb, None, btb.to(DEV), posb.to(DEV), NKV, 64, q_len, 129),))
    scale = 1 / math.sqrt(HD)
    for b, c in enumerate([1, 17]):
        ref = oracle.attention_decode(qa[b].cpu(), KVa[b][0][:c], KVa[b][1][:c], scale).reshape(-1)
        assert torch.allclose(oa[b].cpu().float(), ref.float(), **TOL), ("A", b)
    for r in range(2 * q_len):
        b, c = r // q_len, int(posb[r]) + 1
        ref = oracle.attention_decode(qb[r].cpu(), KVb[b][0][:c], KVb[b][1][:c], scale).reshape(-1)
        assert torch.allclose(ob[r].cpu().float(), ref.float(), **TOL), ("B", r)


# ------------------------------------------------------------------ split-K image launch (gemm_splitk64.hip)
def test_splitk64_head():
    """N = 512 (8 column groups of four tiles), two weight tensors, rows 5 / 17 / 64, slab count read back from every call.
    K = 1024 with one slab allowed is one K split of 8 chunks (one per wave); K = 2048 with two is two splits on four XCDs each.  K = 512 is four chunks,
    fewer than the kernel's eight K-slice waves: its plan refuses that (tests/test_gpu_fused_linear.py pins the refusal), so there is no launch to check."""
    N = 512
    ws = {1024: _w4(1024, N, 31), 2048: _w4(2048, N, 32)}
    x = (torch.randn(64, 2048, generator=_gen(3)) * 0.5).half()
    def call(K, M, max_splits, want_slabs):
        def run():
            slabs = ops.linear_partial_img(ops.act_image_pack(x[:M, :K].contiguous().to(DEV)), ws[K][0], max_splits)
            assert slabs is not None and slabs.shape[0] == want_slabs, None if slabs is None else slabs.shape
            return (slabs,)
        return run
    def check(slabs, K, M):
        y, ref = slabs.sum(0)[:, :N].cpu(), x[:M, :K].float() @ ws[K][1]
        assert torch.allclose(y, ref, **TOL), f"K={K} M={M}: max err {(y - ref).abs().max()}"
    (sa,), (sb,) = _aba(call(1024, 5, 1, 1), call(2048, 64, 2, 2))
    check(sa, 1024, 5); check(sb, 2048, 64)
    (sc,), (sd,) = _aba(call(2048, 17, 2, 2), call(1024, 64, 1, 1))
    check(sc, 2048, 17); check(sd, 1024, 64)
    w512, _ = _w4(512, N, 33)
    assert ops.linear_partial_img(ops.act_image_pack(x[:5, :512].contiguous().to(DEV)), w512) is None


# ------------------------------------------------------------------ the captured step
@pytest.mark.parametrize("B", [5, 17])
def test_captured_step_equals_the_eager_step(B):
    """A 2-layer engine on the image launches (5 rows up): the graph's kernel nodes carry head + struct; replayed twice, with the inputs changed
    through set_inputs in between, it leaves the bits of the eager step."""
    cfg = model.ModelConfig("heads-qwen2", 2, 512, 8, 2, 64, 1024, 2048, max_pos=256)
    w = model.weights_to(model.synth_model(cfg, "w4", "cpu", seed=13, zeros="centered"), DEV)
    mk = lambda: model.DecoderEngine(cfg, w, kv_int8=False, page=16, num_blocks=B * 4, max_batch=B, max_seq_len=64, device=DEV)
    eager, graph = mk(), mk()
    g = _gen(B)
    ins = [(torch.randint(0, cfg.vocab, (B,), generator=g).tolist(), [(3 * i) % 11 for i in range(B)], torch.randperm(B * 4, generator=g).reshape(B, 4)),
           (torch.randint(0, cfg.vocab, (B,), generator=g).tolist(), [15 + (i & 1) for i in range(B)], torch.randperm(B * 4, generator=g).reshape(B, 4))]
    graph.set_inputs(*ins[0])
    graph.capture(B)
    for tok, pos, bt in ins:
        eager.set_inputs(tok, pos, bt); graph.set_inputs(tok, pos, bt)
        eager.step(B); graph.replay(B, 1)
        torch.cuda.synchronize()
        assert torch.equal(graph.logits[:B], eager.logits[:B]) and torch.equal(graph.token_ids[:B], eager.token_ids[:B])
        assert bool(torch.isfinite(eager.logits[:B]).all())
    for l in range(cfg.num_layers):
        assert torch.equal(graph.kv[l], eager.kv[l]), l
    assert eager.oob_count() == 0 and graph.oob_count() == 0
