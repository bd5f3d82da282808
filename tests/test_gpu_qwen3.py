"""Qwen3 dense models on the MI355X: the per-head QK RMSNorm in the RoPE / KV writer (mi355_rope_kv_write_rows_qk_norm), the
stand-alone op (mi355_qk_rmsnorm), the step driver with mi355_decoder_set_qk_norm (hipGraph replay, prefill, verify rows, TP), the
module graph and an HF checkpoint end to end -- each against the CPU reference of tests/qwen3_ref.py (or transformers itself)."""
import os
import socket
from dataclasses import replace

import pytest
import torch
import torch.multiprocessing as mp

from oracle import oracle
from rtp_llm_amd import _C, kvcache, loader, model, ops

import qwen3_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-2, rtol=1e-2)


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _C.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ the writer
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("hd,nh,nkv", [(64, 8, 2), (128, 4, 2)])
@pytest.mark.parametrize("q_len", [1, 4])
def test_rope_kv_write_qk_norm(dtype, int8, hd, nh, nkv, q_len):
    page, max_blocks, nblk, nseq = 16, 8, 64, 3
    T = nseq * q_len
    cs = oracle.rope_cos_sin(hd, 1e6, max_blocks * page)
    g = _gen(hd + nh + q_len)
    W = (nh + 2 * nkv) * hd
    qkv = (torch.randn(T, W, generator=g) * 2).to(dtype)
    bias = (0.3 * torch.randn(W, generator=g)).to(dtype)
    qn, kn = (1 + 0.3 * torch.randn(hd, generator=g)).to(dtype), (1 + 0.3 * torch.randn(hd, generator=g)).to(dtype)
    starts = [0, 13, 100]
    pos = torch.tensor([s + i for s in starts for i in range(q_len)], dtype=torch.int32)
    bt = torch.randperm(nblk, generator=g)[: nseq * max_blocks].reshape(nseq, max_blocks).to(torch.int32)
    kv, sc = kvcache.alloc_layer_cache(nblk, nkv, page, hd, int8, DEV, dtype=dtype)
    q = ops.rope_kv_write_rows_qk_norm(qkv.to(DEV), bias.to(DEV), qn.to(DEV), kn.to(DEV), 1e-6, cs.to(DEV), pos.to(DEV), bt.to(DEV), kv, sc,
                                       nh, nkv, hd, page, q_len)
    torch.cuda.synchronize()
    x = (qkv.float() + bias.float()).to(dtype)                           # the QKV linear's rounded output
    xn = qwen3_ref.qk_norm(x, qn, kn, nh, nkv, hd, 1e-6)
    q_ref = oracle.apply_rope(xn[:, : nh * hd].reshape(T, nh, hd), pos, cs)
    k_ref = oracle.apply_rope(xn[:, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd), pos, cs)
    v_ref = x[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    tol = TOL if dtype == torch.float16 else dict(atol=3e-2, rtol=3e-2)
    assert torch.allclose(q.cpu().float(), q_ref.float(), **tol), float((q.cpu().float() - q_ref.float()).abs().max())
    for t in range(T):
        K, V, ks, vs = kvcache.read_tokens(kv, sc, bt[t // q_len], int(pos[t]) + 1)
        K, V = K[-1].cpu(), V[-1].cpu()
        if not int8:
            assert torch.allclose(K.float(), k_ref[t].float(), **tol)
            assert torch.equal(V, v_ref[t])                                  # V is not normed: a copy of the biased row, bit exact
        else:
            vq, vsc = oracle.quant_kv_int8(v_ref[t])
            assert torch.equal(V, vq) and torch.equal(vs[-1].cpu(), vsc)      # integer path of the un-normed V: bit exact
            kq, ksc = oracle.quant_kv_int8(k_ref[t])
            assert (K.int() - kq.int()).abs().max() <= 1                     # normed + rotated K: a 1-ulp difference may move one code
            assert torch.allclose(ks[-1].cpu(), ksc, rtol=1e-2, atol=0)


def test_rope_kv_write_without_norm_is_unchanged():
    """The Qwen2 / Llama entry point still rotates the un-normed rows (the norm is a separate template instance)."""
    hd, nh, nkv, page = 64, 4, 2, 16
    cs = oracle.rope_cos_sin(hd, 1e6, 128)
    qkv = (torch.randn(2, (nh + 2 * nkv) * hd, generator=_gen(1)) * 3).half()
    pos, bt = torch.tensor([3, 7], dtype=torch.int32), torch.tensor([[0], [1]], dtype=torch.int32)
    kv, sc = kvcache.alloc_layer_cache(4, nkv, page, hd, False, DEV)
    q = ops.rope_kv_write_rows(qkv.to(DEV), None, cs.to(DEV), pos.to(DEV), bt.to(DEV), kv, sc, nh, nkv, hd, page, 1)
    torch.cuda.synchronize()
    assert torch.allclose(q.cpu().float(), oracle.apply_rope(qkv[:, : nh * hd].reshape(2, nh, hd), pos, cs).float(), **TOL)


# ------------------------------------------------------------------ the stand-alone op
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hd,nh,nkv,T", [(64, 14, 2, 5), (128, 32, 8, 33), (128, 16, 8, 1)])
def test_qk_rmsnorm_op(dtype, hd, nh, nkv, T):
    g = _gen(hd * T)
    qkv = (torch.randn(T, (nh + 2 * nkv) * hd, generator=g) * 2).to(dtype)
    qn, kn = (1 + 0.3 * torch.randn(hd, generator=g)).to(dtype), (1 + 0.3 * torch.randn(hd, generator=g)).to(dtype)
    got = ops.qk_rmsnorm_(qkv.to(DEV), qn.to(DEV), kn.to(DEV), 1e-6, nh, nkv, hd).cpu()
    ref = torch.cat([oracle.rmsnorm(qkv[:, : nh * hd].reshape(T, nh, hd), qn, 1e-6).reshape(T, -1),
                     oracle.rmsnorm(qkv[:, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd), kn, 1e-6).reshape(T, -1)], dim=1)
    tol = TOL if dtype == torch.float16 else dict(atol=3e-2, rtol=3e-2)
    assert torch.allclose(got[:, : (nh + nkv) * hd].float(), ref.float(), **tol)
    assert torch.equal(got[:, (nh + nkv) * hd:], qkv[:, (nh + nkv) * hd:])   # V untouched
    # the module form is the same op
    from rtp_llm_amd.modules import FusedQKRMSNorm
    got2 = FusedQKRMSNorm(qn.to(DEV), kn.to(DEV), nh, nkv, hd, 1e-6)(qkv.to(DEV)).cpu()
    assert torch.equal(got2, got)


# ------------------------------------------------------------------ the step driver
def _run_engine(cfg, w, B, parity, *, steps=3, prompt=3, kv_int8=False, tol=1e-2, verify=False, seed=0):
    """Prefill of B prompts, then `steps` graph-replayed decode steps, against the reference (ids on safe rows, logits `tol`)."""
    page = 16
    nb = (prompt + steps + 4 + page - 1) // page + 1
    eng = model.DecoderEngine(cfg, model.weights_to(w, DEV), kv_int8=kv_int8, page=page, num_blocks=B * nb, max_batch=B,
                              max_seq_len=nb * page, device=DEV)
    ref = qwen3_ref.from_canonical(cfg, w)
    okv = oracle.OracleKV(cfg.num_layers, B, kv_int8)
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)
    prompts = torch.randint(0, cfg.vocab, (B, prompt), generator=_gen(seed), dtype=torch.int32)
    got = eng.prefill(prompts.tolist(), bt).cpu()
    toks = prompts.t().reshape(-1)                                     # token-major: a sequence's tokens stay in order
    pos = torch.arange(prompt, dtype=torch.int32).repeat_interleave(B)
    _, ref_all = ref.forward_tokens(toks, pos, okv, list(range(B)) * prompt)
    want = ref_all[-B:]
    assert torch.allclose(got, want, atol=tol, rtol=tol), ("prefill", float((got - want).abs().max()))
    parity.step(got_ids=got.argmax(-1).int(), ref_ids=oracle.greedy(want), ref_logits=want, got_logits=got, tol=tol, label="prefill")
    tok = oracle.greedy(want)
    eng.set_inputs(tok.tolist(), [prompt] * B, bt)
    eng.capture(B)
    # the launch plan is fixed now: the norms cannot be set again
    arr = C_void_p_array(cfg.num_layers)
    assert eng.lib.mi355_decoder_set_qk_norm(eng.handle, arr, arr) == _C.ERR_ARG
    for s in range(steps):
        p = torch.full((B,), prompt + s, dtype=torch.int32)
        _, want = ref.forward_tokens(tok, p, okv, list(range(B)))
        eng.replay(B, 1)
        torch.cuda.synchronize()
        got = eng.logits[:B].cpu()
        assert torch.allclose(got, want, atol=tol, rtol=tol), (s, float((got - want).abs().max()))
        parity.step(got_ids=eng.token_ids[:B].cpu(), ref_ids=oracle.greedy(want), ref_logits=want, got_logits=got, tol=tol, label=f"decode {s}")
        tok = oracle.greedy(want)
        eng.token_ids[:B].copy_(tok)
    if verify:   # speculative verify rows: q_len = 4 rows per sequence through the composed QKV path
        q_len, nseq = 4, B // 4
        base = prompt + steps
        vt = torch.randint(0, cfg.vocab, (nseq, q_len), generator=_gen(seed + 1), dtype=torch.int32)
        vp = (base + torch.arange(q_len, dtype=torch.int32)).repeat(nseq)
        eng.set_inputs(vt.reshape(-1).tolist(), vp.tolist(), bt[:nseq])
        eng.forward(nseq * q_len, q_len)
        torch.cuda.synchronize()
        got = eng.logits[: nseq * q_len].cpu()
        okv2 = okv   # sequences 0..nseq-1 continue from their cached tokens
        rows = []
        for i in range(q_len):   # one position at a time over all sequences keeps every sequence in order
            _, r = ref.forward_tokens(vt[:, i], torch.full((nseq,), base + i, dtype=torch.int32), okv2, list(range(nseq)))
            rows.append(r)
        want = torch.stack(rows, dim=1).reshape(nseq * q_len, -1)
        assert torch.allclose(got, want, atol=tol, rtol=tol), ("verify", float((got - want).abs().max()))
    assert eng.oob_count() == 0
    return eng


def C_void_p_array(n):
    import ctypes
    return (ctypes.c_void_p * n)(*([1] * n))


TOY64 = model.ModelConfig("toy-qwen3-hd64", 2, 512, 8, 2, 64, 1024, 2048, max_pos=256, qkv_bias=False, qk_norm=True)
TOY128 = model.ModelConfig("toy-qwen3-hd128", 2, 512, 8, 4, 128, 1024, 2048, max_pos=256, qkv_bias=False, qk_norm=True)   # nh*hd = 1024 != 512


@pytest.mark.parametrize("B", [1, 8, 64])
@pytest.mark.parametrize("cfg", [TOY64, TOY128], ids=["hd64", "hd128"])
def test_engine_qwen3_toy(cfg, B, parity):
    w = model.synth_model(cfg, "w4", "cpu", seed=7, zeros="centered")
    _run_engine(cfg, w, B, parity, verify=(B == 8))


def test_engine_qwen3_bias_and_int8_cache(parity):
    cfg = replace(TOY64, qkv_bias=True)
    w = model.synth_model(cfg, "w4", "cpu", seed=8, zeros="centered")
    _run_engine(cfg, w, 8, parity, kv_int8=True, tol=3e-2)


def test_engine_without_norm_differs():
    """set_qk_norm is what makes the difference: the same weights without the norms give other logits."""
    w = model.synth_model(TOY64, "w4", "cpu", seed=7, zeros="centered")
    plain = {**w, "layers": [{k: v for k, v in L.items() if k not in ("q_norm", "k_norm")} for L in w["layers"]]}
    outs = []
    for cfg, ww in ((TOY64, w), (replace(TOY64, qk_norm=False), plain)):
        eng = model.DecoderEngine(cfg, model.weights_to(ww, DEV), kv_int8=False, page=16, num_blocks=4, max_batch=1, max_seq_len=32, device=DEV)
        eng.set_inputs([11], [0], torch.zeros(1, 2, dtype=torch.int32))
        for _ in range(4):   # (at position 0 the single key makes attention blind to Q / K: look past it)
            eng.step(1)
        torch.cuda.synchronize()
        outs.append(eng.logits[:1].cpu())
    assert (outs[0] - outs[1]).abs().max() > 1e-2
    with pytest.raises(ValueError):   # norms in the weights but not in the config (or the other way round): refused
        model.DecoderEngine(replace(TOY64, qk_norm=False), model.weights_to(w, DEV), kv_int8=False, page=16, num_blocks=4, max_batch=1,
                            max_seq_len=32, device=DEV)


def test_engine_qwen3_8b_widths_w4(parity):
    cfg = replace(model.QWEN3_8B, num_layers=2, vocab=8192, max_pos=256)
    w = model.synth_model(cfg, "w4", "cpu", seed=9, zeros="centered")
    _run_engine(cfg, w, 64, parity, steps=2, prompt=2)


@pytest.mark.parametrize("B", [4, 16])
def test_engine_qwen3_0_6b_shape_fp16(B, parity):
    cfg = model.ModelConfig("qwen3-0.6b-2l", 2, 1024, 16, 8, 128, 3072, 4096, max_pos=256, qkv_bias=False, qk_norm=True)   # nh*hd = 2048 != 1024
    w = model.synth_model(cfg, "fp16", "cpu", seed=10)
    _run_engine(cfg, w, B, parity, steps=2)


# ------------------------------------------------------------------ the module graph
def test_module_graph_qwen3():
    cfg = TOY64
    w = model.synth_model(cfg, "w4", "cpu", seed=12, zeros="centered")
    wd = model.weights_to(w, DEV)
    B, page = 2, 16
    pym = model.Qwen2DecoderModel(cfg, wd, page, 64)
    ref = qwen3_ref.from_canonical(cfg, w)
    okv = oracle.OracleKV(cfg.num_layers, B, False)
    kvs = [model.LayerKVCache(*kvcache.alloc_layer_cache(8, cfg.nkv, page, cfg.hd, False, DEV), page, i) for i in range(cfg.num_layers)]
    bt = torch.arange(B * 4, dtype=torch.int32).reshape(B, 4)
    toks = torch.randint(0, cfg.vocab, (B, 4), generator=_gen(13), dtype=torch.int32)
    for step in range(4):
        ai = model.PyAttentionInputs(False, torch.full((B,), step, dtype=torch.int32), None, bt.to(DEV))
        hid = pym(toks[:, step].to(DEV), pym.prepare_fmha_impl(ai), kvs)
        _, want = ref.forward_tokens(toks[:, step], torch.full((B,), step, dtype=torch.int32), okv, list(range(B)))
        got = pym.logits(hid).cpu()
        assert torch.allclose(got, want, **TOL), (step, float((got - want).abs().max()))


# ------------------------------------------------------------------ an HF checkpoint end to end
def test_hf_qwen3_checkpoint_through_the_engine(tmp_path):
    hf = qwen3_ref.hf_tiny_model(seed=5, hidden_size=256, intermediate_size=512, num_attention_heads=8, num_key_value_heads=2,
                                 head_dim=64, vocab_size=512)
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    cfg, w = loader.load_hf_checkpoint(str(tmp_path))
    assert cfg.qk_norm and cfg.nh * cfg.hd == 512 != cfg.hidden
    B, page = 2, 16
    eng = model.DecoderEngine(cfg, model.weights_to(w, DEV), kv_int8=False, page=page, num_blocks=8, max_batch=B, max_seq_len=64, device=DEV)
    ids = torch.randint(0, 512, (B, 6), generator=_gen(14), dtype=torch.int32)
    with torch.no_grad():
        want = hf(ids.long()).logits.float()                            # [B, 6, V]
    got = eng.prefill(ids[:, :4].tolist(), torch.arange(B * 4, dtype=torch.int32).reshape(B, 4)).cpu()
    scale = float(want.abs().max())
    assert torch.allclose(got, want[:, 3], atol=2e-2 * scale, rtol=2e-2), float((got - want[:, 3]).abs().max())
    eng.set_inputs(ids[:, 4].tolist(), [4] * B, torch.arange(B * 4, dtype=torch.int32).reshape(B, 4))
    for s in (4, 5):
        eng.token_ids[:B].copy_(ids[:, s].to(DEV))
        eng.forward(B)
        torch.cuda.synchronize()
        got = eng.logits[:B].cpu()
        assert torch.allclose(got, want[:, s], atol=2e-2 * scale, rtol=2e-2), (s, float((got - want[:, s]).abs().max()))
        eng.positions[:B] += 1


# ------------------------------------------------------------------ tensor parallelism: one two-process step on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    try:
        import torch.distributed as dist
        from oracle import oracle
        from rtp_llm_amd import distributed, model
        import qwen3_ref
        torch.cuda.set_device(0)
        torch.set_num_threads(4)
        distributed.init_distributed("gloo")
        ar = distributed.CustomAllReduce(max_bytes=64 * 8192 * 2)
        cfg = model.ModelConfig("tiny-tp-qwen3", 2, 512, 8, 2, 64, 768, 1024, max_pos=256, qkv_bias=False, qk_norm=True)
        w = model.synth_model(cfg, "w4", "cpu", seed=21, zeros="centered")
        V = cfg.vocab
        layers = [model.split_layer_tp(L, cfg, world, rank) for L in w["layers"]]
        head = w["lm_head"].cols(rank * (V // world), (rank + 1) * (V // world))
        shard = {"layers": layers, "embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": head}
        B, page = 5, 16
        eng = model.DecoderEngine(cfg.per_rank(world), model.weights_to(shard, "cuda:0"), kv_int8=False, page=page, num_blocks=B * 2,
                                  max_batch=B, max_seq_len=32, device="cuda:0", tp_size=world, vocab_full=V)
        eng.attach_allreduce(ar, rank * (V // world))
        ref = qwen3_ref.from_canonical(cfg, w)
        okv = oracle.OracleKV(cfg.num_layers, B, False)
        bt = torch.arange(B * 2, dtype=torch.int32).reshape(B, 2)
        tok = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
        eng.set_inputs(tok.tolist(), [0] * B, bt)
        dist.barrier()
        eng.capture(B)
        for step in range(3):
            _, want = ref.forward_tokens(tok, torch.full((B,), step, dtype=torch.int32), okv, list(range(B)))
            eng.replay(B, 1)
            torch.cuda.synchronize()
            parts = [torch.empty(B, V // world) for _ in range(world)]
            dist.all_gather(parts, eng.logits[:B].cpu())
            full = torch.cat(parts, dim=1)
            assert torch.allclose(full, want, atol=1e-2, rtol=1e-2), (step, float((full - want).abs().max()))
            tok = oracle.greedy(want)
            eng.token_ids[:B].copy_(tok)
        assert ar.status() == 0 and eng.oob_count() == 0
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()[-2000:]))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_tp2_qwen3_step_processes_on_one_gpu():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=540) for _ in range(world)]
    except Exception as e:  # noqa: BLE001
        res = [("missing", repr(e))]
    for p in procs:
        p.join(30)
        if p.is_alive():
            p.kill()
    assert sorted(res) == [(r, "ok") for r in range(world)], res
