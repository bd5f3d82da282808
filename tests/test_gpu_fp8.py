"""FP8 e4m3 weight-only linears (128 x 128 block scales) on the MI355X: the staged decode GEMMs at every row-count class, the
numerics contract (fp32 scale on the fp32 group sums), the step driver on synthetic FP8 models and an FP8 checkpoint end to end.
The reference everywhere is W_ref = codes.view(float8_e4m3fn).double() * scale (tests/fp8_util.py) through oracle.linear /
oracle.OracleDecoder / tests/qwen3_ref.py, which take dequantised weights."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from oracle import oracle
from rtp_llm_amd import _C, loader, model, ops, quant

import fp8_util
import qwen3_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-2, rtol=1e-2)     # the project's linear tolerance (tests/test_gpu_parity.py)
MS = (1, 7, 8, 9, 16, 33, 64, 83, 160)   # persistent-kernel boundary, row blocks of the staged kernel, > 64 slabs, >= 128 route
SHAPES = ((256, 64), (384, 208), (1024, 4608))   # two groups; odd group count + ragged last column block; split-K


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _C.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


_CASES = {}


def _case(K, N):
    """One synthetic FP8 linear per shape, shared by every test that needs it: (codes, scales, fp32 W_ref, packed on the GPU, x fp32, bias fp32)."""
    if (K, N) not in _CASES:
        c = model.synth_linear(K, N, "fp8", "cpu", _gen(K + N))
        W = fp8_util.w_ref(c.q, c.scales).float()
        x = torch.randn(max(MS), K, generator=_gen(K * 3 + N)) * 0.5
        bias = torch.randn(N, generator=_gen(N)) * 0.1
        _CASES[(K, N)] = (c, W, c.pack().to(DEV), x, bias)
    return _CASES[(K, N)]


# ------------------------------------------------------------------ 1. linear parity
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,N", SHAPES)
def test_linear_parity(K, N, dtype):
    c, W, packed, x32, b32 = _case(K, N)
    for M in MS:
        x = x32[:M].to(dtype)
        for bias in (None, b32.to(dtype)):
            got = ops.linear(x.to(DEV), packed, None if bias is None else bias.to(DEV)).cpu()
            want = oracle.linear(x, W, bias)
            assert got.dtype == dtype and torch.allclose(got.float(), want.float(), **TOL), (M, bias is not None, float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("M", [5, 33])
def test_linear_silu_epilogue(M):
    K, N = 1024, 4608
    c, W, _, x32, _ = _case(K, N)
    packed = c.pack(gate_up=True).to(DEV)
    x = x32[:M].half()
    got = ops.linear(x.to(DEV), packed, None, epilogue=_C.EPI_SILU_MUL).cpu()
    want = oracle.silu_mul(oracle.linear(x, W))
    assert got.shape == (M, N // 2) and torch.allclose(got.float(), want.float(), **TOL), float((got.float() - want.float()).abs().max())


@pytest.mark.parametrize("M", [4, 40])
def test_linear_partial_and_fold(M):
    """The split-K entry the step driver uses: fp32 slabs, folded by the consumer (here: add + RMSNorm)."""
    K, N = 1024, 4608
    c, W, packed, x32, _ = _case(K, N)
    x = x32[:M].half()
    slabs = torch.empty(16, M, packed.N_pad, dtype=torch.float32, device=DEV)
    ws = ops.weight_struct(packed)
    xd = x.to(DEV)                                           # device tensors stay referenced while their pointers are in use
    ns = _C.lib().mi355_linear_partial(xd.data_ptr(), M, C.byref(ws), slabs.data_ptr(), 16, torch.cuda.current_stream().cuda_stream)
    assert ns > 1, (ns, _C.lib().mi355_last_error())
    ref32 = oracle.linear(x, W, out_f32=True)
    assert torch.allclose(slabs[:ns].sum(0)[:, :N].cpu(), ref32, atol=5e-3, rtol=2e-3)
    res = (torch.randn(M, N, generator=_gen(M)) * 0.5).half()
    nw = (1 + 0.1 * torch.randn(N, generator=_gen(M + 1))).half()
    y, h = torch.empty(M, N, dtype=torch.float16, device=DEV), torch.empty(M, N, dtype=torch.float16, device=DEV)
    resd, nwd = res.to(DEV), nw.to(DEV)
    _C.check(_C.lib().mi355_add_rmsnorm(None, slabs.data_ptr(), ns, packed.N_pad, None, resd.data_ptr(), h.data_ptr(), nwd.data_ptr(),
                                        1e-6, M, N, y.data_ptr(), torch.cuda.current_stream().cuda_stream), "add_rmsnorm")
    h_ref = (ref32 + res.float()).half()                     # residual_out = fp16(sum of the slabs + residual)
    assert torch.allclose(h.cpu().float(), h_ref.float(), **TOL)
    assert torch.allclose(y.cpu().float(), oracle.rmsnorm(h_ref, nw, 1e-6).float(), **TOL)


def test_strategy_and_native_object():
    K, N = 384, 208
    c, W, packed, x32, b32 = _case(K, N)
    from rtp_llm_amd.linear import LinearFactory, Mi355Fp8Linear
    lin = LinearFactory.create_linear(c.q.view(torch.float8_e4m3fn).to(DEV), b32.half().to(DEV), c.scales.to(DEV))
    assert isinstance(lin, Mi355Fp8Linear)
    x = x32[:9].half()
    want = oracle.linear(x, W, b32.half())
    assert torch.allclose(lin(x.to(DEV)).cpu().float(), want.float(), **TOL)
    from rtp_llm_amd import native_ops
    nops = native_ops.load()
    nl = nops.Mi355WeightOnlyLinear(packed.qweight, packed.meta, packed.wbits, packed.K, packed.N, packed.K_pad, packed.N_pad, packed.group_size,
                                    b32.half().to(DEV), packed.wkind)
    assert torch.allclose(nl.forward(x.to(DEV), 0).cpu().float(), want.float(), **TOL)


# ------------------------------------------------------------------ 2. the numerics contract
def _contract_case(M, K, N, seed):
    g = _gen(seed)
    codes = torch.randint(0, 256, (K, N), generator=g, dtype=torch.uint8)
    codes = torch.where((codes & 0x7F) == 0x7F, codes & 0xF8, codes)                 # NaN codes replaced
    KB, NB = (K + 127) // 128, (N + 127) // 128
    u = torch.rand(KB, NB, generator=g, dtype=torch.float64) * 19 + 3                # U(3, 22)
    v = torch.rand(KB, NB, generator=g, dtype=torch.float64)
    bs = (torch.exp2(-u) * (1 + v)).float()                                          # mostly subnormal or inexact in fp16
    scales = quant.expand_fp8_block_scales(bs, N)
    x = torch.randn(M, K, generator=g).half()
    return codes, scales, x


@pytest.mark.parametrize("M,K,N", [(7, 384, 208), (64, 1024, 512)])
def test_contract_fp32_scale_on_fp32_group_sums(M, K, N):
    """Pins what TOL cannot see: the fp32 scale multiplies the fp32 partial sum of its 128-row group (include/mi355_decode.h,
    "FP8 weights"), never an fp16 image of the scale or of scale * w.  Block scales 2^-u (1 + v), u ~ U(3, 22), v ~ U(0, 1): most are
    subnormal or inexact in fp16.  Metric per column: max over rows |y - ref| / max over rows |ref|, ref in fp64.
    Modelled on the CPU for both shapes: the contract's arithmetic (fp32 group sums times fp32 scale) gives 5e-7, a scale rounded to
    fp16 gives 4e-4.  Bound 1e-5: 20 x over the reference model (room for another summation order and the split-K fold), 40 x under the
    failure it exists to catch."""
    codes, scales, x = _contract_case(M, K, N, 100 + M)
    assert float((scales.half().float() != scales).float().mean()) > 0.5            # the inputs do exercise the contract
    packed = quant.pack_fp8_block(codes, scales).to(DEV)
    got = ops.linear(x.to(DEV), packed, None, epilogue=_C.EPI_OUT_F32).cpu().double()
    ref = x.double() @ fp8_util.w_ref(codes, scales)
    err = (got - ref).abs().amax(dim=0) / ref.abs().amax(dim=0)
    print(f"contract M={M} K={K} N={N}: max per-column error {float(err.max()):.3e}")
    # the failure model on the same inputs, for the record: the scale rounded to fp16
    bad = x.double() @ fp8_util.w_ref(codes, scales.half().float())
    print(f"  (fp16-rounded scale would give {float(((bad - ref).abs().amax(dim=0) / ref.abs().amax(dim=0)).max()):.3e})")
    assert float(err.max()) < 1e-5, float(err.max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M", [7, 20])
def test_contract_on_the_step_kernels(M, dtype):
    """The same contract, metric and bound (1e-5; see test_contract_fp32_scale_on_fp32_group_sums) on the launches the captured step
    runs at b <= 32: mi355_linear_partial -- the one- and two-row-block instances of the staged kernel, fp16 and bf16 activations --
    with its fp32 slabs summed on the host."""
    K, N = 384, 208
    codes, scales, x = _contract_case(M, K, N, 200 + M)
    x = x.to(dtype)
    packed = quant.pack_fp8_block(codes, scales).to(DEV)
    slabs = torch.zeros(16, M, packed.N_pad, dtype=torch.float32, device=DEV)
    ws, xd = ops.weight_struct(packed, dtype), x.to(DEV)
    ns = _C.lib().mi355_linear_partial(xd.data_ptr(), M, C.byref(ws), slabs.data_ptr(), 16, torch.cuda.current_stream().cuda_stream)
    assert ns >= 1, (ns, _C.lib().mi355_last_error())
    torch.cuda.synchronize()
    got = slabs[:ns].cpu().double().sum(0)[:, :N]
    ref = x.double() @ fp8_util.w_ref(codes, scales)
    err = (got - ref).abs().amax(dim=0) / ref.abs().amax(dim=0)
    print(f"contract (partial) M={M} {dtype} ns={ns}: max per-column error {float(err.max()):.3e}")
    assert float(err.max()) < 1e-5, float(err.max())


# ------------------------------------------------------------------ 3. the step driver
TOY64 = model.ModelConfig("toy-qwen3-hd64-fp8", 2, 512, 8, 2, 64, 1024, 2048, max_pos=256, qkv_bias=False, qk_norm=True)
TOYQ2 = model.ModelConfig("toy-qwen2-fp8", 2, 512, 8, 2, 64, 1024, 2048, max_pos=256, qkv_bias=True)


def _reference(cfg, w, dtype=torch.float16):
    wd = fp8_util.dense_canonical(w)
    if cfg.qk_norm:
        return qwen3_ref.from_canonical(cfg, wd)
    cast = (lambda t: t) if dtype == torch.float16 else (lambda t: None if t is None else t.to(dtype))
    ow = {"embedding": cast(wd["embedding"]), "final_norm": cast(wd["final_norm"]), "lm_head": wd["lm_head"].w.float(),
          "layers": [{"input_norm": cast(L["input_norm"]), "post_norm": cast(L["post_norm"]), "qkv_bias": cast(L["qkv_bias"]),
                      **{k: L[k].w.float() for k in ("qkv", "o", "gate_up", "down")}} for L in wd["layers"]]}
    return oracle.OracleDecoder({**cfg.__dict__}, ow)


def _to_dtype(w, dtype):
    """The canonical dict as the loader gives it for bf16 activations: 16-bit tensors in bf16, FP8 codes / fp32 scales untouched."""
    if dtype == torch.float16:
        return w
    def conv(v):
        if torch.is_tensor(v):
            return v.to(dtype) if v.dtype == torch.float16 else v
        if isinstance(v, model.CanonLinear):
            return model.CanonLinear("fp16", v.K, v.N, w=v.w.to(dtype)) if v.kind == "fp16" else v
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, list):
            return [conv(x) for x in v]
        return v
    return conv(w)


def _run_engine(cfg, w, B, parity, *, steps=3, prompt=3, kv_int8=False, tol=1e-2, dtype=torch.float16, seed=0):
    """Prefill of B prompts, then `steps` graph-replayed decode steps, against the reference (ids on safe rows, logits `tol`)."""
    page = 16
    nb = (prompt + steps + 4 + page - 1) // page + 1
    w = _to_dtype(w, dtype)
    eng = model.DecoderEngine(cfg, model.weights_to(w, DEV), kv_int8=kv_int8, page=page, num_blocks=B * nb, max_batch=B,
                              max_seq_len=nb * page, device=DEV, **({} if dtype == torch.float16 else {"dtype": dtype}))
    ref = _reference(cfg, w, dtype)
    okv = oracle.OracleKV(cfg.num_layers, B, kv_int8)
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)
    prompts = torch.randint(0, cfg.vocab, (B, prompt), generator=_gen(seed), dtype=torch.int32)
    got = eng.prefill(prompts.tolist(), bt).cpu()
    toks = prompts.t().reshape(-1)
    pos = torch.arange(prompt, dtype=torch.int32).repeat_interleave(B)
    _, ref_all = ref.forward_tokens(toks, pos, okv, list(range(B)) * prompt)
    want = ref_all[-B:]
    assert torch.allclose(got, want, atol=tol, rtol=tol), ("prefill", float((got - want).abs().max()))
    parity.step(got_ids=got.argmax(-1).int(), ref_ids=oracle.greedy(want), ref_logits=want, got_logits=got, tol=tol, label="prefill")
    tok = oracle.greedy(want)
    eng.set_inputs(tok.tolist(), [prompt] * B, bt)
    eng.capture(B)
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
    assert eng.oob_count() == 0
    return eng


_MODELS = {}


def _model(cfg, seed):
    if (cfg.name, seed) not in _MODELS:
        _MODELS[(cfg.name, seed)] = model.synth_model(cfg, "fp8", "cpu", seed=seed)
    return _MODELS[(cfg.name, seed)]


@pytest.mark.parametrize("kv_int8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("B", [1, 8])
def test_engine_qwen3_toy_fp8(B, kv_int8, parity):
    _run_engine(TOY64, _model(TOY64, 7), B, parity, kv_int8=kv_int8, tol=3e-2 if kv_int8 else 1e-2)


def test_engine_qwen2_bias_b33_crosses_the_row_block_steps(parity):
    """33 rows: past fuse_rows and through the 16 / 32 / 64-row instances of the staged chain, which the planner falls back to for a
    format no image launcher takes; prefill of 99 tokens goes through the > 64-row slabs."""
    _run_engine(TOYQ2, _model(TOYQ2, 8), 33, parity, steps=2)


def test_engine_bf16(parity):
    _run_engine(TOY64, _model(TOY64, 7), 8, parity, dtype=torch.bfloat16, tol=3e-2)


def test_fp8_checkpoint_through_the_engine(tmp_path):
    """The toy model written as an FP8 checkpoint and loaded back gives the logits of the engine built from the canonical weights."""
    w = _model(TOY64, 7)
    fp8_util.write_fp8_ckpt(str(tmp_path), TOY64, w)
    cfg, lw = loader.load_hf_checkpoint(str(tmp_path))
    assert cfg.qk_norm and lw["layers"][0]["qkv"].kind == "fp8"
    B, page = 2, 16
    ids = torch.randint(0, TOY64.vocab, (B, 6), generator=_gen(14), dtype=torch.int32)
    bt = torch.arange(B * 4, dtype=torch.int32).reshape(B, 4)
    outs = []
    for c, ww in ((TOY64, w), (cfg, lw)):
        eng = model.DecoderEngine(c, model.weights_to(ww, DEV), kv_int8=False, page=page, num_blocks=8, max_batch=B, max_seq_len=64, device=DEV)
        seq = [eng.prefill(ids[:, :4].tolist(), bt).cpu()]
        eng.set_inputs(ids[:, 4].tolist(), [4] * B, bt)
        for s in (4, 5):
            eng.token_ids[:B].copy_(ids[:, s].to(DEV))
            eng.forward(B)
            torch.cuda.synchronize()
            seq.append(eng.logits[:B].cpu().clone())
            eng.positions[:B] += 1
        outs.append(torch.stack(seq))
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    ref = _reference(TOY64, w)
    okv = oracle.OracleKV(TOY64.num_layers, B, False)
    _, r = ref.forward_tokens(ids[:, :4].t().reshape(-1), torch.arange(4, dtype=torch.int32).repeat_interleave(B), okv, list(range(B)) * 4)
    assert torch.allclose(outs[1][0], r[-B:], **TOL)


# ------------------------------------------------------------------ 4. tensor parallelism: one two-process step on one GPU
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
        import fp8_util
        import qwen3_ref
        torch.cuda.set_device(0)
        torch.set_num_threads(4)
        distributed.init_distributed("gloo")
        ar = distributed.CustomAllReduce(max_bytes=64 * 8192 * 2)
        cfg = model.ModelConfig("tiny-tp-qwen3-fp8", 2, 512, 8, 2, 64, 768, 1024, max_pos=256, qkv_bias=False, qk_norm=True)
        w = model.synth_model(cfg, "fp8", "cpu", seed=21)
        V = cfg.vocab
        layers = [model.split_layer_tp(L, cfg, world, rank) for L in w["layers"]]
        head = w["lm_head"].cols(rank * (V // world), (rank + 1) * (V // world))
        shard = {"layers": layers, "embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": head}
        B, page = 5, 16
        eng = model.DecoderEngine(cfg.per_rank(world), model.weights_to(shard, "cuda:0"), kv_int8=False, page=page, num_blocks=B * 2,
                                  max_batch=B, max_seq_len=32, device="cuda:0", tp_size=world, vocab_full=V)
        eng.attach_allreduce(ar, rank * (V // world))
        ref = qwen3_ref.from_canonical(cfg, fp8_util.dense_canonical(w))
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
def test_tp2_fp8_step_processes_on_one_gpu():
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
