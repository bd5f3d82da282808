"""MXFP4 weight-only linears (e2m1 codes, e8m0 scale per 32 rows) on the MI355X: the exact decode of every code at every nibble
position under every admitted scale (which pins the nibble order of the image and the scale handling), the accumulation
contract, the staged decode GEMMs at every row-count class, the step driver on synthetic MXFP4 models and a Quark-form checkpoint
end to end.  The reference everywhere is W_ref = E2M1_VALUES[code].double() * 2.0 ** (byte - 127) (tests/mxfp4_util.py) through
oracle.linear / oracle.OracleDecoder / tests/qwen3_ref.py, which take dequantised weights."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from oracle import oracle
from rtp_llm_amd import _C, loader, model, ops, quant

import mxfp4_util
import qwen3_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-2, rtol=1e-2)     # the project's linear tolerance (tests/test_gpu_parity.py)
MS = (1, 3, 8, 9, 16, 17, 33, 64, 130)   # persistent-kernel boundary, the 1 / 2 / 4 row-block instances, > 64 slabs, the >= 128 route
SHAPES = ((160, 48), (384, 208), (1024, 512))   # ragged last chunk; odd chunk count + ragged last column block; split-K


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _C.lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ 1. exact decode
def _decode_case():
    """K = 256, N = 48: codes (7 n + 3 k + k // 32) % 16 and scale bytes 114 + (48 g + n) % 27."""
    K, N = 256, 48
    k, n = torch.arange(K).reshape(K, 1), torch.arange(N).reshape(1, N)
    codes = ((7 * n + 3 * k + k // 32) % 16).to(torch.uint8)
    g = torch.arange(K // 32).reshape(K // 32, 1)
    sb = (114 + (48 * g + n) % 27).to(torch.uint8)
    # coverage, checked here on the host: all 16 patterns at every nibble position e, every q and every k-step s ...
    for s in range(4):
        for q in range(4):
            for e in range(8):
                rows = [128 * c + 32 * s + 8 * q + e for c in range(2)]
                assert set(codes[rows].reshape(-1).tolist()) == set(range(16)), (s, q, e)
    # ... every admitted scale byte, and every byte position of the meta dword sees the two ends of the range
    assert set(sb.reshape(-1).tolist()) == set(range(114, 141))
    for s in range(4):
        assert {114, 140} <= set(sb[s::4].reshape(-1).tolist()), s
    return codes, sb


def _as_output(W, rows, dtype):
    """Rows of W_ref in the activation dtype as a GEMM returns them: bit for bit, except that the code 8 (-0.0) comes back as +0.0 --
    y is a sum over K of products, all but one of them zeros of either sign, on a +0.0 accumulator, and (+0) + (-0) = +0 in round
    to nearest.  Adding +0.0 maps -0.0 to +0.0 and leaves every other value as it is."""
    return W[rows].to(dtype) + torch.zeros((), dtype=dtype)


_DECODE = {}


def _decode_packed():
    if not _DECODE:
        codes, sb = _decode_case()
        packed, flushed = quant.pack_mxfp4(codes, sb)
        assert flushed == (0, 0)
        _DECODE["v"] = (codes, sb, mxfp4_util.w_ref(codes, sb), packed.to(DEV))
    return _DECODE["v"]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_exact_decode_every_code_position_and_scale(dtype):
    """x = the 256 one-hot rows (M = 256: 64-row slabs of the four-row-block instances), so y[k] is row k of W as the kernel decoded
    it: bit-equal to W_ref in the activation dtype.  A swapped nibble order, a wrong byte of the meta dword or a scale applied
    anywhere but as the exact power of two all show here."""
    codes, sb, W, packed = _decode_packed()
    want = _as_output(W, slice(None), dtype)
    assert torch.equal(want.double(), W)                       # the contract: every operand is exact in the activation dtype (-0 == +0 here)
    assert int((want.view(torch.int16) == 0).sum()) == 2 * 256 * 48 // 16   # codes 0 and 8: the +0.0 pattern
    x = torch.eye(256, dtype=dtype)
    got = ops.linear(x.to(DEV), packed, None).cpu()
    assert got.dtype == dtype
    bad = (got.view(torch.int16) != want.view(torch.int16))
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())


ROWS8 = (0, 41, 82, 123, 132, 173, 214, 255)                  # every k-step s and every q once per chunk, e = 0 .. 7


@pytest.mark.parametrize("hint", [0, _C.HINT_NO_PERSISTENT], ids=["persistent", "staged"])
def test_exact_decode_m8(hint):
    """The same on 8 chosen rows: M = 8 fp16 runs on the persistent kernel, with the hint on the one-row-block staged instance."""
    codes, sb, W, packed = _decode_packed()
    assert {(r % 128) // 32 for r in ROWS8} == {0, 1, 2, 3} and {(r % 32) // 8 for r in ROWS8} == {0, 1, 2, 3} and {r % 8 for r in ROWS8} == set(range(8))
    x = torch.zeros(8, 256, dtype=torch.float16)
    x[torch.arange(8), torch.tensor(ROWS8)] = 1.0
    got = ops.linear(x.to(DEV), packed, None, epilogue=hint).cpu()
    want = _as_output(W, list(ROWS8), torch.float16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (got.float() - want.float()).abs().max()


def test_exact_decode_m24_bf16_and_fp16():
    """24 one-hot rows: the two-row-block instance of the staged kernel, both activation dtypes."""
    codes, sb, W, packed = _decode_packed()
    rows = torch.arange(24) * 11 % 256
    for dtype in (torch.float16, torch.bfloat16):
        x = torch.zeros(24, 256, dtype=dtype)
        x[torch.arange(24), rows] = 1.0
        got = ops.linear(x.to(DEV), packed, None).cpu()
        want = _as_output(W, rows, dtype)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), dtype


# ------------------------------------------------------------------ 2. the accumulation contract
def _contract_case(M, K, N, dtype, seed):
    g = _gen(seed)
    codes = torch.randint(0, 16, (K, N), generator=g, dtype=torch.uint8)
    sb = torch.randint(114, 141, (K // 32, N), generator=g, dtype=torch.uint8)
    x = torch.randn(M, K, generator=g).to(dtype)
    packed, flushed = quant.pack_mxfp4(codes, sb)
    assert flushed == (0, 0)
    W = mxfp4_util.w_ref(codes, sb)
    return x, W, packed.to(DEV), K * 2.0 ** -23 * (x.double().abs() @ W.abs())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,K,N", [(7, 384, 208), (64, 1024, 512)])
def test_contract_exact_products_fp32_accumulation(M, K, N, dtype):
    """fp32 output: |y - x @ W_ref| <= K 2^-23 (|x| @ |W_ref|) elementwise.  The operands 2^E e2m1 and the products with a 16-bit x
    are exact, so the only error is that of summing K terms in fp32: the standard bound (K - 1) u sum |terms|, u = 2^-24, here with a
    factor-2 margin; it holds for any accumulation order, split-K folds included.
    Measured on the MI355X: max error / bound = 2.1e-3 and 3.4e-3 (M = 7, fp16 / bf16), 1.7e-3 and 1.8e-3 (M = 64)."""
    x, W, packed, bound = _contract_case(M, K, N, dtype, 100 + M)
    got = ops.linear(x.to(DEV), packed, None, epilogue=_C.EPI_OUT_F32).cpu().double()
    err = (got - x.double() @ W).abs()
    print(f"contract M={M} K={K} N={N} {dtype}: max err / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,K,N", [(7, 384, 208), (64, 1024, 512)])
def test_contract_on_linear_partial(M, K, N, dtype):
    """The same bound on the split-K entry of the step driver: the fp32 slabs of mi355_linear_partial summed on the host in fp64.
    Measured: max error / bound = 4.4e-3 and 3.7e-3 (M = 7, one slab), 1.2e-3 and 1.1e-3 (M = 64, four slabs)."""
    x, W, packed, bound = _contract_case(M, K, N, dtype, 200 + M)
    slabs = torch.zeros(16, M, packed.N_pad, dtype=torch.float32, device=DEV)
    ws, xd = ops.weight_struct(packed, dtype), x.to(DEV)
    ns = _C.lib().mi355_linear_partial(xd.data_ptr(), M, C.byref(ws), slabs.data_ptr(), 16, torch.cuda.current_stream().cuda_stream)
    assert ns >= 1, (ns, _C.lib().mi355_last_error())
    torch.cuda.synchronize()
    got = slabs[:ns].cpu().double().sum(0)[:, :N]
    err = (got - x.double() @ W).abs()
    print(f"contract (partial) M={M} K={K} N={N} {dtype} ns={ns}: max err / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((slabs[:ns, :, N:] == 0).all())               # padding columns: code 0


# ------------------------------------------------------------------ 3. linear parity
_CASES = {}


def _case(K, N):
    """One synthetic MXFP4 linear per shape, shared by every test that needs it: (canonical, fp32 W_ref, packed on the GPU, x fp32, bias fp32)."""
    if (K, N) not in _CASES:
        c = model.synth_linear(K, N, "mxfp4", "cpu", _gen(K + N))
        W = mxfp4_util.w_ref(c.q, c.scales).float()
        x = torch.randn(max(MS), K, generator=_gen(K * 3 + N)) * 0.5
        bias = torch.randn(N, generator=_gen(N)) * 0.1
        _CASES[(K, N)] = (c, W, c.pack().to(DEV), x, bias)
    return _CASES[(K, N)]


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
    K, N = 1024, 512
    c, W, _, x32, _ = _case(K, N)
    packed = c.pack(gate_up=True).to(DEV)
    x = x32[:M].half()
    got = ops.linear(x.to(DEV), packed, None, epilogue=_C.EPI_SILU_MUL).cpu()
    want = oracle.silu_mul(oracle.linear(x, W))
    assert got.shape == (M, N // 2) and torch.allclose(got.float(), want.float(), **TOL), float((got.float() - want.float()).abs().max())


@pytest.mark.parametrize("M", [4, 40])
def test_linear_partial_and_fold(M):
    """The split-K entry the step driver uses: fp32 slabs, folded by the consumer (here: add + RMSNorm)."""
    K, N = 1024, 512
    c, W, packed, x32, _ = _case(K, N)
    x = x32[:M].half()
    slabs = torch.zeros(16, M, packed.N_pad, dtype=torch.float32, device=DEV)
    ws = ops.weight_struct(packed)
    xd = x.to(DEV)                                           # device tensors stay referenced while their pointers are in use
    ns = _C.lib().mi355_linear_partial(xd.data_ptr(), M, C.byref(ws), slabs.data_ptr(), 16, torch.cuda.current_stream().cuda_stream)
    assert ns >= 1, (ns, _C.lib().mi355_last_error())
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
    from rtp_llm_amd.linear import LinearFactory, Mi355Mxfp4Linear
    w8, s8 = mxfp4_util.to_quark(c)
    lin = LinearFactory.create_linear(w8.to(DEV), b32.half().to(DEV), s8.to(DEV))
    assert isinstance(lin, Mi355Mxfp4Linear) and lin.packed.wkind == 2
    x = x32[:9].half()
    want = oracle.linear(x, W, b32.half())
    assert torch.allclose(lin(x.to(DEV)).cpu().float(), want.float(), **TOL)
    from rtp_llm_amd import native_ops
    nops = native_ops.load()
    nl = nops.Mi355WeightOnlyLinear(packed.qweight, packed.meta, packed.wbits, packed.K, packed.N, packed.K_pad, packed.N_pad, packed.group_size,
                                    b32.half().to(DEV), packed.wkind)
    assert torch.allclose(nl.forward(x.to(DEV), 0).cpu().float(), want.float(), **TOL)


# ------------------------------------------------------------------ 3. the step driver
TOY64 = model.ModelConfig("toy-qwen3-hd64-mxfp4", 2, 512, 8, 2, 64, 1024, 2048, max_pos=256, qkv_bias=False, qk_norm=True)
TOYQ2 = model.ModelConfig("toy-qwen2-mxfp4", 2, 512, 8, 2, 64, 1024, 2048, max_pos=256, qkv_bias=True)


def _reference(cfg, w, dtype=torch.float16):
    wd = mxfp4_util.dense_canonical(w)
    if cfg.qk_norm:
        return qwen3_ref.from_canonical(cfg, wd)
    cast = (lambda t: t) if dtype == torch.float16 else (lambda t: None if t is None else t.to(dtype))
    ow = {"embedding": cast(wd["embedding"]), "final_norm": cast(wd["final_norm"]), "lm_head": wd["lm_head"].w.float(),
          "layers": [{"input_norm": cast(L["input_norm"]), "post_norm": cast(L["post_norm"]), "qkv_bias": cast(L["qkv_bias"]),
                      **{k: L[k].w.float() for k in ("qkv", "o", "gate_up", "down")}} for L in wd["layers"]]}
    return oracle.OracleDecoder({**cfg.__dict__}, ow)


def _to_dtype(w, dtype):
    """The canonical dict as the loader gives it for bf16 activations: 16-bit tensors in bf16, MXFP4 codes / scale bytes untouched."""
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


def _reference_trace(cfg, w, B, *, steps=3, prompt=3, kv_int8=False, tol=1e-2, dtype=torch.float16, seed=0):
    """The reference alone, on the host: (prompts, [logits after the prefill, after decode step 0, ...]) along its own greedy tokens.
    Greedy ids are required only on rows whose reference top-2 margin exceeds `tol`; the seeds of this file are chosen so that this
    exempts at most a quarter of the rows of every step, which is asserted here, from the reference and nothing else."""
    ref = _reference(cfg, _to_dtype(w, dtype), dtype)
    okv = oracle.OracleKV(cfg.num_layers, B, kv_int8)
    prompts = torch.randint(0, cfg.vocab, (B, prompt), generator=_gen(seed), dtype=torch.int32)
    _, ref_all = ref.forward_tokens(prompts.t().reshape(-1), torch.arange(prompt, dtype=torch.int32).repeat_interleave(B), okv, list(range(B)) * prompt)
    wants = [ref_all[-B:]]
    for s in range(steps):
        _, want = ref.forward_tokens(oracle.greedy(wants[-1]), torch.full((B,), prompt + s, dtype=torch.int32), okv, list(range(B)))
        wants.append(want)
    for i, want in enumerate(wants):
        top2 = want.float().topk(2, dim=-1).values
        safe = int(((top2[:, 0] - top2[:, 1]) > tol).sum())
        assert 4 * safe >= 3 * B, (i, safe, B)
    return prompts, wants


def _run_engine(cfg, w, B, parity, *, steps=3, prompt=3, kv_int8=False, tol=1e-2, dtype=torch.float16, seed=0):
    """Prefill of B prompts, then `steps` graph-replayed decode steps, against the reference (ids on safe rows, logits `tol`)."""
    page = 16
    nb = (prompt + steps + 4 + page - 1) // page + 1
    prompts, wants = _reference_trace(cfg, w, B, steps=steps, prompt=prompt, kv_int8=kv_int8, tol=tol, dtype=dtype, seed=seed)
    w = _to_dtype(w, dtype)
    eng = model.DecoderEngine(cfg, model.weights_to(w, DEV), kv_int8=kv_int8, page=page, num_blocks=B * nb, max_batch=B,
                              max_seq_len=nb * page, device=DEV, **({} if dtype == torch.float16 else {"dtype": dtype}))
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)
    got = eng.prefill(prompts.tolist(), bt).cpu()
    want = wants[0]
    assert torch.allclose(got, want, atol=tol, rtol=tol), ("prefill", float((got - want).abs().max()))
    parity.step(got_ids=got.argmax(-1).int(), ref_ids=oracle.greedy(want), ref_logits=want, got_logits=got, tol=tol, label="prefill")
    tok = oracle.greedy(want)
    eng.set_inputs(tok.tolist(), [prompt] * B, bt)
    eng.capture(B)
    for s in range(steps):
        want = wants[s + 1]
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
        _MODELS[(cfg.name, seed)] = model.synth_model(cfg, "mxfp4", "cpu", seed=seed)
    return _MODELS[(cfg.name, seed)]


@pytest.mark.parametrize("kv_int8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("B", [1, 8])
def test_engine_qwen3_toy_mxfp4(B, kv_int8, parity):
    _run_engine(TOY64, _model(TOY64, 7), B, parity, kv_int8=kv_int8, tol=3e-2 if kv_int8 else 1e-2)


def test_engine_qwen2_bias_b33_crosses_the_row_block_steps(parity):
    """33 rows: past fuse_rows and through the 16 / 32 / 64-row instances of the staged chain, which the planner falls back to for a
    format no image launcher takes; prefill of 99 tokens goes through the > 64-row slabs."""
    _run_engine(TOYQ2, _model(TOYQ2, 8), 33, parity, steps=2)


def test_engine_bf16(parity):
    _run_engine(TOY64, _model(TOY64, 7), 8, parity, dtype=torch.bfloat16, tol=3e-2, seed=2)   # prompt seed: see _reference_trace


def test_sampling_and_logprobs_in_the_captured_step():
    """The sampling tail and the log-probability record behind MXFP4 linears: top_k = 1 sampling inside the captured graph gives the
    greedy tokens of the same engine, and each recorded token log-probability is the reference's log-softmax at that token within
    2 x the logits tolerance (|d logit| + |d logsumexp|)."""
    w = _model(TOY64, 7)
    B, N, page = 4, 3, 16
    prompts = torch.randint(0, TOY64.vocab, (B, 3), generator=_gen(31), dtype=torch.int32).tolist()
    bt = torch.arange(B * 2, dtype=torch.int32).reshape(B, 2)
    mk = lambda: model.DecoderEngine(TOY64, model.weights_to(w, DEV), kv_int8=False, page=page, num_blocks=B * 2, max_batch=B, max_seq_len=32, device=DEV)
    greedy = mk().generate(prompts, bt, N)
    toks, rec = mk().generate_sampled_graph(prompts, bt, N, seeds=list(range(B)), top_logprobs=2, top_k=1, temperature=1.0)
    assert toks == greedy
    ref = _reference(TOY64, w)
    okv = oracle.OracleKV(TOY64.num_layers, B, False)
    pt = torch.tensor(prompts, dtype=torch.int32)
    _, ref_all = ref.forward_tokens(pt.t().reshape(-1), torch.arange(3, dtype=torch.int32).repeat_interleave(B), okv, list(range(B)) * 3)
    want = ref_all[-B:]
    tk = torch.tensor(toks)
    for s in range(N):
        lp = torch.log_softmax(want.double(), dim=-1).gather(1, tk[:, s: s + 1].long())[:, 0]
        assert torch.allclose(rec["token_logprobs"][:, s].cpu().double(), lp, atol=2e-2, rtol=0), (s, float((rec["token_logprobs"][:, s].cpu().double() - lp).abs().max()))
        if s + 1 < N:
            _, want = ref.forward_tokens(tk[:, s].int(), torch.full((B,), 3 + s, dtype=torch.int32), okv, list(range(B)))


def test_mxfp4_checkpoint_through_the_engine(tmp_path):
    """The toy model written as an MXFP4 checkpoint and loaded back gives the logits of the engine built from the canonical weights."""
    w = _model(TOY64, 7)
    mxfp4_util.write_mxfp4_ckpt(str(tmp_path), TOY64, w)
    cfg, lw = loader.load_hf_checkpoint(str(tmp_path))
    assert cfg.qk_norm and lw["layers"][0]["qkv"].kind == "mxfp4"
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
        import mxfp4_util
        import qwen3_ref
        torch.cuda.set_device(0)
        torch.set_num_threads(4)
        distributed.init_distributed("gloo")
        ar = distributed.CustomAllReduce(max_bytes=64 * 8192 * 2)
        cfg = model.ModelConfig("tiny-tp-qwen3-mxfp4", 2, 512, 8, 2, 64, 768, 1024, max_pos=256, qkv_bias=False, qk_norm=True)
        w = model.synth_model(cfg, "mxfp4", "cpu", seed=21)
        V = cfg.vocab
        layers = [model.split_layer_tp(L, cfg, world, rank) for L in w["layers"]]
        head = w["lm_head"].cols(rank * (V // world), (rank + 1) * (V // world))
        shard = {"layers": layers, "embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": head}
        B, page = 5, 16
        eng = model.DecoderEngine(cfg.per_rank(world), model.weights_to(shard, "cuda:0"), kv_int8=False, page=page, num_blocks=B * 2,
                                  max_batch=B, max_seq_len=32, device="cuda:0", tp_size=world, vocab_full=V)
        eng.attach_allreduce(ar, rank * (V // world))
        ref = qwen3_ref.from_canonical(cfg, mxfp4_util.dense_canonical(w))
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
def test_tp2_mxfp4_step_processes_on_one_gpu():
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
