"""Log-probabilities inside the step driver (mi355_decoder_set_logprobs): the two launches behind the greedy and the sampled tail, the
per-slot recorder in eager steps and in the captured graph, on the tiny model and the prompts of tests/test_gpu_sampled_step.py."""
import numpy as np
import pytest
import torch

from rtp_llm_amd import _C, model, ops
from tests import logprob_ref as lr
from tests import sample_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = model.ModelConfig("tiny-sampler", 2, 512, 8, 2, 64, 1024, 2048, max_pos=512)
PROMPTS = [[5, 9, 2, 7], [11, 3], [8, 8, 8, 1, 4, 6]]
BT = torch.arange(3 * 8, dtype=torch.int32).reshape(3, 8)
B, N, TOP = 3, 10, 5
SEEDS = [0x9E3779B97F4A7C15, 12345, 0xFFFFFFFF00000001]
PARAMS = dict(top_k=[1, 0, 20], top_p=[0.9, 0.8, 0.95], temperature=[1.3, 0.7, 1.0])     # row 0: a greedy row under a sampling config
KEYS = ("token_logprobs", "top_ids", "top_logprobs", "cum_log_probs", "count")


@pytest.fixture(scope="module")
def weights():
    return model.synth_model(CFG, "w4", DEV, seed=3)


def _mk(w, **kw):
    return model.DecoderEngine(CFG, w, kv_int8=False, page=16, num_blocks=64, max_batch=8, max_seq_len=128, device=DEV, **kw)


def _seeds():
    return sr.seeds_as_int64(SEEDS)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _fp32_running_sum(cols):
    """cols [B, T] fp32 -> the fp32 sum in column order, one add per step."""
    acc = np.zeros(cols.shape[0], dtype=np.float32)
    for c in range(cols.shape[1]):
        acc = (acc + cols[:, c].numpy().astype(np.float32)).astype(np.float32)
    return torch.from_numpy(acc)


@pytest.fixture(scope="module")
def graph_run(weights):
    """One sampled run through the graph with log-probabilities on, shared: (engine, tokens, read-back)."""
    eng = _mk(weights)
    toks, rec = eng.generate_sampled_graph(PROMPTS, BT, N, seeds=_seeds(), top_logprobs=TOP, **PARAMS)
    return eng, toks, rec


def test_tokens_are_the_same_with_logprobs_on(weights, graph_run):
    greedy = _mk(weights).generate(PROMPTS, BT, N)
    eng = _mk(weights)
    eng.set_logprobs(TOP, N)
    assert eng.generate(PROMPTS, BT, N) == greedy
    torch.cuda.synchronize()
    lp = eng.logprobs
    assert lp["count"][:B].tolist() == [N] * B
    tok = torch.tensor(greedy, device=DEV, dtype=torch.int32)
    assert torch.equal(lp["top_ids"][:B, :N, 0], tok)                                       # greedy: the token leads its alternatives
    assert torch.equal(_bits(lp["top_logprobs"][:B, :N, 0]), _bits(lp["token_logprobs"][:B, :N]))
    assert torch.equal(_bits(lp["cum_log_probs"][:B]), _bits(_fp32_running_sum(lp["token_logprobs"][:B, :N].cpu())))
    _, toks, rec = graph_run
    assert _mk(weights).generate_sampled_graph(PROMPTS, BT, N, seeds=_seeds(), **PARAMS) == toks
    assert rec["token_logprobs"].shape == (B, N) and rec["top_ids"].shape == (B, N, TOP) and rec["cum_log_probs"].shape == (B,)
    assert torch.isfinite(rec["token_logprobs"]).all() and (rec["token_logprobs"] <= 0).all()


def test_eager_steps_equal_capture_and_replay(weights, graph_run):
    eng_g, toks, rec = graph_run
    eng = _mk(weights)
    eng.set_logprobs(TOP, N)                                   # before the sampling config: the order does not matter
    eng.set_sampling(seeds=_seeds(), history_ld=max(len(p) for p in PROMPTS) + N, **PARAMS)
    eng.begin_sampled(PROMPTS, BT, N)
    for _ in range(N - 1):
        eng.step(B)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(_bits(eng.logprobs[k][:B]), _bits(eng_g.logprobs[k][:B])), k
    assert eng.logprobs["count"][:B].tolist() == [N] * B
    hist = eng.sampling["history"][:B].cpu()
    assert [hist[b, len(p): len(p) + N].tolist() for b, p in enumerate(PROMPTS)] == toks
    for e in (eng, eng_g):
        cols = e.logprobs["token_logprobs"][:B, :N].cpu()
        assert torch.equal(_bits(e.logprobs["cum_log_probs"][:B]), _bits(_fp32_running_sum(cols)))
    assert torch.equal(_bits(rec["token_logprobs"]), _bits(eng.logprobs["token_logprobs"][:B, :N]))
    # the greedy row of the sampling config: its token leads, with the token's own value
    assert eng.logprobs["top_ids"][0, :N, 0].tolist() == toks[0]
    assert torch.equal(_bits(eng.logprobs["top_logprobs"][0, :N, 0]), _bits(eng.logprobs["token_logprobs"][0, :N]))


def _check_column(lp, col, logits, temp, ids, exact_ids):
    ref = lr.reference(logits, temp, ids, TOP)
    got_tok = lp["token_logprobs"][:B, col].cpu()
    got_ids, got_val = lp["top_ids"][:B, col].cpu(), lp["top_logprobs"][:B, col].cpu()
    lr.assert_close(got_tok, ref["token"], f"column {col}: token value")
    assert (got_ids >= 0).all() and (got_ids < CFG.vocab).all()
    at_ids = np.take_along_axis(ref["lp"], got_ids.numpy().astype(np.int64), axis=1)
    lr.assert_close(got_val, at_ids, f"column {col}: value of a reported alternative at its id")
    lr.assert_close(got_val, ref["top_lp"], f"column {col}: sorted top-N values")
    assert all(len(set(r)) == TOP for r in got_ids.tolist())
    if exact_ids:
        assert np.array_equal(got_ids.numpy(), ref["top_ids"]), f"column {col}: ids"


def test_recorded_values_against_the_reference_step_by_step(weights):
    # temperature, top-k / top-p and a repetition penalty: eng.logits holds the penalised logits after a step
    eng = _mk(weights)
    eng.set_sampling(seeds=_seeds(), history_ld=max(len(p) for p in PROMPTS) + N, repetition_penalty=1.3, **PARAMS)
    eng.set_logprobs(TOP, N)
    eng.begin_sampled(PROMPTS, BT, N)
    temp = torch.tensor(PARAMS["temperature"])
    for step in range(1, N):
        eng.step(B)
        torch.cuda.synchronize()
        _check_column(eng.logprobs, step, eng.logits[:B].cpu(), temp, eng.token_ids[:B].cpu(), exact_ids=False)
    lp = eng.logprobs
    assert lp["top_ids"][0, 1:N, 0].tolist() == eng.sampling["history"][0, len(PROMPTS[0]) + 1: len(PROMPTS[0]) + N].tolist()
    assert torch.equal(_bits(lp["top_logprobs"][0, 1:N, 0]), _bits(lp["token_logprobs"][0, 1:N]))
    # temperature NULL, no penalties (the greedy tail), first token included: ids exact.  No reference gap is asserted first, as the
    # op-level tests do: with temperature NULL x = l exactly, so device and reference order the same fp32 values by the same tie rule
    eng = _mk(weights)
    eng.set_logprobs(TOP, N)
    logits = eng.prefill(PROMPTS, BT)
    first = ops.argmax(logits)
    eng.record_first_logprobs(logits, first)
    eng.set_inputs([0] * B, [len(p) for p in PROMPTS], BT)
    eng.token_ids[:B].copy_(first)
    _check_column(eng.logprobs, 0, logits.cpu(), None, first.cpu(), exact_ids=True)
    for step in range(1, N):
        eng.step(B)
        torch.cuda.synchronize()
        ids = eng.token_ids[:B].cpu()
        _check_column(eng.logprobs, step, eng.logits[:B].cpu(), None, ids, exact_ids=True)
        assert eng.logprobs["top_ids"][:B, step, 0].cpu().tolist() == ids.tolist()
        assert torch.equal(_bits(eng.logprobs["top_logprobs"][:B, step, 0]), _bits(eng.logprobs["token_logprobs"][:B, step]))
    assert eng.oob_count() == 0


def test_recorder_saturates_restarts_and_leaves_other_slots_alone(weights, graph_run):
    eng_g, toks, rec = graph_run
    L = 4
    eng = _mk(weights)
    eng.set_sampling(seeds=_seeds(), history_ld=max(len(p) for p in PROMPTS) + N, **PARAMS)
    lp = eng.set_logprobs(TOP, L)
    lp["token_logprobs"][B:].fill_(-7.25); lp["top_ids"][B:].fill_(-99); lp["top_logprobs"][B:].fill_(-7.25)
    lp["cum_log_probs"][B:].fill_(-7.25); lp["count"][B:].fill_(-99)
    eng.begin_sampled(PROMPTS, BT, N)
    eng.capture(B)
    eng.replay(B, L - 1)
    torch.cuda.synchronize()
    full = {k: lp[k].clone() for k in KEYS}
    assert lp["count"][:B].tolist() == [L] * B
    eng.replay(B, N - L)                                       # full: nothing more is recorded, the running sum goes on
    torch.cuda.synchronize()
    assert lp["count"][:B].tolist() == [L] * B
    for k in ("token_logprobs", "top_ids", "top_logprobs"):
        assert torch.equal(_bits(lp[k]), _bits(full[k])), k
        assert torch.equal(_bits(lp[k][:B]), _bits(rec[k][:, :L])), k
    assert torch.equal(_bits(lp["cum_log_probs"][:B]), _bits(rec["cum_log_probs"]))
    hist = eng.sampling["history"][:B].cpu()
    assert [hist[b, len(p): len(p) + N].tolist() for b, p in enumerate(PROMPTS)] == toks
    # slots past the batch keep what they held
    assert (lp["token_logprobs"][B:] == -7.25).all() and (lp["top_ids"][B:] == -99).all() and (lp["top_logprobs"][B:] == -7.25).all()
    assert (lp["cum_log_probs"][B:] == -7.25).all() and (lp["count"][B:] == -99).all()
    # the host rewrites count and the sum, the SAME graph records from column 0 again
    eng.begin_sampled(PROMPTS, BT, N)                          # same request again: the same tokens, the same values
    lp["count"][:B].zero_(); lp["cum_log_probs"][:B].zero_()
    lp["token_logprobs"][:B].fill_(9.0)
    eng.replay(B, 3)
    torch.cuda.synchronize()
    assert lp["count"][:B].tolist() == [3] * B
    assert torch.equal(_bits(lp["token_logprobs"][:B, :3]), _bits(rec["token_logprobs"][:, 1:4]))
    assert torch.equal(lp["top_ids"][:B, :3].cpu(), rec["top_ids"][:, 1:4])
    assert (lp["token_logprobs"][:B, 3] == 9.0).all()
    assert torch.equal(_bits(lp["cum_log_probs"][:B]), _bits(_fp32_running_sum(rec["token_logprobs"][:, 1:4])))


def _launches(prof):
    return {k: v["launches"] for k, v in prof.items()}


def test_launch_counts_and_tensor_parallel_refusal(weights):
    steps = 2

    def prof(e):
        e.set_inputs([1, 2, 3], [4, 2, 6], BT)
        return _launches(e.profile(B, steps))
    base = prof(_mk(weights))
    eng = _mk(weights)
    assert prof(eng) == base
    eng.set_logprobs(TOP, 16)
    with_lp = prof(eng)
    assert with_lp == {**base, "other": base["other"] + 2 * steps}
    eng.clear_logprobs()
    assert prof(eng) == base and eng.logprobs is None
    eng.set_sampling(seeds=_seeds(), history_ld=64, repetition_penalty=1.1, **PARAMS)
    sampled = prof(eng)
    eng.set_logprobs(0, 16)
    assert prof(eng) == {**sampled, "other": sampled["other"] + 2 * steps}
    eng.clear_sampling()
    assert prof(eng) == with_lp
    eng.clear_logprobs()
    assert prof(eng) == base
    # verify rows record nothing
    eng.set_logprobs(TOP, 16)
    eng.set_inputs([1, 2, 3, 4], [4, 5, 2, 3], BT[:2])
    st, h, lib = eng._st(), eng.handle, eng.lib
    _C.check(lib.mi355_decoder_begin_rows(h, 2, 2, st), "decoder_begin")
    for l in range(CFG.num_layers):
        _C.check(lib.mi355_decoder_layer_attn(h, l, st), "decoder_layer_attn")
        _C.check(lib.mi355_decoder_layer_mlp(h, l, st), "decoder_layer_mlp")
    _C.check(lib.mi355_decoder_finish(h, 1, st), "decoder_finish")          # with the (greedy) tail
    torch.cuda.synchronize()
    assert eng.logprobs["count"].tolist() == [0] * 8
    world = 2
    cfg = model.ModelConfig("tiny-tp", 2, 512, 8, 2, 64, 768, 1024, max_pos=256)
    w = model.synth_model(cfg, "w4", "cpu", seed=23, zeros="centered")
    shard = {"layers": [model.split_layer_tp(L, cfg, world, 0) for L in w["layers"]], "embedding": w["embedding"],
             "final_norm": w["final_norm"], "lm_head": w["lm_head"].cols(0, cfg.vocab // world)}
    tp = model.DecoderEngine(cfg.per_rank(world), model.weights_to(shard, DEV), kv_int8=False, page=16, num_blocks=8, max_batch=4,
                             max_seq_len=32, device=DEV, tp_size=world, vocab_full=cfg.vocab)
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        tp.set_logprobs(2, 4)
