"""Sampled decoding inside the step driver (mi355_decoder_set_sampling): the sampling tail in eager steps and in the captured graph,
on the tiny model of test_generate_sampled_end_to_end."""
import numpy as np
import pytest
import torch

from rtp_llm_amd import _C, model, ops
from tests import sample_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = model.ModelConfig("tiny-sampler", 2, 512, 8, 2, 64, 1024, 2048, max_pos=512)
PROMPTS = [[5, 9, 2, 7], [11, 3], [8, 8, 8, 1, 4, 6]]
BT = torch.arange(3 * 8, dtype=torch.int32).reshape(3, 8)
N = 12
SEEDS = [0x9E3779B97F4A7C15, 12345, 0xFFFFFFFF00000001]
OTHER = [7, 0xDEADBEEFCAFEF00D, 99]
PARAMS = dict(top_k=[8, 0, 20], top_p=[0.9, 0.8, 0.95], temperature=[1.3, 0.7, 1.0])


@pytest.fixture(scope="module")
def weights():
    return model.synth_model(CFG, "w4", DEV, seed=3)


def _mk(w):
    return model.DecoderEngine(CFG, w, kv_int8=False, page=16, num_blocks=64, max_batch=8, max_seq_len=128, device=DEV)


def _seeds(vals):
    return sr.seeds_as_int64(vals)


@pytest.fixture(scope="module")
def sampled(weights):
    """One sampled run through the graph, shared: (engine, tokens)."""
    eng = _mk(weights)
    toks = eng.generate_sampled_graph(PROMPTS, BT, N, seeds=_seeds(SEEDS), **PARAMS)
    return eng, toks


def test_greedy_rows_in_the_graph_equal_generate(weights):
    greedy = _mk(weights).generate(PROMPTS, BT, N)
    assert _mk(weights).generate_sampled_graph(PROMPTS, BT, N, top_k=1, seeds=_seeds(SEEDS)) == greedy
    assert _mk(weights).generate_sampled_graph(PROMPTS, BT, N, top_k=0, top_p=1e-6, temperature=0.7, seeds=_seeds(SEEDS)) == greedy
    # back to the greedy tail: the replayed tokens are the greedy ones again
    eng = _mk(weights)
    eng.generate_sampled_graph(PROMPTS, BT, 3, seeds=_seeds(SEEDS), **PARAMS)
    eng.clear_sampling()
    assert eng.generate(PROMPTS, BT, N) == greedy
    assert eng.oob_count() == 0


def test_eager_steps_equal_capture_and_replay(weights, sampled):
    eng_g, toks = sampled
    eng = _mk(weights)
    eng.set_sampling(seeds=_seeds(SEEDS), history_ld=max(len(p) for p in PROMPTS) + N, **PARAMS)
    eng.begin_sampled(PROMPTS, BT, N)
    for _ in range(N - 1):
        eng.step(3)
    torch.cuda.synchronize()
    lens = torch.tensor([len(p) for p in PROMPTS], dtype=torch.int32)
    for e in (eng, eng_g):
        hist, n = e.sampling["history"][:3].cpu(), e.sampling["history_len"][:3].cpu()
        assert torch.equal(n, lens + N) and torch.equal(e.positions[:3].cpu(), lens + N - 1)
        for b, pr in enumerate(PROMPTS):
            assert hist[b, : len(pr)].tolist() == pr and hist[b, len(pr): len(pr) + N].tolist() == toks[b], b
        assert int(e.token_ids[0]) == toks[0][-1]
        assert e.oob_count() == 0
    # the history saturates at history_ld: the token is still produced, the length stays
    eng.step(3)
    torch.cuda.synchronize()
    n = eng.sampling["history_len"][:3].cpu()
    assert int(n[2]) == eng.sampling["history"].shape[1] and torch.equal(eng.positions[:3].cpu(), lens + N)


def test_seeds_decide_the_tokens_and_may_be_rewritten_between_replays(weights, sampled):
    eng, toks = sampled
    assert _mk(weights).generate_sampled_graph(PROMPTS, BT, N, seeds=_seeds(SEEDS), **PARAMS) == toks
    fresh = _mk(weights).generate_sampled_graph(PROMPTS, BT, N, seeds=_seeds(OTHER), **PARAMS)
    assert fresh != toks
    # rewrite the seed array in place, prefill again, replay the SAME captured graph
    eng.sampling["seed"][:3].copy_(_seeds(OTHER))
    assert eng.generate_sampled_graph(PROMPTS, BT, N, reuse_sampling=True) == fresh
    eng.sampling["seed"][:3].copy_(_seeds(SEEDS))
    assert eng.generate_sampled_graph(PROMPTS, BT, N, reuse_sampling=True) == toks


def test_every_graph_token_is_a_valid_draw_from_teacher_forced_logits(weights, sampled):
    """Feed the graph's tokens to a fresh engine step by step (logits only): every token passes the op-level kept-set and CDF-interval
    checks against those logits with the numpy Philox number of (seed, position).  The logits are the model's, not the test's choice:
    at a step whose k-th and (k+1)-th scaled logits are closer than the op-level tests require of their inputs (1e-3; the kernel ranks
    exp(x - max) in fp32, which separates values about 1e-6 apart), the entries within that distance of the k-th value are undecided
    like those of the top-p band, and count towards the same limit of 8."""
    _, toks = sampled
    eng = _mk(weights)
    lens = [len(p) for p in PROMPTS]
    temp, tk, tp = (torch.tensor(PARAMS["temperature"]), torch.tensor(PARAMS["top_k"], dtype=torch.int32), torch.tensor(PARAMS["top_p"]))
    logits = eng.prefill(PROMPTS, BT)
    eng.set_inputs([0] * 3, lens, BT)
    for i in range(N):
        u = torch.from_numpy(sr.philox_uniform(SEEDS, [l + i for l in lens]))
        ids, out = ops.sample_logits(logits.clone(), temp, tk, tp, uniform=u, return_probs=True)
        sr.check_rows(logits.cpu(), temp, tk, tp, u, ids, out, k_band=True)
        assert ids.cpu().tolist() == [t[i] for t in toks], i
        if i + 1 < N:
            eng.token_ids[:3].copy_(ids)
            eng.forward(3)
            eng.positions[:3] += 1
            logits = eng.logits[:3]


def test_presence_penalty_over_the_device_history(weights):
    pp = _mk(weights).generate_sampled_graph(PROMPTS, BT, 16, top_k=1, presence_penalty=1e4, seeds=_seeds(SEEDS))
    for b in range(3):
        assert len(set(pp[b])) == 16 and not set(pp[b]) & set(PROMPTS[b]), (b, pp[b])


def test_set_sampling_is_refused_under_tensor_parallelism():
    world = 2
    cfg = model.ModelConfig("tiny-tp", 2, 512, 8, 2, 64, 768, 1024, max_pos=256)
    w = model.synth_model(cfg, "w4", "cpu", seed=23, zeros="centered")
    shard = {"layers": [model.split_layer_tp(L, cfg, world, 0) for L in w["layers"]], "embedding": w["embedding"],
             "final_norm": w["final_norm"], "lm_head": w["lm_head"].cols(0, cfg.vocab // world)}
    eng = model.DecoderEngine(cfg.per_rank(world), model.weights_to(shard, DEV), kv_int8=False, page=16, num_blocks=8, max_batch=4,
                              max_seq_len=32, device=DEV, tp_size=world, vocab_full=cfg.vocab)
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        eng.set_sampling(top_k=5, seeds=1)
    assert _C.ERR_UNSUPPORTED == -3
