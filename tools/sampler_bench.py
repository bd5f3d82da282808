#!/usr/bin/env python3
"""Launch times of the sampler kernels behind lm_head at the Qwen2 vocabulary (B rows x 152064 fp32 logits, 2048-token history).

    sampler_bench.py            the single launches of the host-side sampler (host wrapper + launch)
    sampler_bench.py --tail     the fused sampling tail (mi355_sample_logits) against the chain temperature + softmax_rows +
                                top_k_top_p_sample, both replayed from a graph (device time, no host wrapper), alternating
    sampler_bench.py --step     ms / step of the Qwen2-7B W4A16 decode step (b = 64, ctx 1024, graph replay): greedy tail against the
                                sampled tail, each without and with the log-probability recorder (top 0 / top 20), and the
                                host-side generate_sampled loop next to them
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtp_llm_amd import model, ops  # noqa: E402


def timed(fn, iters=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def graphed(fn):
    """fn recorded once into a graph: replays cost device time only (the host wrappers allocate and convert per call)."""
    fn(); fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def alternate(pairs, reps=7, iters=30):
    """us per call of every (name, replay) in `pairs`, alternating them: median and range over `reps` windows of `iters` replays."""
    res = {name: [] for name, _ in pairs}
    for _ in range(reps):
        for name, fn in pairs:
            res[name].append(timed(fn, iters))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in res.items()}


def bench_tail(B, V, L):
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    peaked = (torch.randn(B, V, generator=g) * 3).to(dev)
    flat = torch.randn(B, V, generator=g).to(dev)
    hist_rows = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32).to(dev)      # fused: [B][L], lengths on the device
    hist_cols = hist_rows.t().contiguous()                                                 # chain: [L][B]
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    u = torch.rand(B, generator=g).to(dev)
    f32 = lambda v: torch.full((B,), v, dtype=torch.float32, device=dev)
    # T + 1e-6 == 1 in fp32 and neutral penalties: the in-place launches of both sides leave the rows unchanged from replay to replay
    temp, rep, zero = f32(1.0 - 1e-6), f32(1.0), f32(0.0)
    k50, p90, p100 = torch.full((B,), 50, dtype=torch.int32, device=dev), f32(0.9), f32(1.0)
    settings = [("k = 50, p = 0.9 (randn * 3)", peaked, k50, p90, False), ("p = 0.9 alone, flat randn * 1 rows", flat, None, p90, False),
                ("k = 0, p = 1 (randn * 3)", peaked, None, p100, False), ("p = 0.9 flat + penalties over a 2048-token history", flat, None, p90, True)]
    print(f"# sampling tail, B = {B} rows x V = {V} fp32: fused mi355_sample_logits vs the chain (graph replay, us per call: median [min .. max] of 7 windows x 30)")
    for name, x, k, p, pen in settings:
        x = x.clone()

        def chain():
            if pen:
                ops.apply_penalties(x, temperature=temp, repetition_penalty=rep, presence_penalty=zero, frequency_penalty=zero,
                                    output_ids=hist_cols, max_input_length=0, step=L)
            else:
                ops.apply_penalties(x, temperature=temp)
            ops.top_k_top_p_sample(ops.softmax_rows(x), k, p, u)

        def fused():
            if pen:
                ops.apply_penalties_history(x, hist_rows, lens, rep, zero, zero)
            ops.sample_logits(x, temp, k, p, uniform=u)
        same = torch.equal(ops.sample_logits(x, temp, k, p, uniform=u), ops.top_k_top_p_sample(ops.softmax_rows(x), k, p, u))
        r = alternate([("chain", graphed(chain)), ("fused", graphed(fused))])
        c, f = r["chain"], r["fused"]
        print(f"{name:52s} chain {c[0]:8.1f} [{c[1]:7.1f} .. {c[2]:7.1f}]   fused {f[0]:7.1f} [{f[1]:6.1f} .. {f[2]:6.1f}]   "
              f"chain / fused {c[0] / f[0]:5.2f}   same ids: {same}")
    survivors = int((ops.sample_logits(flat, temp, None, p90, uniform=u, return_probs=True)[1][0] > 0).sum())
    print(f"# survivors of row 0 in the flat p = 0.9 setting: {survivors}")
    # the two launches of mi355_logprobs on the same rows (what a step with the recorder adds to its tail)
    ids = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).to(dev)
    r = alternate([(f"top {n}", graphed(lambda n=n: ops.logprobs(peaked, ids=ids, temperature=temp, top_n=n))) for n in (0, 1, 20, 32)])
    print(f"# mi355_logprobs, B = {B} rows x V = {V} fp32 (graph replay, us per call: median [min .. max] of 7 windows x 30)")
    for name, t in r.items():
        print(f"logprobs {name:43s} {t[0]:7.1f} [{t[1]:6.1f} .. {t[2]:6.1f}]")


def bench_step(B, ctx, steps):
    dev = "cuda:0"
    cfg = model.QWEN2_7B
    gen = torch.Generator(device=dev).manual_seed(1000)
    layers = [model.synth_layer(cfg, "w4", dev, gen, zeros="centered") for _ in range(cfg.num_layers)]
    gs = torch.Generator(device=dev).manual_seed(7)
    for Lw in layers:
        Lw["input_norm"] = (1.0 + 0.1 * torch.randn(cfg.hidden, device=dev, generator=gs)).half()
        Lw["post_norm"] = (1.0 + 0.1 * torch.randn(cfg.hidden, device=dev, generator=gs)).half()
    weights = {"layers": layers, "embedding": (torch.randn(cfg.vocab, cfg.hidden, device=dev, generator=gs) * 0.5).half(),
               "final_norm": (1.0 + 0.1 * torch.randn(cfg.hidden, device=dev, generator=gs)).half(),
               "lm_head": model.synth_linear(cfg.hidden, cfg.vocab, "fp16", dev, gen)}
    page, max_seq = 16, ctx + 4 * steps + 64
    bps = (max_seq + page - 1) // page
    eng = model.DecoderEngine(cfg, weights, kv_int8=False, page=page, num_blocks=B * bps, max_batch=B, max_seq_len=max_seq, device=dev)
    del weights, layers
    for l in range(cfg.num_layers):
        eng.kv[l].copy_(torch.randn(eng.kv[l].shape, device=dev, generator=gen, dtype=torch.float16))
    ids0 = torch.randint(0, cfg.vocab, (B,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    bt = torch.randperm(B * bps, generator=torch.Generator().manual_seed(2)).reshape(B, bps).to(torch.int32)
    hist0 = torch.randint(0, cfg.vocab, (B, ctx), generator=torch.Generator().manual_seed(3), dtype=torch.int32)

    def reset():
        eng.set_inputs(ids0.tolist(), [ctx - 1] * B, bt)
        if getattr(eng, "sampling", None) is not None:
            eng.sampling["history"][:, :ctx].copy_(hist0)
            eng.sampling["history_len"].fill_(ctx)
        if eng.logprobs is not None:
            eng.logprobs["count"].zero_()                      # every timed step records

    def replay_ms():
        reset(); eng.capture(B); eng.replay(B, 8); torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            reset(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); eng.replay(B, steps); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / steps)
        return ts
    passes = 2
    print(f"# decode step, Qwen2-7B W4A16, fp16 KV, b = {B}, ctx {ctx}, graph replay of {steps} steps "
          f"(ms / step: median [min .. max] of {5 * passes} windows, the rows taken in turn {passes} times; earlier forms of this "
          f"mode took 5 windows per row in one pass and repeated the greedy row: their lines do not compare with these one to one)")
    sampled = dict(temperature=0.7, top_k=20, top_p=0.8)
    rows = [("greedy tail", None, None), ("greedy tail + logprobs top 0", None, 0), ("greedy tail + logprobs top 20", None, 20),
            ("sampled tail: T 0.7, k 20, p 0.8", sampled, None), ("sampled tail + logprobs top 0", sampled, 0),
            ("sampled tail + logprobs top 20", sampled, 20),
            ("sampled tail: + repetition penalty 1.05", dict(sampled, repetition_penalty=1.05), None),
            ("sampled tail: + repetition penalty 1.05 + logprobs top 20", dict(sampled, repetition_penalty=1.05), 20)]
    res = {name: [] for name, _, _ in rows}
    for _ in range(passes):
        for name, kw, top in rows:
            if kw is None:
                eng.clear_sampling()
            else:
                eng.set_sampling(seeds=torch.arange(B, dtype=torch.int64) + 11, history_ld=max_seq + 1, **kw)
            if top is None:
                eng.clear_logprobs()
            else:
                eng.set_logprobs(top, steps + 8)
            res[name] += replay_ms()
    for name, _, _ in rows:
        t = sorted(res[name])
        print(f"{name:58s} {t[len(t) // 2]:7.3f} [{t[0]:7.3f} .. {t[-1]:7.3f}] ms / step")
    eng.clear_logprobs()
    # the host-side path of generate_sampled: one eager step without sampling, sampler.sample_greedy over its logits, ids.cpu()
    from rtp_llm_amd import sampler
    eng.clear_sampling()
    lens = torch.full((B,), ctx, dtype=torch.int32)
    n = min(steps, 16)
    hist = torch.zeros(B, ctx + n + 2, dtype=torch.int32); hist[:, :ctx] = hist0
    for name, pen in (("generate_sampled loop (host-side sampler): T 0.7, k 20, p 0.8", False), ("generate_sampled loop: + repetition penalty 1.05", True)):
        ts = []
        for rep_i in range(3):
            reset(); eng.forward(B); torch.cuda.synchronize()
            seq = lens.clone()
            u = torch.rand(n, B, generator=torch.Generator().manual_seed(5))
            t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(n):
                step = int(seq.max())
                params = sampler.GreedyParams(logits=eng.logits[:B], input_lengths=lens, sequence_lengths=seq, token_ids=hist[:, : step + 1].contiguous(),
                                              step=step, top_k=torch.full((B,), 20, dtype=torch.int32), top_p=torch.full((B,), 0.8),
                                              temperature=torch.full((B,), 0.7), repetition_penalty=torch.full((B,), 1.05) if pen else None,
                                              presence_penalty=torch.zeros(B) if pen else None, frequency_penalty=torch.zeros(B) if pen else None,
                                              uniform=u[i])
                ids = sampler.sample_greedy(params)
                hist[torch.arange(B), seq.long()] = ids.cpu()
                seq += 1
                eng.token_ids[:B].copy_(ids)
                eng.forward(B)
                eng.positions[:B] += 1
            t1.record(); torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1) / n)
        ts.sort()
        print(f"{name:66s} {ts[1]:7.3f} [{ts[0]:7.3f} .. {ts[2]:7.3f}] ms / step ({n} steps per window)")
    print(f"# oob_count {eng.oob_count()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64); ap.add_argument("--vocab", type=int, default=152064); ap.add_argument("--hist", type=int, default=2048)
    ap.add_argument("--tail", action="store_true", help="fused sampling tail against the chain"); ap.add_argument("--step", action="store_true", help="greedy against sampled decode step")
    ap.add_argument("--ctx", type=int, default=1024); ap.add_argument("--steps", type=int, default=64)
    a = ap.parse_args()
    if a.tail or a.step:
        if a.tail:
            bench_tail(a.batch, a.vocab, a.hist)
        if a.step:
            bench_step(a.batch, a.ctx, a.steps)
        return
    dev = "cuda:0"
    B, V, L = a.batch, a.vocab, a.hist
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(B, V, generator=g) * 3).to(dev)
    hist = torch.randint(0, V, (L, B), generator=g, dtype=torch.int32).to(dev)
    ones = torch.ones(B)
    probs = ops.softmax_rows(logits)
    u = torch.rand(B, generator=g).to(dev)
    rows = [
        ("argmax (greedy fast path)", lambda: ops.argmax(logits)),
        ("apply_penalties: temperature", lambda: ops.apply_penalties(logits, temperature=ones * 0.8)),
        ("apply_penalties: repetition + presence + frequency", lambda: ops.apply_penalties(logits, repetition_penalty=ones * 1.1, presence_penalty=ones * 0.1,
                                                                                              frequency_penalty=ones * 0.1, output_ids=hist, max_input_length=0, step=L)),
        ("ban_repeat_ngram (n = 3)", lambda: ops.ban_repeat_ngram(logits, hist.t().contiguous(), torch.full((B,), L - 1, dtype=torch.int32), torch.full((B,), 3, dtype=torch.int32))),
        ("softmax_rows", lambda: ops.softmax_rows(logits)),
        ("sample_rows (no filter)", lambda: ops.sample_rows(probs, u)),
        ("top_k_top_p_sample (k = 50, p = 0.9)", lambda: ops.top_k_top_p_sample(probs, torch.full((B,), 50, dtype=torch.int32), ones * 0.9, u)),
        ("top_k_top_p_sample (p = 0.9, renormalised probabilities out)", lambda: ops.top_k_top_p_sample(probs, None, ones * 0.9, u, return_probs=True)),
    ]
    print(f"# sampler kernels, B = {B} rows x V = {V} fp32, history {L} tokens (host wrapper + launch, us per call)")
    for name, fn in rows:
        print(f"{name:62s} {timed(fn):9.1f} us")


if __name__ == "__main__":
    main()
