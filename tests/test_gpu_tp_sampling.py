"""Sampled decoding and log-probabilities under tensor parallelism, with the ranks as PROCESSES ON ONE GPU (the harness of
tests/test_gpu_allreduce.py: IPC handles map a peer's buffers across processes on one device as across devices, gloo is the control
plane): the vocabulary all-gather of the fp32 logits (mi355_allgather_logits), the step driver's tail on the gathered rows
(mi355_decoder_set_gathered_logits + set_sampling / set_logprobs at tp_size > 1) over both transports, its contract, and
generate_sampled_graph at world 2.  Everything the ranks compute is compared bit for bit with the tp-1 ops run on the concatenated
logits, and against the CPU references of tests/sample_ref.py / tests/logprob_ref.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

NAN_PAYLOAD = 0x7FC12345          # a quiet NaN whose payload must survive the gather


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_cpu(t, world):
    import torch.distributed as dist
    outs = [torch.empty_like(t.cpu()) for _ in range(world)]
    dist.all_gather(outs, t.cpu().contiguous())
    return outs


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _cat_bits(t, world):
    """The ranks' fp32 [B, V] slices side by side, exchanged and compared as int32 (NaN payloads intact)."""
    return torch.cat(_gather_cpu(_bits(t), world), dim=1)


def _diff_report(got, want, raw):
    """Where two [B, V] fp32 tensors differ bitwise: per row the count and the first columns, with the values (and the unpenalised one)."""
    g, w, r = _bits(got), _bits(want), raw.detach().cpu()
    out = []
    for b in range(g.shape[0]):
        cols = torch.nonzero(g[b] != w[b]).reshape(-1)
        if cols.numel():
            c = int(cols[0])
            out.append((b, int(cols.numel()), cols[:4].tolist(), float(got[b, c]), float(want[b, c]), float(r[b, c])))
    return out


def _same_on_all_ranks(t, world, what):
    parts = _gather_cpu(_bits(t), world)
    assert all(torch.equal(parts[0], o) for o in parts[1:]), what


# ---------------------------------------------------------------------------------------------------------------- 1. the gather op
def _gather_mode(ar, rank, world, dev, distributed, dist):
    small = distributed.CustomAllReduce(max_bytes=64 << 10, verify=False)      # (64, 516) = 129 KB: three launches per call
    g = torch.Generator().manual_seed(900 + rank)

    def slice_of(B, V, salt=0):
        x = torch.randn(B, V, generator=g) * (3.0 + salt)
        xi = x.view(torch.int32)
        row = min(1, B - 1)
        x[row, 0], x[row, 1] = float("-inf"), float("inf")
        xi[row, 2] = NAN_PAYLOAD + rank
        return x

    def check(ctx, x, what):
        got = ctx.all_gather_logits(x.to(dev))
        torch.cuda.synchronize()
        assert got.shape == (x.shape[0], x.shape[1] * world)
        assert torch.equal(_bits(got), _cat_bits(x, world)), what

    shapes = [(1, 4), (5, 1000), (64, 516), (3, 37988)]
    for ctx, name in ((ar, "one launch"), (small, "64 KiB context")):
        for B, V in shapes:
            check(ctx, slice_of(B, V), (name, B, V))
    assert distributed.logits_gather_bytes(64, 516) > small.max_bytes and distributed.logits_gather_bytes(3, 37988) <= ar.max_bytes
    # an odd number of calls back to back, no host synchronisation in between: both parities, the last call on the first one again
    xs = [slice_of(5, 1000, i) for i in range(3)]
    for ctx in (ar, small):
        outs = [ctx.all_gather_logits(x.to(dev)) for x in xs]
        torch.cuda.synchronize()
        for i, (x, o) in enumerate(zip(xs, outs)):
            assert torch.equal(_bits(o), _cat_bits(x, world)), ("back to back", i)
    # interleaved with all-reduces of two widths and the cross-rank arg-max on the same context: every location keeps its owner block
    idx = lambda T, H: torch.arange(T * H, dtype=torch.int64).reshape(T, H)
    pat = lambda T, H, r: ((idx(T, H) * (r + 3) + r) % 61 - 30).to(torch.float16)       # |value| <= 30: the sums of 4 ranks are exact
    a896, a3584 = pat(7, 896, rank).to(dev), pat(33, 3584, rank).to(dev)
    lg = torch.randn(9, 512, generator=torch.Generator().manual_seed(5))
    lg[4, 100] = 60.0 + rank                                                            # the last rank holds the largest value
    x1, x2, x3 = slice_of(64, 516), slice_of(5, 1000), slice_of(3, 37988)
    o1 = ar.all_gather_logits(x1.to(dev))
    s1 = ar.all_reduce(a896.clone())
    o2 = ar.all_gather_logits(x2.to(dev))
    s2 = ar.all_reduce(a3584.clone())
    ids = ar.argmax(lg.to(dev), rank * 512)
    o3 = ar.all_gather_logits(x3.to(dev))
    s3 = ar.all_reduce(a896.clone())
    torch.cuda.synchronize()
    for x, o in ((x1, o1), (x2, o2), (x3, o3)):
        assert torch.equal(_bits(o), _cat_bits(x, world)), ("interleaved", tuple(x.shape))
    want896 = sum(pat(7, 896, r).float() for r in range(world)).half()
    assert torch.equal(s1.cpu(), want896) and torch.equal(s3.cpu(), want896)
    assert torch.equal(s2.cpu(), sum(pat(33, 3584, r).float() for r in range(world)).half())
    full = torch.cat(_gather_cpu(lg, world), dim=1)
    assert torch.equal(ids.cpu(), torch.argmax(full, -1).int())
    # captured and replayed 7 times (odd: both parities, the counters end where an eager call expects them); the 64 KiB context's launches too
    xa, xb = torch.empty(64, 516, device=dev), torch.empty(5, 1000, device=dev)
    oa, ob = torch.empty(64, 516 * world, device=dev), torch.empty(5, 1000 * world, device=dev)
    torch.cuda.synchronize(); dist.barrier()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        xa.copy_(slice_of(64, 516)); xb.copy_(slice_of(5, 1000))
        small.all_gather_logits(xa, oa); ar.all_gather_logits(xb, ob)              # warm-up
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            small.all_gather_logits(xa, oa)
            ar.all_gather_logits(xb, ob)
        for rep in range(7):
            ha, hb = slice_of(64, 516, rep), slice_of(5, 1000, rep)
            xa.copy_(ha); xb.copy_(hb); oa.zero_(); ob.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(oa), _cat_bits(ha, world)) and torch.equal(_bits(ob), _cat_bits(hb, world)), ("replay", rep)
    # one rank (rotating) held back by a matmul in front of its call: its peers really wait on its flags
    slow = torch.randn(1024, 1024, device=dev)
    for it in range(world + 1):
        x = slice_of(64, 516, it)
        xd = x.to(dev)
        if it % world == rank:
            for _ in range(4):
                slow = (slow @ slow).clamp_(-1, 1)
        got = (small if it % 2 else ar).all_gather_logits(xd)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _cat_bits(x, world)), ("delayed rank", it)
    # refusals
    from rtp_llm_amd import _C
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        ar.all_gather_logits(torch.zeros(4, 6, device=dev))                        # not whole 16-byte vectors
    assert ar.status() == 0 and small.status() == 0
    small.close()


# ---------------------------------------------------------------------------------------------------------------- the tiny-tp engine
def _engine(world, rank, dev, w, max_batch=None):
    from rtp_llm_amd import model
    from tests import tp_sampling_cases as tc
    mb = tc.B if max_batch is None else max_batch
    return model.DecoderEngine(tc.CFG.per_rank(world), model.weights_to(tc.shard(w, world, rank), dev), kv_int8=False, page=tc.PAGE,
                               num_blocks=mb * 2, max_batch=mb, max_seq_len=32, device=dev, tp_size=world, vocab_full=tc.CFG.vocab)


def _start(eng):
    """Step 0 of the decode-only runs: the shared first tokens at position 0, each its sequence's one-token history."""
    from tests import tp_sampling_cases as tc
    tok = tc.first_tokens()
    eng.set_inputs(tok.tolist(), [0] * tc.B, torch.arange(tc.B * 2, dtype=torch.int32).reshape(tc.B, 2))
    if getattr(eng, "sampling", None) is not None:
        eng.sampling["history"].zero_(); eng.sampling["history_len"].zero_()
        eng.sampling["history"][:tc.B, 0].copy_(tok)
        eng.sampling["history_len"][:tc.B].fill_(1)


def _set_sampling(eng):
    from tests import sample_ref as sr
    from tests import tp_sampling_cases as tc
    eng.set_sampling(seeds=sr.seeds_as_int64(tc.SEEDS), presence_penalty=tc.PRESENCE, history_ld=16, **tc.PARAMS)


def _sampled_steps(eng, rank, world, dev, dist, nsteps=6, logprobs_top=None):
    """Capture, then `nsteps` replayed steps of the sampled tail, each checked against the tp-1 ops on the concatenated logits."""
    from rtp_llm_amd import ops
    from tests import logprob_ref as lr
    from tests import sample_ref as sr
    from tests import tp_sampling_cases as tc
    B, V = tc.B, tc.CFG.vocab
    temp, tk, tp = torch.tensor(tc.PARAMS["temperature"]), torch.tensor(tc.PARAMS["top_k"], dtype=torch.int32), torch.tensor(tc.PARAMS["top_p"])
    pres = torch.tensor(tc.PRESENCE)
    s = eng.sampling
    _start(eng)
    dist.barrier()
    eng.capture(B)
    cols = []
    for step in range(nsteps):
        hist0, len0, pos0, tok0 = s["history"].clone(), s["history_len"].clone(), eng.positions.clone(), eng.token_ids.clone()
        eng.replay(B, 1)
        torch.cuda.synchronize()
        concat = torch.cat(_gather_cpu(_bits(eng.logits[:B]), world), dim=1).view(torch.float32).to(dev)     # the ranks' raw slices
        assert concat.shape == (B, V)
        pen = ops.apply_penalties_history(concat.clone(), hist0[:B].contiguous(), len0[:B], None, pres, None)
        assert torch.equal(_bits(eng.full_logits[:B]), _bits(pen)), ("rows of the tail", step, _diff_report(eng.full_logits[:B], pen, concat))
        free = [b for b in range(B) if tc.PRESENCE[b] == 0.0]                      # penalties off: the gathered rows bit for bit
        assert torch.equal(_bits(eng.full_logits[free]), _bits(concat[free])), step
        want = ops.sample_logits(pen.clone(), temp, tk, tp, seed=s["seed"][:B], draw_positions=pos0[:B] + 1)
        ids = eng.token_ids[:B].clone()
        assert torch.equal(ids, want), (step, ids.tolist(), want.tolist())
        # the tp-1 contract of the feedback, identical on every rank
        assert torch.equal(eng.positions[:B], pos0[:B] + 1)
        assert torch.equal(s["history_len"][:B], len0[:B] + 1)
        assert torch.equal(s["history"][torch.arange(B, device=dev), len0[:B].long()], ids)
        keep = s["history"][:B].clone(); keep[torch.arange(B, device=dev), len0[:B].long()] = hist0[torch.arange(B, device=dev), len0[:B].long()]
        assert torch.equal(keep, hist0[:B])
        for t, what in ((ids, "tokens"), (eng.positions[:B], "positions"), (s["history"], "history"), (s["history_len"], "history_len")):
            _same_on_all_ranks(t, world, (what, step))
        if step == 0:       # against the CPU reference: kept set, renormalised probabilities, CDF interval of the draw
            u = torch.from_numpy(sr.philox_uniform(tc.SEEDS, (pos0[:B].cpu() + 1).tolist()))
            ids2, out = ops.sample_logits(pen.clone(), temp, tk, tp, uniform=u, return_probs=True)
            sr.check_rows(pen.cpu(), temp, tk, tp, u, ids2, out, k_band=True)
            assert torch.equal(ids2, ids)
        if logprobs_top is not None:
            lp = eng.logprobs
            r = ops.logprobs(pen, ids=ids, temperature=temp, top_n=logprobs_top)
            assert torch.equal(_bits(lp["token_logprobs"][:B, step]), _bits(r["token_logprobs"])), step
            assert torch.equal(lp["top_ids"][:B, step], r["top_ids"]) and torch.equal(_bits(lp["top_logprobs"][:B, step]), _bits(r["top_logprobs"])), step
            ref = lr.reference(pen.cpu(), temp, ids, logprobs_top)
            lr.assert_close(lp["token_logprobs"][:B, step], ref["token"], f"step {step}: token value")
            lr.assert_close(lp["top_logprobs"][:B, step], ref["top_lp"], f"step {step}: sorted top-N values")
            cols.append(r["token_logprobs"].cpu())
            for k in ("token_logprobs", "top_ids", "top_logprobs", "cum_log_probs", "count"):
                _same_on_all_ranks(lp[k], world, (k, step))
        if step == nsteps - 1:     # an eager step from the same state gives the same tokens as the replay (the K/V it rewrites are the same)
            got_lp = None if logprobs_top is None else {k: v.clone() for k, v in eng.logprobs.items() if torch.is_tensor(v)}
            s["history"].copy_(hist0); s["history_len"].copy_(len0); eng.positions.copy_(pos0); eng.token_ids.copy_(tok0)
            if logprobs_top is not None:
                eng.logprobs["count"][:B] -= 1
            eng.step(B)
            torch.cuda.synchronize()
            assert torch.equal(eng.token_ids[:B], ids) and torch.equal(eng.positions[:B], pos0[:B] + 1)
            if logprobs_top is not None:
                assert torch.equal(_bits(eng.logprobs["token_logprobs"][:B, step]), _bits(got_lp["token_logprobs"][:B, step]))
    if logprobs_top is not None:
        acc = np.zeros(B, dtype=np.float32)
        for c in cols:
            acc = (acc + c.numpy()).astype(np.float32)
        # (the eager repeat of the last step added its value once more: one more fp32 add)
        acc = (acc + cols[-1].numpy()).astype(np.float32)
        assert torch.equal(_bits(eng.logprobs["cum_log_probs"][:B]), _bits(torch.from_numpy(acc)))
        assert eng.logprobs["count"][:B].tolist() == [nsteps] * B


def _greedy_logprob_steps(eng, rank, world, dev, dist, nsteps=6, top=3):
    """The greedy tail with log-probabilities on: ids = arg-max of the concatenated row, values bit-equal to ops.logprobs on the gathered rows."""
    from rtp_llm_amd import ops
    from tests import logprob_ref as lr
    from tests import tp_sampling_cases as tc
    B = tc.B
    _start(eng)
    dist.barrier()
    eng.capture(B)
    for step in range(nsteps):
        eng.replay(B, 1)
        torch.cuda.synchronize()
        concat = torch.cat(_gather_cpu(_bits(eng.logits[:B]), world), dim=1).view(torch.float32)
        assert torch.equal(_bits(eng.full_logits[:B]), _bits(concat)), step
        ids = eng.token_ids[:B].clone()
        assert torch.equal(ids.cpu(), torch.argmax(concat, -1).int()), step
        assert torch.equal(eng.positions[:B].cpu(), torch.full((B,), step + 1, dtype=torch.int32))
        lp = eng.logprobs
        r = ops.logprobs(concat.to(dev), ids=ids, top_n=top)
        assert torch.equal(_bits(lp["token_logprobs"][:B, step]), _bits(r["token_logprobs"])), step
        assert torch.equal(lp["top_ids"][:B, step], r["top_ids"]) and torch.equal(_bits(lp["top_logprobs"][:B, step]), _bits(r["top_logprobs"])), step
        assert torch.equal(lp["top_ids"][:B, step, 0], ids)                        # greedy: the token leads its alternatives
        ref = lr.reference(concat, None, ids, top)
        lr.assert_close(lp["token_logprobs"][:B, step], ref["token"], f"greedy step {step}: token value")
        lr.assert_close(lp["top_logprobs"][:B, step], ref["top_lp"], f"greedy step {step}: sorted top-N values")
        for k in ("token_logprobs", "top_ids", "top_logprobs", "cum_log_probs", "count"):
            _same_on_all_ranks(lp[k], world, (k, step))
    cols = eng.logprobs["token_logprobs"][:B, :nsteps].cpu()
    acc = np.zeros(B, dtype=np.float32)
    for c in range(nsteps):
        acc = (acc + cols[:, c].numpy()).astype(np.float32)
    assert torch.equal(_bits(eng.logprobs["cum_log_probs"][:B]), _bits(torch.from_numpy(acc)))


class _StubTransport:
    """mi355_collective_t whose callbacks enqueue the IPC kernels (RCCL refuses two ranks on one device): the `transport` mode of
    tests/test_gpu_allreduce.py."""

    def __init__(self, ar, hidden):
        from rtp_llm_amd import _C
        lib = _C.lib()

        def all_reduce(ctx, buf, count, stream):
            return lib.mi355_allreduce_sum(ar.handle, buf, buf, count // hidden, hidden, stream)

        def all_gather(ctx, send, recv, nbytes, stream):
            assert nbytes % 16 == 0
            return lib.mi355_allgather_hidden(ar.handle, send, recv, 1, nbytes // 2, stream)
        self._fns = (_C.ALL_REDUCE_FN(all_reduce), _C.ALL_GATHER_FN(all_gather))
        self.collective = _C.Collective(None, self._fns[0], _C.ALL_REDUCE_FN(), self._fns[1], ar.rank, ar.world)


def _contract_mode(ar, rank, world, dev, dist, w):
    import ctypes as C
    from rtp_llm_amd import _C
    from tests import tp_sampling_cases as tc
    B, Vl = tc.B, tc.CFG.vocab // world
    eng, plain = _engine(world, rank, dev, w), _engine(world, rank, dev, w)
    for e in (eng, plain):
        e.attach_allreduce(ar, rank * Vl)
    # without the buffer: refused exactly as before
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        _set_sampling(eng)
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        eng.set_logprobs(3, 8)
    # one byte short
    need = eng.lib.mi355_decoder_gathered_logits_bytes(C.byref(eng._structs[0]))
    assert need >= B * world * Vl * 4
    buf = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert eng.lib.mi355_decoder_set_gathered_logits(eng.handle, buf.data_ptr(), need - 1) == _C.ERR_WORKSPACE
    assert eng.lib.mi355_decoder_set_gathered_logits(eng.handle, buf.data_ptr() + 16, need) == _C.ERR_ARG          # not 256-byte aligned
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        eng.set_logprobs(3, 8)                                                     # a refused buffer enables nothing
    # the buffer enabled, no config: launch for launch the step of an engine without it
    eng.enable_gathered_logits()
    assert eng.full_logits.shape == (B, world * Vl) and eng.full_logits.dtype == torch.float32
    _start(eng); _start(plain)
    dist.barrier()
    pa, pb = eng.profile(B, 1), plain.profile(B, 1)
    assert {k: v["launches"] for k, v in pa.items()} == {k: v["launches"] for k, v in pb.items()}, (pa, pb)
    greedy_comm = pb["comm"]["launches"]
    assert torch.equal(eng.token_ids[:B], plain.token_ids[:B]) and torch.equal(_bits(eng.logits[:B]), _bits(plain.logits[:B]))
    # accepted now; each config adds what the issue says and nothing else: one gather launch (COMM), the tail's launches (OTHER)
    _set_sampling(eng)
    eng.set_logprobs(3, 8)
    _start(eng)
    dist.barrier()
    ps = eng.profile(B, 1)
    assert ps["comm"]["launches"] == greedy_comm                                   # the gather launch replaces the cross-rank arg-max launch
    with pytest.raises(_C.Mi355Error, match="mi355 error -1"):
        eng.disable_gathered_logits()                                              # a config is active
    # verify rows (q_len = 2) stay greedy and gather nothing: the gathered rows, the history and the recorder are left alone
    eng.full_logits.fill_(-7.0)
    len0, cnt0 = eng.sampling["history_len"].clone(), eng.logprobs["count"].clone()
    nseq, q_len = 2, 2
    toks = torch.randint(0, tc.CFG.vocab, (nseq * q_len,), generator=torch.Generator().manual_seed(77), dtype=torch.int32)
    eng.set_inputs(toks.tolist(), [1, 2, 1, 2], torch.arange(nseq * 2, dtype=torch.int32).reshape(nseq, 2))
    dist.barrier()
    st, h, lib = eng._st(), eng.handle, eng.lib
    _C.check(lib.mi355_decoder_begin_rows(h, nseq, q_len, st), "decoder_begin_rows")
    for l in range(tc.CFG.num_layers):
        _C.check(lib.mi355_decoder_layer_attn(h, l, st), "decoder_layer_attn")
        _C.check(lib.mi355_decoder_layer_mlp(h, l, st), "decoder_layer_mlp")
    _C.check(lib.mi355_decoder_finish(h, 1, st), "decoder_finish")
    torch.cuda.synchronize()
    full = torch.cat(_gather_cpu(_bits(eng.logits[:nseq * q_len]), world), dim=1).view(torch.float32)
    assert torch.equal(eng.token_ids[:nseq * q_len].cpu(), torch.argmax(full, -1).int())
    assert bool((eng.full_logits == -7.0).all())
    assert torch.equal(eng.sampling["history_len"], len0) and torch.equal(eng.logprobs["count"], cnt0)
    eng.clear_sampling(); eng.clear_logprobs()
    eng.disable_gathered_logits()
    assert eng.full_logits is None
    with pytest.raises(_C.Mi355Error, match="mi355 error -3"):
        eng.set_logprobs(3, 8)
    # a slice that is not at rank * vocab is refused
    other = _engine(world, rank, dev, w)
    other.attach_allreduce(ar, (world - 1 - rank) * Vl)
    other.enable_gathered_logits()
    if world - 1 - rank != rank:
        with pytest.raises(_C.Mi355Error, match="mi355 error -1"):
            other.set_logprobs(3, 8)
    assert ar.status() == 0 and eng.oob_count() == 0


def _generate_mode(ar, rank, world, dev, dist, w):
    from rtp_llm_amd import ops
    from tests import sample_ref as sr
    from tests import tp_sampling_cases as tc
    prompts = [[5, 9, 2, 7], [11, 3], [8, 8, 8, 1, 4, 6]]
    bt = torch.arange(3 * 2, dtype=torch.int32).reshape(3, 2)
    n, seeds = 8, tc.SEEDS[:3]
    params = dict(top_k=[8, 0, 20], top_p=[0.9, 0.8, 0.95], temperature=[1.3, 0.7, 1.0])
    Vl = tc.CFG.vocab // world
    eng = _engine(world, rank, dev, w, max_batch=8)
    eng.attach_allreduce(ar, rank * Vl)
    eng.enable_gathered_logits()
    dist.barrier()
    toks, rec = eng.generate_sampled_graph(prompts, bt, n, seeds=sr.seeds_as_int64(seeds), top_logprobs=2, **params)
    assert eng.oob_count() == 0
    assert all(len(t) == n and all(0 <= x < tc.CFG.vocab for x in t) for t in toks)
    both = [None] * world
    dist.all_gather_object(both, (toks, {k: _bits(v).tolist() for k, v in rec.items()}))
    assert all(b == both[0] for b in both[1:])
    assert rec["token_logprobs"].shape == (3, n) and rec["top_ids"].shape == (3, n, 2)
    assert torch.isfinite(rec["token_logprobs"]).all() and (rec["token_logprobs"] <= 0).all()
    # teacher-forced: every token passes the kept-set and CDF-interval checks against the gathered logits of a fresh engine
    ref = _engine(world, rank, dev, w, max_batch=8)
    ref.attach_allreduce(ar, rank * Vl)
    lens = [len(p) for p in prompts]
    temp, tk, tp = torch.tensor(params["temperature"]), torch.tensor(params["top_k"], dtype=torch.int32), torch.tensor(params["top_p"])
    dist.barrier()
    logits = ar.all_gather_logits(ref.prefill(prompts, bt))
    ref.set_inputs([0] * 3, lens, bt)
    for i in range(n):
        u = torch.from_numpy(sr.philox_uniform(seeds, [l + i for l in lens]))
        ids, out = ops.sample_logits(logits.clone(), temp, tk, tp, uniform=u, return_probs=True)
        sr.check_rows(logits.cpu(), temp, tk, tp, u, ids, out, k_band=True)
        assert ids.cpu().tolist() == [t[i] for t in toks], i
        if i + 1 < n:
            ref.token_ids[:3].copy_(ids)
            ref.forward(3)
            ref.positions[:3] += 1
            logits = ar.all_gather_logits(ref.logits[:3])
    assert ar.status() == 0 and ref.oob_count() == 0


def _worker(rank, world, port, q, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if mode.endswith("_ff"):      # plain stores between system-scope release / acquire fences
        os.environ["MI355_AR_FULL_FENCES"] = "1"
        mode = mode[:-3]
    elif mode.endswith("_ll"):    # the granule protocol: the gather keeps the flag form, next to granule all-reduces on the same context
        os.environ["MI355_AR_LL"] = "1"
        mode = mode[:-3]
    try:
        import torch.distributed as dist
        from rtp_llm_amd import distributed
        from tests import tp_sampling_cases as tc
        dev = "cuda:0"
        torch.cuda.set_device(0)
        torch.set_num_threads(max(1, min(32, (os.cpu_count() or 8) // world)))
        distributed.init_distributed("gloo")
        ar = distributed.CustomAllReduce(max_bytes=300 * 8192 * 2)
        assert ar.shared_device
        Vl = tc.CFG.vocab // world
        if mode == "gather":
            _gather_mode(ar, rank, world, dev, distributed, dist)
        else:
            w = tc.weights()
        if mode == "sampled":
            eng = _engine(world, rank, dev, w)
            eng.attach_allreduce(ar, rank * Vl)
            eng.enable_gathered_logits()
            _set_sampling(eng)
            _sampled_steps(eng, rank, world, dev, dist)
            assert ar.status() == 0 and eng.oob_count() == 0
        elif mode == "logprobs":
            eng = _engine(world, rank, dev, w)
            eng.attach_allreduce(ar, rank * Vl)
            eng.enable_gathered_logits()
            eng.set_logprobs(3, 8)                                 # before the sampling config: the order does not matter
            _set_sampling(eng)
            _sampled_steps(eng, rank, world, dev, dist, logprobs_top=3)
            greedy = _engine(world, rank, dev, w)
            greedy.attach_allreduce(ar, rank * Vl)
            greedy.enable_gathered_logits()
            greedy.set_logprobs(3, 8)
            _greedy_logprob_steps(greedy, rank, world, dev, dist)
            assert ar.status() == 0 and eng.oob_count() == 0 and greedy.oob_count() == 0
        elif mode == "transport":
            eng = _engine(world, rank, dev, w)
            eng.attach_collective(_StubTransport(ar, tc.CFG.hidden), rank * Vl)
            eng.enable_gathered_logits()
            _set_sampling(eng)
            _sampled_steps(eng, rank, world, dev, dist)
            assert ar.status() == 0 and eng.oob_count() == 0
        elif mode == "contract":
            _contract_mode(ar, rank, world, dev, dist, w)
        elif mode == "generate":
            _generate_mode(ar, rank, world, dev, dist, w)
        assert ar.status() == 0
        dist.barrier()
        ar.close()
        q.put((rank, "ok"))
    except BaseException as e:  # noqa: BLE001  (pytest.raises failures are BaseException-derived Failed)
        import traceback
        q.put((rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()[-2500:]}"))
    finally:
        try:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:  # noqa: BLE001
            pass


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode,world", [("gather", 2), ("gather", 4), ("gather_ff", 2), ("gather_ll", 2), ("sampled", 2), ("logprobs", 2),
                                        ("transport", 2), ("contract", 2), ("generate", 2)])
def test_tp_sampling_processes_on_one_gpu(mode, world):
    assert torch.cuda.is_available()
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, mode)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=240))
            if res[-1][1] != "ok":       # a rank that failed leaves its peers waiting in a collective: report it now
                break
    except Exception as e:  # noqa: BLE001  (queue.Empty: a rank died or hung)
        res.append(("missing", repr(e)))
    failed = any(r[1] != "ok" for r in res)
    for p in procs:
        p.join(1 if failed else 30)
        if p.is_alive():
            p.kill()
    assert sorted(res) == [(r, "ok") for r in range(world)], res
