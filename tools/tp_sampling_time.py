"""What the sampled tail costs a tensor-parallel step: the replayed step greedy vs sampled vs sampled + log-probabilities, and the logits
gather launch alone, with the ranks as processes on ONE GPU.

    python tools/tp_sampling_time.py [--worlds 2,4] [--batches 8,64] [--layers 4] [--steps 50] [--runs 5] [--greedy-only] [--out profiles/tp_sampling_tail.txt]

Qwen2-7B per-rank widths (hidden 3584, 28 q / 4 kv heads, FFN 18944, the whole 152064-token vocabulary), `--layers` of its 28 layers: the
tail does not depend on the depth, and the table gives the step of the same depth beside it.  Started without WORLD_SIZE the script
becomes the launcher of its own ranks, like `bench.py --gpus N`.  The arms alternate inside one process, `--runs` blocks of `--steps`
replayed steps each; median and the min-max spread of the blocks are printed (the spread of the greedy arm is the run-to-run noise a
comparison with another build has to beat).

One-device peers share an L2 / MALL and no link: every figure here is a LOWER bound of what a fabric costs.  Per rank and step the
gather pulls (world - 1) / world * B * V * 4 bytes from its peers; no xGMI hop has ever run for this repository."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launch(args):
    import socket
    lines = []
    for world in [int(x) for x in args.worlds.split(",")]:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        procs = []
        for r in range(world):
            env = {**os.environ, "RANK": str(r), "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                   "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True))
        out, _ = procs[0].communicate()
        rcs = [p.wait() for p in procs]
        if any(rcs):
            print(f"world {world}: ranks exited with {rcs}", file=sys.stderr)
            return 1
        lines.append("".join(l for l in out.splitlines(True) if not l.startswith("[Gloo]")))     # the control plane's own chatter
    text = __doc__.split("\n\n")[-1].replace("\n", " ") + "\n\n" + "".join(lines)
    print(text)
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write(text)
    return 0


def rank_main(args):
    import torch
    import torch.distributed as dist
    from rtp_llm_amd import distributed, model
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = "cuda:0"
    torch.cuda.set_device(0)
    distributed.init_distributed("gloo")
    batches = [int(x) for x in args.batches.split(",")]
    MB = max(batches)
    full = model.QWEN2_7B
    cfg = model.ModelConfig("qwen2-7b-widths", args.layers, full.hidden, full.nh, full.nkv, full.hd, full.inter, full.vocab, max_pos=512)
    w = model.synth_model(cfg, "w4", dev, seed=5, zeros="centered")
    Vl = cfg.vocab // world
    shard = {"layers": [model.split_layer_tp(L, cfg, world, rank) for L in w["layers"]], "embedding": w["embedding"],
             "final_norm": w["final_norm"], "lm_head": w["lm_head"].cols(rank * Vl, (rank + 1) * Vl)}
    del w
    ar = distributed.CustomAllReduce(max_bytes=MB * cfg.hidden * 2 if args.greedy_only else max(MB * cfg.hidden * 2, distributed.logits_gather_bytes(MB, Vl)))
    ctx, page = 256, 16
    nblk = (ctx + 64 + page - 1) // page
    eng = model.DecoderEngine(cfg.per_rank(world), shard, kv_int8=False, page=page, num_blocks=MB * nblk, max_batch=MB,
                              max_seq_len=ctx + 64, device=dev, tp_size=world, vocab_full=cfg.vocab)
    eng.attach_allreduce(ar, rank * Vl)
    if not args.greedy_only:
        eng.enable_gathered_logits()
    bt = torch.arange(MB * nblk, dtype=torch.int32).reshape(MB, nblk)

    def block(B):
        """One timed block of args.steps replayed steps from the same start (max over ranks: a TP step ends when its slowest rank does)."""
        eng.set_inputs([1] * B, [ctx] * B, bt[:B])
        if getattr(eng, "sampling", None) is not None:
            eng.sampling["history_len"].zero_()
        if eng.logprobs is not None:
            eng.logprobs["count"].zero_()
        torch.cuda.synchronize(); dist.barrier()
        t0 = time.perf_counter()
        eng.replay(B, args.steps)
        torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t) / args.steps * 1e3

    def arm(name):
        if name == "greedy":
            if getattr(eng, "sampling", None) is not None:
                eng.clear_sampling()
            if eng.logprobs is not None:
                eng.clear_logprobs()
        elif name == "sampled":
            eng.set_sampling(top_k=50, top_p=0.9, temperature=0.8, seeds=list(range(1, MB + 1)), history_ld=args.steps + 2)
            if eng.logprobs is not None:
                eng.clear_logprobs()
        else:
            eng.set_sampling(top_k=50, top_p=0.9, temperature=0.8, seeds=list(range(1, MB + 1)), history_ld=args.steps + 2)
            eng.set_logprobs(5, args.steps)

    out = [f"world {world} (processes on one GPU), Qwen2-7B widths, {args.layers} layers, per-rank vocabulary {Vl}, ctx {ctx}, {args.steps} replayed steps x {args.runs} blocks, "
           f"hand-over {ar.hand_over}\n"]
    fmt = lambda v: f"{statistics.median(v):.4f} ({min(v):.4f}-{max(v):.4f})"
    for B in batches:
        times = {"greedy": []} if args.greedy_only else {"greedy": [], "sampled": [], "sampled+logprobs": []}
        for run in range(args.runs + 1):                   # arms alternate; the first block of each arm (capture, cold caches) is dropped
            for name in times:
                arm(name)
                dist.barrier()
                eng.capture(B)
                v = block(B)
                if run:
                    times[name].append(v)
        if args.greedy_only:       # the arm a build without the feature has too: for A/B runs of two trees on one machine
            out.append(f"  b = {B:2d}: step ms  greedy {fmt(times['greedy'])}\n")
            continue
        # the gather launch alone: events around 20 launches, 5 times
        x = torch.randn(B, Vl, device=dev)
        y = torch.empty(B, Vl * world, device=dev)
        gl = []
        for _ in range(6):
            torch.cuda.synchronize(); dist.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                ar.all_gather_logits(x, y)
            e1.record(); torch.cuda.synchronize()
            t = torch.tensor([e0.elapsed_time(e1) / 20 * 1e3], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            gl.append(float(t))
        pulled = (world - 1) * B * Vl * 4 / 1e6
        out.append(f"  b = {B:2d}: step ms  greedy {fmt(times['greedy'])}  sampled {fmt(times['sampled'])}  sampled+logprobs {fmt(times['sampled+logprobs'])}  |  "
                   f"gather launch alone {statistics.median(gl[1:]):.1f} us ({min(gl[1:]):.1f}-{max(gl[1:]):.1f}), {pulled:.1f} MB pulled per rank\n")
    st = ar.status()
    if st or eng.oob_count():
        raise RuntimeError(f"all-reduce status {st} / out-of-range tokens")
    if rank == 0:
        sys.stdout.write("".join(out))
        sys.stdout.flush()
    dist.barrier()
    ar.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="2,4")
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--greedy-only", action="store_true", help="time the greedy step only (runs on a tree without the feature: A/B of two builds)")
    a = ap.parse_args()
    sys.exit(launch(a) if "WORLD_SIZE" not in os.environ else rank_main(a))
