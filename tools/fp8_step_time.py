"""Step time of Qwen3-8B widths with FP8 e4m3 weights (128 x 128 block scales, synthetic, fp16 KV cache, hipGraph replay) at
b = 1, 8, 64 against two INT8 arms on the same build, alternating in one process:

  fp8        FP8 codes + fp32 group scales: the staged chain (gemm_smallm / gemm_wq_kernel FP8 instances);
  int8_g128  INT8 codes with 128-row groups (pack_w8 + a grouped {zneg, scale} meta): the same staged chain, the instances the
             FP8 ones sit next to -- the like-for-like comparison;
  int8_pc    per-channel INT8: takes the image launches, the ceiling an FP8 image instance would aim for.

Each arm keeps its engine (captured once); the timed replays of the arms alternate, `--runs` of them each, and the table
reports the median and the spread.  Algorithmic bytes per step: every quantised weight once at 1 + 4/128 bytes, the fp16 lm_head
at 2 bytes, the KV cache rows read; the fraction is of the 8 TB/s HBM peak.

    python tools/fp8_step_time.py [--layers 36] [--steps 50] [--runs 4] [--ctx 256] [--batches 1,8,64]
"""
import argparse
import json
import os
import statistics
import sys
from dataclasses import replace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtp_llm_amd import model, quant  # noqa: E402

HBM_PEAK_GBS = 8000.0


class Int8G128:
    """INT8 codes with one fp16 scale per (128-row group, column): the format launch_gemm_t<8, 4> serves.  Only what DecoderEngine
    asks of a layer's linear: pack()."""

    def __init__(self, K, N, device, gen):
        a = (6.0 / (K + N)) ** 0.5
        w = (torch.rand(K, N, device=device, generator=gen) * 2 - 1) * a
        amax = w.reshape(K // 128, 128, N).abs().amax(dim=1).clamp(min=1e-8)
        self.scales = (amax / 127.0).half()
        self.q = torch.clamp((w.reshape(K // 128, 128, N) / self.scales.float()[:, None, :]).round(), -128, 127).to(torch.int8).reshape(K, N)
        self.K, self.N = K, N

    def pack(self, gate_up=False, dtype=torch.float16):
        il = (lambda t: quant.interleave_gate_up(t, -1)) if gate_up else (lambda t: t)
        K_pad, N_pad = quant._ceil_to(self.K, 128), quant._ceil_to(self.N, 16)
        z = torch.full_like(self.scales, 128, dtype=torch.int16)
        return quant.PackedWeight(quant.pack_w8(il(self.q)), quant.make_meta(z, il(self.scales), N_pad), 8, self.K, self.N, K_pad, N_pad, 128)


def with_linears(w, make):
    return {**w, "layers": [{**L, **{k: make(L[k].K, L[k].N) for k in ("qkv", "o", "gate_up", "down")}} for L in w["layers"]]}


def make_engine(cfg, w, B, steps, ctx, page=16):
    nb = (ctx + steps + 16 + page - 1) // page
    eng = model.DecoderEngine(cfg, w, kv_int8=False, page=page, num_blocks=B * nb, max_batch=B, max_seq_len=nb * page, device="cuda:0")
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)
    eng.set_inputs(list(range(100, 100 + B)), [ctx] * B, bt)
    eng.capture(B)
    eng.replay(B, 5)
    torch.cuda.synchronize()
    return eng, bt


def timed(eng, bt, B, steps, ctx):
    eng.set_inputs(list(range(100, 100 + B)), [ctx] * B, bt)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream())
    eng.replay(B, steps)
    b.record(torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert eng.oob_count() == 0
    return a.elapsed_time(b) / steps


def step_bytes(cfg, B, ctx):
    qkv_n = (cfg.nh + 2 * cfg.nkv) * cfg.hd
    per_layer = cfg.hidden * qkv_n + cfg.nh * cfg.hd * cfg.hidden + cfg.hidden * 2 * cfg.inter + cfg.inter * cfg.hidden
    weights = cfg.num_layers * per_layer * (1 + 4 / 128)
    return weights + cfg.hidden * cfg.vocab * 2 + cfg.num_layers * B * ctx * 2 * cfg.nkv * cfg.hd * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--ctx", type=int, default=256)
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = replace(model.QWEN3_8B, num_layers=a.layers, max_pos=4096)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    base = model.synth_model(cfg, "fp8", "cuda:0", seed=0)
    arms = {"fp8": base,
            "int8_g128": with_linears(base, lambda K, N: Int8G128(K, N, "cuda:0", gen)),
            "int8_pc": with_linears(base, lambda K, N: model.synth_linear(K, N, "int8", "cuda:0", gen))}
    out = {"model": f"qwen3-8b widths, {a.layers} layers, 8-bit weights, fp16 KV, ctx {a.ctx}, hipGraph replay, {a.steps} steps x {a.runs} alternating runs",
           "rows": []}
    for B in [int(x) for x in a.batches.split(",")]:
        engines = {k: make_engine(cfg, w, B, a.steps, a.ctx) for k, w in arms.items()}
        times = {k: [] for k in arms}
        for _ in range(a.runs):
            for k, (eng, bt) in engines.items():
                times[k].append(timed(eng, bt, B, a.steps, a.ctx))
        del engines
        torch.cuda.empty_cache()
        nbytes = step_bytes(cfg, B, a.ctx)
        row = {"b": B, "bytes_per_step": int(nbytes)}
        for k, ts in times.items():
            med = statistics.median(ts)
            row[k] = {"ms": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
                      "hbm_frac": round(nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        row["fp8_vs_int8_g128_pct"] = round(100 * (row["fp8"]["ms"] / row["int8_g128"]["ms"] - 1), 2)
        row["fp8_vs_int8_pc_pct"] = round(100 * (row["fp8"]["ms"] / row["int8_pc"]["ms"] - 1), 2)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
