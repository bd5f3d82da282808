"""Step time of Qwen3-8B widths with MXFP4 weights (e2m1 codes, e8m0 scale per 32 rows, synthetic, fp16 KV cache, hipGraph
replay) at b = 1, 8, 64 against three integer W4 arms on the same build, alternating in one process:

  mxfp4       e2m1 codes + e8m0 bytes (4.25 bits per weight): the staged chain (gemm_wq_kernel MXFP4 instances);
  w4_g32      integer W4 with 32-row groups (5 bits per weight), FORCED onto the same staged chain -- the like-for-like comparison:
              same launches, same block shapes, the instances the MXFP4 ones sit next to;
  w4_g128     integer W4 with 128-row groups (4.25 bits, the bytes of MXFP4), forced onto the staged chain as well;
  w4_g128_img integer W4 g128 on the launches the step driver picks for it by default (the image launches): the ceiling an MXFP4 image
              instance would aim for.

Forcing uses the tuning build's switches (mi355_debug_set; the product library has none): 5 = 2 and 6 = 99 while the engine is
created (no image launches, no few-row fused launches: what the plan predicates answer for MXFP4 anyway), 5 = 1 while the step is
captured (no gemm_wide, which has no MXFP4 instance either).  The MXFP4 engine is built and captured under the same switches, so the
three staged arms record the same launch sequence.

Each arm keeps its engine (captured once); the timed replays of the arms alternate, `--runs` of them each, and the table reports
the median and the spread.  Algorithmic bytes per step: every quantised weight once at its format's bits, the fp16 lm_head at 2
bytes, the KV cache rows read; the fraction is of the 8 TB/s HBM peak.

    python tools/mxfp4_step_time.py [--layers 36] [--steps 50] [--runs 4] [--ctx 256] [--batches 1,8,64] [--out profiles/mxfp4_step_time.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from dataclasses import replace

os.environ["MI355_TUNING_LIB"] = "1"   # before rtp_llm_amd._C is imported: the tuning build carries the switches

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtp_llm_amd import _C, model  # noqa: E402

HBM_PEAK_GBS = 8000.0
BITS = {"mxfp4": 4.25, "w4_g32": 5.0, "w4_g128": 4.25, "w4_g128_img": 4.25}


def tune(**kv):
    lib = _C.lib()
    lib.mi355_debug_set.argtypes = [C.c_int, C.c_int]
    for k, v in kv.items():
        lib.mi355_debug_set(int(k[1:]), int(v))


def make_engine(cfg, w, B, steps, ctx, staged, page=16):
    nb = (ctx + steps + 16 + page - 1) // page
    tune(t5=2 if staged else 0, t6=99 if staged else 0)                # the launch plan is made when the engine is created
    eng = model.DecoderEngine(cfg, w, kv_int8=False, page=page, num_blocks=B * nb, max_batch=B, max_seq_len=nb * page, device="cuda:0")
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)
    eng.set_inputs(list(range(100, 100 + B)), [ctx] * B, bt)
    tune(t5=1 if staged else 0)                                        # the GEMM family is chosen when the step is captured
    eng.capture(B)
    tune(t5=0, t6=0)
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


def step_bytes(cfg, B, ctx, bits):
    qkv_n = (cfg.nh + 2 * cfg.nkv) * cfg.hd
    per_layer = cfg.hidden * qkv_n + cfg.nh * cfg.hd * cfg.hidden + cfg.hidden * 2 * cfg.inter + cfg.inter * cfg.hidden
    weights = cfg.num_layers * per_layer * bits / 8
    return weights + cfg.hidden * cfg.vocab * 2 + cfg.num_layers * B * ctx * 2 * cfg.nkv * cfg.hd * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--ctx", type=int, default=256)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=None, help="also write the table lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_step_time: no GPU (a step time is measured on the MI355X or not at all)")
    torch.cuda.set_device(0)
    cfg = replace(model.QWEN3_8B, num_layers=a.layers, max_pos=4096)
    weights = {"mxfp4": model.synth_model(cfg, "mxfp4", "cuda:0", seed=0),
               "w4_g32": model.synth_model(cfg, "w4", "cuda:0", seed=0, group_size=32, zeros="centered"),
               "w4_g128": model.synth_model(cfg, "w4", "cuda:0", seed=0, group_size=128, zeros="centered")}
    arms = {"mxfp4": ("mxfp4", True), "w4_g32": ("w4_g32", True), "w4_g128": ("w4_g128", True), "w4_g128_img": ("w4_g128", False)}
    lines = [f"# qwen3-8b widths, {a.layers} layers, 4-bit weights, fp16 KV, ctx {a.ctx}, hipGraph replay, {a.steps} steps x {a.runs} alternating runs; "
             "ms per step: median (min .. max), share of the 8 TB/s HBM peak on the arm's own algorithmic bytes"]
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        engines = {k: make_engine(cfg, weights[wk], B, a.steps, a.ctx, staged) for k, (wk, staged) in arms.items()}
        times = {k: [] for k in arms}
        for _ in range(a.runs):
            for k, (eng, bt) in engines.items():
                times[k].append(timed(eng, bt, B, a.steps, a.ctx))
        del engines
        torch.cuda.empty_cache()
        row = {"b": B}
        for k, ts in times.items():
            med, nbytes = statistics.median(ts), step_bytes(cfg, B, a.ctx, BITS[k])
            row[k] = {"ms": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "bytes_per_step": int(nbytes),
                      "hbm_frac": round(nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            vs = "" if k == "mxfp4" else f"  mxfp4 vs this: {100 * (row['mxfp4']['ms'] / med - 1):+.2f} %"
            lines.append(f"b={B:<3d} {k:<12s} {med:8.4f} ms ({min(ts):.4f} .. {max(ts):.4f})  hbm {row[k]['hbm_frac']:.3f}{vs}")
            print(lines[-1], flush=True)
        rows.append(row)
    print(json.dumps({"model": lines[0][2:], "rows": rows}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
