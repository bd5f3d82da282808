"""Step time of Qwen3-8B W4A16 (synthetic weights, fp16 KV cache, hipGraph replay) at b = 1, 8, 64 with the per-head QK norm and the
same shape without it: the difference prices the composed QKV path (split-K QKV + normalising KV writer) that replaces the fused
QKV launches when the norm is on.

    python tools/qwen3_step_time.py [--layers 36] [--steps 50] [--ctx 256] [--batches 1,8,64]
"""
import argparse
import json
import os
import sys
from dataclasses import replace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtp_llm_amd import model  # noqa: E402


def step_ms(cfg, w, B, steps, ctx, page=16):
    nb = (ctx + steps + 16 + page - 1) // page
    eng = model.DecoderEngine(cfg, w, kv_int8=False, page=page, num_blocks=B * nb, max_batch=B, max_seq_len=nb * page, device="cuda:0")
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)
    eng.set_inputs(list(range(100, 100 + B)), [ctx] * B, bt)
    eng.capture(B)
    eng.replay(B, 5)
    torch.cuda.synchronize()
    eng.set_inputs(list(range(100, 100 + B)), [ctx] * B, bt)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream())
    eng.replay(B, steps)
    b.record(torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert eng.oob_count() == 0
    del eng
    torch.cuda.empty_cache()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--ctx", type=int, default=256)
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    on = replace(model.QWEN3_8B, num_layers=a.layers, max_pos=4096)
    off = replace(on, qk_norm=False)
    w = model.synth_model(on, "w4", "cuda:0", seed=0, zeros="centered")
    w_off = {**w, "layers": [{k: v for k, v in L.items() if k not in ("q_norm", "k_norm")} for L in w["layers"]]}
    out = {"model": f"qwen3-8b W4A16 g128, {a.layers} layers, fp16 KV, ctx {a.ctx}, hipGraph replay, {a.steps} steps", "rows": []}
    for B in [int(x) for x in a.batches.split(",")]:
        t_on = step_ms(on, w, B, a.steps, a.ctx)
        t_off = step_ms(off, w_off, B, a.steps, a.ctx)
        row = {"b": B, "qk_norm_ms": round(t_on, 4), "no_norm_ms": round(t_off, 4), "delta_ms": round(t_on - t_off, 4),
               "delta_pct": round(100 * (t_on - t_off) / t_off, 2)}
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
