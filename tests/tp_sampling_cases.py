"""What the CPU and the GPU tests of sampled decoding under tensor parallelism share (tests/test_tp_sampling_cpu.py,
tests/test_gpu_tp_sampling.py): the tiny-tp model of tests/test_gpu_allreduce.py, the per-row sampling parameters of the sampled step,
and the oracle's view of its first step."""
import torch

from oracle import oracle
from rtp_llm_amd import model

CFG = model.ModelConfig("tiny-tp", 2, 512, 8, 2, 64, 768, 1024, max_pos=256)
WEIGHT_SEED = 21          # tests/test_tp_sampling_cpu.py checks that the oracle's step-0 rows stay inside sample_ref.MAX_FREE with it
B, PAGE = 5, 16
SEEDS = [0x9E3779B97F4A7C15, 12345, 0xFFFFFFFF00000001, 7, 0xDEADBEEFCAFEF00D]
# row 0: top_k == 1 (greedy under a sampling config); row 1: top-p only; rows 2, 3: mixed / top-k only; row 4: a tight nucleus
PARAMS = dict(temperature=[1.3, 0.7, 1.0, 0.9, 1.1], top_k=[1, 0, 20, 8, 0], top_p=[0.9, 0.8, 0.95, 1.0, 0.6])
PRESENCE = [0.0, 0.0, 0.8, 0.0, 0.5]      # a presence penalty on rows 2 and 4 (0: the row's logits pass through bit for bit)


def first_tokens():
    return torch.randint(0, CFG.vocab, (B,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)


def weights(seed=WEIGHT_SEED):
    return model.synth_model(CFG, "w4", "cpu", seed=seed, zeros="centered")


def oracle_decoder(w):
    dense = lambda c: (c.w.float() if c.kind == "fp16" else oracle.dequant_groupwise(c.q, c.z_eff, c.scales, c.group_size))
    ow = {"embedding": w["embedding"], "final_norm": w["final_norm"], "lm_head": dense(w["lm_head"]),
          "layers": [{"input_norm": L["input_norm"], "post_norm": L["post_norm"], "qkv_bias": L["qkv_bias"],
                      **{k: dense(L[k]) for k in ("qkv", "o", "gate_up", "down")}} for L in w["layers"]]}
    return oracle.OracleDecoder({**CFG.__dict__}, ow)


def shard(w, world, rank):
    """This rank's weights: Megatron split of the layers, the vocabulary columns [rank * V / world, (rank + 1) * V / world) of the lm_head."""
    V = CFG.vocab
    return {"layers": [model.split_layer_tp(L, CFG, world, rank) for L in w["layers"]], "embedding": w["embedding"],
            "final_norm": w["final_norm"], "lm_head": w["lm_head"].cols(rank * (V // world), (rank + 1) * (V // world))}


def oracle_step0_rows(w):
    """The oracle's logits of the sampled step's first step, after the presence penalty over the one-token history: [B, vocab] fp32."""
    tok = first_tokens()
    _, ref = oracle_decoder(w).forward_tokens(tok, torch.zeros(B, dtype=torch.int32), oracle.OracleKV(CFG.num_layers, B, False), list(range(B)))
    return oracle.apply_penalties(ref, presence_penalty=PRESENCE, output_ids=tok.reshape(1, B).numpy(), input_lengths=[1] * B, max_input_length=1, step=1)
