// Entry points shared between translation units of libmi355_decode.so but not part
// of the public C-ABI (include/mi355_decode.h).
#pragma once
#include "../../include/mi355_decode.h"
/* Why an entry point must refuse this cache's intra-block layout (mi355_kv_layer_t.layout), or NULL: the non-native layouts exist for
 * the 16-bit caches with hd 64 / 128 and page 16 / 32 / 64 only; every entry point that takes a cache asks before it launches anything. */
static inline const char* mi355_kv_layout_problem(int32_t layout, int32_t kv_dtype, int32_t hd, int32_t page) {
    if (layout == MI355_KV_LAYOUT_NATIVE) return 0;
    if (layout != MI355_KV_LAYOUT_REF && layout != MI355_KV_LAYOUT_REF_VVEC) return "unknown kv layout";
    if (kv_dtype != MI355_KV_FP16 && kv_dtype != MI355_KV_BF16) return "the reference kv layouts take fp16 / bf16 caches only (no INT8)";
    if (hd != 64 && hd != 128) return "the reference kv layouts take hd 64 or 128";
    if (page != 16 && page != 32 && page != 64) return "the reference kv layouts take page 16, 32 or 64";
    return 0;
}
#define MI355_CHECK_KV_LAYOUT(kv, name)                                                                                         \
    do {                                                                                                                        \
        if (const char* why__ = mi355_kv_layout_problem((kv)->layout, (kv)->kv_dtype, (kv)->hd, (kv)->page)) {                  \
            mi355_set_error("%s: layout=%d kv_dtype=%d hd=%d page=%d: %s", name, (kv)->layout, (kv)->kv_dtype, (kv)->hd, (kv)->page, why__); \
            return MI355_ERR_ARG;                                                                                               \
        }                                                                                                                       \
    } while (0)
/* Format code the GEMM launchers take in place of a bare mi355_weight_t.wbits (their `wbits` parameter): 4 / 8 / 16 for integer / 16-bit
 * weights, MI355_WFMT_FP8 for wkind = MI355_WKIND_FP8_E4M3.  A launcher without an FP8 instance matches none of its integer cases on
 * that code and returns MI355_ERR_UNSUPPORTED, so an FP8 image can never be decoded as INT8 g128 by falling through.  MI355_WFMT_MXFP4
 * (wkind = MI355_WKIND_MXFP4) works the same way: no launcher's `wbits == 4` case matches it, so an e2m1 image is never read as integer
 * W4 g32. */
enum { MI355_WFMT_FP8 = 0x108, MI355_WFMT_MXFP4 = 0x204 };
static inline int mi355_wfmt(const mi355_weight_t* w) {
    return w->wkind == MI355_WKIND_FP8_E4M3 ? MI355_WFMT_FP8 : w->wkind == MI355_WKIND_MXFP4 ? MI355_WFMT_MXFP4 : w->wbits;
}
#ifdef __cplusplus
extern "C" {
#endif
int mi355_gemm_plan(int M, const mi355_weight_t* w, int max_splits, int* nbw_out, int* cps_out);
int mi355_linear_direct(const void* x, int32_t M, const mi355_weight_t* w, const void* bias, void* y, int32_t epilogue,
                        void* workspace, size_t workspace_bytes, mi355_stream_t stream);
int mi355_argmax_ex(const float* logits, int32_t B, int32_t V, int32_t ld, int32_t* ids, int32_t* positions, void* workspace,
                    size_t workspace_bytes, mi355_stream_t stream);
/* seq_lens_minus_one != 0: seq_lens[] holds tokens already cached (decode "positions"), context = value + 1 */
int mi355_paged_decode_attn_ex(const void* q, const mi355_kv_layer_t* kv, const int32_t* block_table,
                               int32_t max_blocks_per_seq, const int32_t* seq_lens, int32_t seq_lens_minus_one, int32_t B,
                               int32_t nh, float scale, int32_t max_seq_len, void* out, void* workspace,
                               size_t workspace_bytes, mi355_stream_t stream);
int mi355_fullk_weight_ok(const mi355_weight_t* w);
int mi355_fullk64_weight_ok(const mi355_weight_t* w);     /* gemm.hip: the full-K launches on activation images (gemm_fullk64.hip) take this linear */
int mi355_fullk64_qkv_ok(const mi355_weight_t* w, int32_t hd);   /* ... as the QKV + RoPE launch (also K up to 9600 when its tile pairs leave half the chip free) */
int mi355_gemm_wide_direct_ok(const mi355_weight_t* w);   /* gemm_wide.hip: the one-launch form takes this linear (N fills the chip) */
int mi355_gemm_splitk64_plan(int M, int NT, int KC, int wbits, int group_size, int max_splits, int* cps_out);   /* gemm_splitk64.hip: slabs, or < 0 */
int mi355_gemm_splitk64_direct_plan(int M, int NT, int KC, int wbits, int group_size);   /* gemm_splitk64.hip, direct form: tiles per block, or < 0 */
int mi355_prefetch(const void* ptr, size_t bytes, void* sink, mi355_stream_t stream);
/* Touch plan: the blocks a latency-bound launch has to spare (the slab fold in front of a QKV launch: 64 blocks on 256 CUs) read one dword per
 * 128-byte line of the weights the NEXT launch streams, so that its first requests are served by the Infinity Cache (or the XCD's L2)
 * instead of HBM under the launch burst.  Unit u = what block u of the next launch reads, touched by a block on the same XCD (block b runs
 * on XCD b % 8 -- observed, speed only).  For gemm_fullk64's QKV launch unit u is the (d, d + hd/2) tile pair u: two runs of run_bytes at
 * tiles (u / hh) 2 hh + u % hh and + hh, and the (zero, scale) words of those tiles.  No effect on any result. */
typedef struct {
    const void* qw; const void* meta;     /* weight image, (zero, scale) words [groups][N_pad] */
    uint32_t run_bytes;                   /* bytes of one tile's weights (contiguous) */
    uint32_t meta_groups, meta_stride;    /* groups along K, dwords from group to group */
    int32_t  n_units, hh;                 /* tile pairs, tiles per half head */
    void*    sink;                        /* a dword nobody reads */
    int32_t  delay;                       /* the spare blocks wait delay x 512 cycles first (the launch's own requests go out ahead) */
} mi355_touch_t;
int mi355_qkv_touch_plan(const mi355_weight_t* wqkv, int32_t hd, void* sink, mi355_touch_t* out);   /* gemm.hip: MI355_OK, or MI355_ERR_UNSUPPORTED */
int mi355_add_rmsnorm_img_touch(const void* x_f16, const float* partials, int32_t nsplit, int32_t ld, const void* bias, const void* residual_in,
                                void* residual_out, const void* weight, float eps, int32_t M, int32_t H, void* y_img, int32_t act_dtype,
                                const mi355_touch_t* touch, mi355_stream_t stream);
/* Round 6, tensor parallelism: a row-parallel shard (O / down) written by its full-K GEMM straight into the rank's registered all-reduce buffer.
 * allreduce.hip fills the target (slot layout of the NEXT <= 64-row call of the context), gemm.hip's mi355_linear_publish_img passes it to gemm_fullk64.hip. */
typedef struct {
    const uint32_t* epoch;                /* device: per-block call counters of the context */
    void*    data;                        /* this rank's registered buffer */
    uint32_t bytes, parity_elems, slot_elems;
    int32_t  plain_stores;                /* full-fence hand-over: plain stores (the all-reduce launch's release fence publishes them) */
} mi355_publish_target_t;
int mi355_allreduce_publish_target(mi355_allreduce_t* ar, int32_t T, int32_t H, mi355_publish_target_t* out);
int mi355_fullk64_publish_ok(const mi355_weight_t* w);    /* gemm.hip: mi355_linear_publish_img takes this linear (W4 g128 / per-channel W8, K <= 5760; up to 9600 when its tile pairs leave half the chip free) */
int mi355_argmax_candidates(const float* logits, int32_t B, int32_t V, int32_t ld, void* workspace, size_t workspace_bytes,
                            mi355_stream_t stream);
int mi355_argmax_pairs(const float* logits, int32_t B, int32_t V, int32_t ld, int32_t vocab_offset, void* pairs_out,
                       void* workspace, size_t workspace_bytes, mi355_stream_t stream);
int mi355_argmax_pick(const void* pairs_all, int32_t world, int32_t B, int32_t* ids, int32_t* positions, mi355_stream_t stream);
/* sample_fused.hip: mi355_sample_logits drawing at draw_positions[r] + position_add, and the feedback launch of a sampled step
 * (positions + 1, ids appended to the history while it has room; history / history_len may be NULL) */
int mi355_sample_logits_ex(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature, const int32_t* top_k,
                           const float* top_p, const float* uniform_samples, const uint64_t* seed, const int32_t* draw_positions,
                           int32_t position_add, int32_t* ids, float* uniform_out, float* probs_out, int32_t ld_out, void* workspace,
                           size_t workspace_bytes, mi355_stream_t stream);
int mi355_sample_feedback(const int32_t* ids, int32_t B, int32_t* positions, int32_t* history, int32_t* history_len,
                          int32_t history_ld, mi355_stream_t stream);
/* logprobs.hip: the two launches of mi355_logprobs one by one (the step driver runs and profiles them as two ops).  _rows also takes the
 * recorder of mi355_decoder_set_logprobs: with count != NULL row r writes column count[r] of token_logprobs [rows][log_ld] and of
 * top_ids / top_logprobs [rows][log_ld][top_ld] while count[r] < log_ld and then advances it; cum_log_probs[r] (nullable) += the
 * token's value either way.  count == NULL, log_ld = 1: the public op. */
int mi355_logprobs_segments(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature, int32_t top_n,
                            void* workspace, size_t workspace_bytes, mi355_stream_t stream);
int mi355_logprobs_rows(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature, const int32_t* ids,
                        int32_t top_n, float* token_logprobs, float* lse_out, int32_t* top_ids, float* top_logprobs, int32_t top_ld,
                        int32_t log_ld, int32_t* count, float* cum_log_probs, void* workspace, size_t workspace_bytes,
                        mi355_stream_t stream);
/* allreduce.hip: mi355_allgather_logits launch by launch (the step driver runs and counts each as one MI355_KC_COMM op), the rank of a
 * context, and the reorder behind an external transport's all_gather of the logits: [world][B][V] -> [B][world * V] */
int mi355_allgather_logits_launches(mi355_allreduce_t* ar, int32_t B, int32_t V_local);
int mi355_allgather_logits_part(mi355_allreduce_t* ar, const float* local, int32_t ld, float* out, int32_t B, int32_t V_local, int32_t part,
                                mi355_stream_t stream);
int mi355_allreduce_rank(const mi355_allreduce_t* ar);
int mi355_interleave_logits(const float* staged, float* out, int32_t world, int32_t B, int32_t V, mi355_stream_t stream);
#ifdef __cplusplus
}
#endif
