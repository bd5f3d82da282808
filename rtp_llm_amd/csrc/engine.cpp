// Decode-step driver: enqueues one whole decode step of a Qwen2/Llama-style decoder
// from C++ and replays it as a hipGraph.
//
// Scope: the body of Qwen3Model.forward / Qwen3DecoderLayer.forward
// (rtp_llm/models_py/model_desc/qwen3.py:57-79,124-138), CausalAttention.forward
// (modules/hybrid/causal_attention.py:75-93), DenseMLP.forward
// (modules/hybrid/dense_mlp.py:95-106), lm_head + greedy
// (rtp_llm/cpp/models/PyWrappedModel.cc:938-1080, bindings/core/CudaSampleOp.cc:687-700)
// and the per-batch-size graph capture of rtp_llm/cpp/cuda_graph/cuda_graph_runner.cc.
//
// Launch table.  Rows: configuration classes; columns: the stages of one layer; cells: the entry point (mi355_ dropped, " = as above).  plan_launches decides once
// which classes the config and the weights allow (LaunchCaps), resolve_step picks one selector per stage for a step (StepPlan): a new launch variant is a new
// cell here, a selector value there and one case in its stage's switch.  A published O or down shard falls back to its slab cell on its own (K too deep).
//   class                                                 | QKV                                           | O                                   | gate_up                  | down                                | partial sums + residual + next norm
//   tp 1, <= fuse_rows (W4, fp16 step: gemm_fullk.hip)    | qkv_rope_kv_write [norm on load from layer 1] | linear_residual [+ sums of squares] | norm_linear              | linear_residual [+ sums of squares] | in the epilogues (rmsnorm launch: no fused norm; the final norm)
//   tp 1, > fuse_rows: images (fullk64 / wide / splitk64) | qkv_rope_kv_write_img                         | linear_residual_prenorm_img         | linear_deferred_norm_img | linear_partial_img (4 K quarters)   | add_rmsnorm_img_touch (final norm: add_rmsnorm)
//     ... opt-in (set_qkv_slab_rows): q_len 1, native cache| linear_partial_img (slabs -> attention)       | "                                   | "                        | "                                   | "
//     ... gate_up / down without their image launch       | "                                             | linear_residual_img + rmsnorm       | linear_direct            | linear_partial                      | "
//     ... INT8 cache, Qwen3 QK norm                       | linear_partial + rope_kv_write_rows[_qk_norm] | "                                   | "                        | "                                   | add_rmsnorm
//   other formats: staged split-K                         | linear_partial + rope_kv_write_rows           | linear_partial                      | linear_direct            | linear_partial                      | add_rmsnorm
//   TP attached, > tp_fuse_rows, published                | qkv_rope_kv_write_img                         | linear_publish_img                  | linear_direct_img        | linear_publish_img                  | allreduce_fused_published
//   TP attached, > tp_fuse_rows, slabs                    | qkv_rope_kv_write_img                         | linear_partial                      | linear_direct[_img]      | linear_partial_img                  | allreduce_fused_img
//   TP attached, <= tp_fuse_rows                          | qkv_rope_kv_write, or as staged               | linear_partial                      | linear_direct            | linear_partial                      | allreduce_fused
//   TP, external transport / segment caller               | "                                             | linear_partial                      | linear_direct            | linear_partial                      | add_rmsnorm (fold -> ar_buf) + all-reduce; add_rmsnorm opens the next segment
// Between QKV and O: paged_attn_rows (+ partition reduce), as paged_attn_rows_img where the O launch reads an image; behind the slab row of QKV
// paged_attn_qkv_slabs_img, whose prologue folds the slabs, adds the bias, rotates and writes the new token's k / v (no q tensor, no writer launch).  Activations are handed over row-major
// or as fragment-ordered images (common.h act_img_index); no standalone reduce / add / activation kernels.  The KV block layout (mi355_decoder_set_kv_layout)
// is not a column: every cell that touches a cache takes it through kv_of, which carries the layout -- the same launches, other addresses.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <string.h>
#include <map>
#include <new>
#include <vector>
#include "internal.h"
#ifdef MI355_TUNING
extern int g_tune[16];   // gemm.hip: experiment switches of the tuning build
#define TUNE(i) g_tune[i]
#else
#define TUNE(i) 0
#endif

void mi355_set_error(const char* fmt, ...);

namespace {
constexpr int kMaxSplits = 16;
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int    imax(int a, int b) { return a > b ? a : b; }
inline int    ssq_pitch(const mi355_model_config_t& c) { return (c.hidden / 16 + 3) & ~3; }   // row pitch of the per-tile sums of squares: hidden / 16 rounded up to 4
inline size_t weight_bytes(const mi355_weight_t* w) { return (size_t)w->K_pad * w->N_pad * w->wbits / 8; }
} // namespace

// What the config and the weight formats allow, decided once (plan_launches).  Each field is documented where it is computed.
struct LaunchCaps {
    bool fuse_qkv, fuse_o, fuse_down, fuse_norm;   // few-row full-K launches with their consumer fused (gemm_fullk.hip)
    bool img_qkv, img_o, img_gate_up, img_down;    // tp = 1: launches on activation images (gemm_fullk64 / gemm_wide / gemm_splitk64.hip)
    bool slab_qkv, slab_qkv_img;                   // tp = 1: QKV as split-K slabs folded in the attention launch's prologue; ... produced from the image (else from row-major xn)
    int  slab_rows;                                // ... from this many rows of a q_len = 1 step
    bool tp_img_qkv, tp_img_down, tp_img_gate;     // the same launches for the shards of a TP step with the all-reduce context attached
    bool tp_pub_o, tp_pub_down;                    // row-parallel shards published straight into the registered all-reduce buffer
    int  fuse_rows, tp_fuse_rows;                  // up to this many rows the (TP) step keeps the few-row launches
};
// The launch chain of ONE step: one selector per stage, resolved in mi355_decoder_begin_rows (resolve_step) and read by every launch
// site.  Each activation hand-over has one layout flag, derived from its CONSUMER's selector; producer and consumer both read it.
enum class QkvSel  { IMG, FULLK, SPLITK, ATTN_SLABS };
enum class OSel    { PUBLISH, IMG_PRENORM, IMG, FULLK, SPLITK };
enum class GateSel { DEFERRED_NORM_IMG, NORM_ON_LOAD, DIRECT_IMG, DIRECT };
enum class DownSel { FULLK, PUBLISH, QUARTERS, SPLITK };
enum class MeetSel { LOCAL, FUSED_AR, EXT };   // where partial sums, residual and norm meet: tp = 1 | attached context | local fold + external all-reduce
struct StepPlan {
    QkvSel qkv; OSel o; GateSel gate_up; DownSel down; MeetSel meet;
    bool xn_is_image;        // normed hidden rows into QKV: xn_img, else xn
    bool attn_is_image;      // attention output into O: attn_img, else attn_out
    bool gate_in_is_image;   // (pre-)normed rows into gate_up: xg_img, else xn
    bool act_is_image;       // SiLU-gated rows into down: act_img, else act
    bool resid_ssq;          // no norm launches: O / down leave the per-tile sums of squares (ssq), QKV / gate_up normalise resid on load
};

struct mi355_decoder {
    mi355_model_config_t               cfg;
    std::vector<mi355_layer_weights_t> layers;
    mi355_model_weights_t              model;
    mi355_step_buffers_t               bufs;
    // carved workspace
    void *resid, *xn, *q_buf, *attn_out, *act, *attn_ws, *argmax_ws;
    // activation images (mi355_act_image_*), see StepPlan: the normed hidden rows, the attention output, gate_up's input (gamma 2^-e h' where
    // the norm is deferred), the SiLU-gated rows
    void *xn_img, *attn_img, *xg_img, *act_img;
    int32_t* oob_count; // tokens refused by the KV writer (stale position / block id)
    const float* prefill_cos_sin = nullptr;   // mi355_decoder_set_prefill_rope_table: {cos, sin} rows of the NEXT prefill chunks (dynamic-NTK prompts past the original context), or null
    mi355_allreduce_t* ar; // attached all-reduce context (tp_size > 1): the TP step runs entirely from C++
    int    vocab_offset;
    // external transport (RCCL) for the same points when the peer mapping is not available: local fold -> fp16 ar_buf ->
    // in-place all-reduce -> residual + norm launch; greedy = all-gather of one (max, global index) pair per row
    mi355_collective_t ext;
    bool   has_ext;
    void  *pairs_local, *pairs_all;
    bool   embed_split;   // the embedding table holds this rank's hidden / tp columns: lookup + all-gather (embedding.py:50-58)
    // comm / weight-stream overlap: while the (latency-bound, <= 64 blocks) all-reduce kernel runs on the main stream, a
    // side stream pulls the NEXT GEMM's weight shard into the Infinity Cache
    hipStream_t side_stream;
    hipEvent_t  ev_fork, ev_join;
    bool        overlap;
    // weight prefetch one launch ahead (all tp): while a latency- or issue-bound launch runs on the main stream, a side stream
    // streams the weights of a LATER linear into the Infinity Cache (256 MB, memory side); the linear then starts from cache
    // instead of paying the first-byte latency of HBM under its own launch burst.  pf_mask: MI355_PF_* bits.
    int         pf_mask;
    bool        pf_pending;
    float* partials;
    size_t attn_ws_bytes, argmax_ws_bytes, partials_bytes;
    void*    wide_ws;        // max_batch > 64: buffers of the generic large-batch step (mi355_decoder_prefill with q_len = 1)
    size_t   wide_ws_bytes;
    int32_t* iota;           // [max_batch] 0, 1, 2, ...: "logits of every row"
    int    B;       // rows of the step in flight (= sequences * q_len)
    int    q_len;   // rows per sequence: 1 = decode, > 1 = target-verify / prefill chunk (causal over the paged cache)
    LaunchCaps caps;   // plan_launches
    StepPlan   plan;   // of the step in flight, like B and q_len
    std::vector<int> post_norm_exp;   // per layer: e >= log2(max |post_norm weight|) of the deferred norm
    // per-tile sums of h^2 a producer GEMM leaves for the next GEMM's on-the-fly RMSNorm, [rows][ssq_pitch]: 16 rows (few-row launches), 64 (images)
    float *ssq, *ssq64;
    // Qwen3 (mi355_decoder_set_qk_norm): per-layer [hd] weights of the per-head Q / K RMSNorm, empty for Qwen2 / Llama.  Set, the QKV
    // half of every layer is split-K + mi355_rope_kv_write_rows_qk_norm: plan_launches takes the fused QKV launches away
    std::vector<const void*> q_norm, k_norm;
    int    kv_layout; // MI355_KV_LAYOUT_* of every layer's cache (mi355_decoder_set_kv_layout); native unless set
    bool   started;   // a step, prefill or capture has been enqueued: the launch plan is fixed
    // sampled decoding (mi355_decoder_set_sampling): the tail of a decode step samples instead of taking the arg-max
    bool             sampling_on;
    mi355_sampling_t sampling;
    int32_t*         penalty_ws;   // carved from sampling.workspace: [max_batch][vocab] counts (with penalties), then the fused op's workspace
    void*            sample_ws;
    size_t           sample_ws_bytes;
    // log-probabilities of the chosen tokens (mi355_decoder_set_logprobs): two more launches behind the choice, recorded per slot
    bool             logprobs_on;
    mi355_logprobs_t logprobs;
    // tp_size > 1 (mi355_decoder_set_gathered_logits): the vocabulary-gathered fp32 rows [max_batch][tp_size * vocab] the sampled tail and the
    // log-probability recorder run on, then the staging [tp_size][max_batch][vocab] of an external transport's all_gather; null = off
    float*           gathered;
    float*           gather_stage;
    // graphs
    hipStream_t                    cap_stream;
    std::map<int, hipGraphExec_t>  graphs;
    // profiling
    bool                     prof_on;
    std::vector<hipEvent_t>  ev;
    std::vector<int>         ev_class;
    size_t                   ev_used;
};

namespace {

struct Carve {
    char*  base;
    size_t off;
    void*  take(size_t bytes) {
        void* p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    }
};

struct PrefillBufs;
size_t carve_prefill(const mi355_model_config_t& c, int T, int nseq, void* base, PrefillBufs* out);

size_t carve_all(mi355_decoder* d, const mi355_model_config_t& c, void* base) {
    Carve cv{(char*)base, 0};
    const size_t MB_ = (size_t)(c.max_batch < 64 ? c.max_batch : 64);   // the fused small-batch path handles <= 64 rows per step
    const int qdim = c.nh * c.hd, qkvdim = (c.nh + 2 * c.nkv) * c.hd;
    const int npad = (imax(qkvdim, c.hidden) + 15) & ~15;
    void* resid    = cv.take(MB_ * c.hidden * 2);
    void* xn       = cv.take(MB_ * c.hidden * 2);
    void* q_buf    = cv.take(MB_ * qdim * 2);
    void* attn_out = cv.take(MB_ * qdim * 2);
    void* act      = cv.take(MB_ * c.inter * 2);
    // split-K slabs: qkv / o / down use up to kMaxSplits of [max_batch, npad]; a K-split gate_up (TP shards) up to 4 of [max_batch, 2 inter]
    const size_t pbytes = std::max((size_t)kMaxSplits * MB_ * npad * 4, (size_t)4 * MB_ * ((2 * c.inter + 15) & ~15) * 4);
    void* partials = cv.take(pbytes);
    const size_t aw = mi355_paged_attn_workspace_bytes((int)MB_, c.nh, c.hd, c.max_seq_len);
    void* attn_ws  = cv.take(aw);
    const size_t gw = (size_t)c.max_batch * 64 * 8;
    void* argmax_ws = cv.take(gw);
    void* oob = cv.take(256);
    void* ssq = cv.take((size_t)16 * ssq_pitch(c) * 4);   // per-tile sums of squares of the residual rows (fused norm, <= 16 rows)
    void* xn_img = cv.take(mi355_act_image_bytes(64, c.hidden));
    void* xg_img = cv.take(mi355_act_image_bytes(64, c.hidden));
    void* act_img = cv.take(mi355_act_image_bytes(64, c.inter));
    void* ssq64 = cv.take((size_t)64 * ssq_pitch(c) * 4);
    void* attn_img = cv.take(mi355_act_image_bytes(64, qdim));
    const size_t wide_bytes = c.max_batch > 64 ? carve_prefill(c, c.max_batch, c.max_batch, nullptr, nullptr) : 0;
    void* wide_ws = cv.take(wide_bytes);
    void* iota = cv.take((size_t)c.max_batch * 4);
    if (d) {
        d->ssq = (float*)ssq; d->xn_img = xn_img; d->attn_img = attn_img; d->xg_img = xg_img; d->ssq64 = (float*)ssq64; d->act_img = act_img;
        d->oob_count = (int32_t*)oob; d->wide_ws = wide_ws; d->wide_ws_bytes = wide_bytes; d->iota = (int32_t*)iota;
        d->resid = resid; d->xn = xn; d->q_buf = q_buf; d->attn_out = attn_out; d->act = act;
        d->partials = (float*)partials; d->partials_bytes = pbytes; d->attn_ws = attn_ws; d->attn_ws_bytes = aw;
        d->argmax_ws = argmax_ws; d->argmax_ws_bytes = gw;
    }
    return cv.off;
}

// run one op, optionally bracketed by events for the per-class profile
template <class F>
int run_op(mi355_decoder* d, int kclass, hipStream_t st, F&& f) {
    if (!d->prof_on) return f();
    if (d->ev_used + 2 > d->ev.size()) {
        for (int i = 0; i < 2; ++i) { hipEvent_t e; hipEventCreate(&e); d->ev.push_back(e); }
    }
    hipEventRecord(d->ev[d->ev_used], st);
    const int rc = f();
    hipEventRecord(d->ev[d->ev_used + 1], st);
    d->ev_class.push_back(kclass);
    d->ev_used += 2;
    return rc;
}

#define ADT (d->cfg.act_dtype)   /* activation dtype of every norm call below */
#define RUN(kclass, expr)                                                  \
    do {                                                                   \
        int rc__ = run_op(d, kclass, st, [&]() -> int { return (expr); }); \
        if (rc__ < 0) return rc__;                                         \
    } while (0)

mi355_kv_layer_t kv_of(const mi355_decoder* d, int l) {
    mi355_kv_layer_t kv;
    kv.kv_base = d->layers[l].kv_base; kv.scale_base = d->layers[l].kv_scale_base;
    kv.kv_dtype = d->cfg.kv_dtype; kv.page = d->cfg.page; kv.nkv = d->cfg.nkv; kv.hd = d->cfg.hd;
    kv.num_blocks = d->cfg.num_blocks;
    kv.act_dtype = d->cfg.act_dtype;
    kv.layout = d->kv_layout;
    return kv;
}

} // namespace

extern "C" size_t mi355_decoder_workspace_bytes(const mi355_model_config_t* cfg) {
    if (!cfg) return 0;
    return carve_all(nullptr, *cfg, nullptr);
}

namespace {
// Which launches serve which step heights (LaunchCaps), decided from the config and the weight formats in mi355_decoder_create and again
// when mi355_decoder_set_qk_norm takes the fused QKV launches away.  The result is the mix an INT8-KV config runs: composed QKV reading
// xn, image O / gate_up / down above fuse_rows.
int plan_launches(mi355_decoder* d) {
    const mi355_model_config_t& c = d->cfg;
    LaunchCaps& k = d->caps;
    const bool bf_act = c.act_dtype == MI355_ACT_BF16, tp = c.tp_size > 1;
    // QKV + bias + RoPE + KV write in one launch: a 16-bit cache of the activation dtype (INT8 caches keep the quantising writer of rope_kv.hip),
    // not with the per-head QK norm of Qwen3 (a fused QKV launch's block / epilogue job owns 32 of a head's hd columns, the norm needs the whole head)
    const bool qkv_fusable = c.kv_dtype == (bf_act ? MI355_KV_BF16 : MI355_KV_FP16) && c.rope_dim == c.hd && d->q_norm.empty();
    // few-row full-K launches (gemm_fullk.hip): QKV as above, O / down projection + residual add without split-K slabs (tp = 1: under TP the partial
    // sums of the row-parallel linears meet in the all-reduce first).  Only up to fuse_rows rows: every block reads ALL activation rows of its K range
    // from L2, which is free at a few rows and 2x slower than the staged split-K kernels at 64 (measured M = 64: qkv+rope 20.8 vs 9.0 + 4.9 us,
    // o 18.6 vs 9.7 + slab fold; M = 1: 6.8 vs 7.3 + 3.1 us).  W4 layers only: for small fp16 models (the 0.5B draft of speculative decoding: 36-56
    // blocks per launch) the fused launches measured behind the staged kernels (draft step 1.11 vs 1.05 ms), although the kernels take fp16 weights
    auto w4ok = [](const mi355_weight_t* w) { return w->wbits == 4 && mi355_fullk_weight_ok(w); };
    k.fuse_qkv = qkv_fusable; k.fuse_o = k.fuse_down = !tp;
    // the norm launches disappear as well when every GEMM of the few-row layer is a full-K launch: O / down leave the per-tile sums of squares of
    // the new residual rows, QKV / gate_up rebuild 1 / rms from them and normalise on load
    bool gate_w4 = c.hidden % 64 == 0;
    for (const auto& L : d->layers) {
        k.fuse_qkv = k.fuse_qkv && w4ok(&L.qkv); k.fuse_o = k.fuse_o && w4ok(&L.o); k.fuse_down = k.fuse_down && w4ok(&L.down);
        gate_w4 = gate_w4 && w4ok(&L.gate_up);
    }
    k.fuse_norm = k.fuse_qkv && k.fuse_o && k.fuse_down && gate_w4;
    // tp = 1, 1-64 rows: QKV + bias + RoPE + KV write and O + residual as one full-K launch each on activation images handed over by the producing
    // launches (gemm_fullk64.hip: W4 group-wise or per-channel W8, K <= 5760; either activation dtype: the images are fp16, the epilogues store the
    // step's dtype).  TUNE(5) == 2: A/B against the split-K + fold launches
    k.img_qkv = qkv_fusable && !tp && TUNE(5) != 2;
    k.img_o = !tp && TUNE(5) != 2;
    for (const auto& L : d->layers) {   // the launchers' own predicate (gemm.hip)
        k.img_qkv = k.img_qkv && mi355_fullk64_weight_ok(&L.qkv) != 0; k.img_o = k.img_o && mi355_fullk64_weight_ok(&L.o) != 0;
    }
    // QKV as a plain split-K launch whose slabs the attention launch folds itself (bias, RoPE, KV write in its prologue: attention.hip, QS): what
    // the fused launch is fusable for, with the attention output as an image.  The slabs come from the image (gemm_splitk64.hip) where that launch has a
    // plan for the shape, else from the staged kernel on row-major rows (narrow models: K too short for eight K slices per block)
    k.slab_qkv = k.img_qkv && k.img_o;
    k.slab_qkv_img = k.slab_qkv;
    for (const auto& L : d->layers)
        k.slab_qkv_img = k.slab_qkv_img && L.qkv.K % 128 == 0 && L.qkv.K_pad == L.qkv.K &&
                         mi355_gemm_splitk64_plan(64, L.qkv.N_pad / 16, L.qkv.K_pad / 128, mi355_wfmt(&L.qkv), L.qkv.group_size, kMaxSplits, nullptr) > 0;
    // ... the post-attention RMSNorm deferred into gate_up's accumulators (mi355_deferred_norm_t): the O launch leaves gamma 2^-e h' as an image + the
    // per-tile sums of h'^2, the wide GEMM applies rsqrt(mean h'^2 + eps) 2^e: 6 launches per layer
    k.img_gate_up = k.img_o && c.hidden % 64 == 0 && TUNE(5) != 3;
    for (const auto& L : d->layers) k.img_gate_up = k.img_gate_up && mi355_gemm_wide_direct_ok(&L.gate_up);
    // ... and down_proj as 4 K-quarters from the image gate_up's SiLU epilogue writes (gemm_splitk64.hip) instead of 15 slabs
    auto quarters_ok = [](const mi355_weight_t& w) {
        return w.K % 128 == 0 && w.K_pad == w.K && mi355_gemm_splitk64_plan(64, w.N_pad / 16, w.K_pad / 128, mi355_wfmt(&w), w.group_size, kMaxSplits, nullptr) > 0;
    };
    k.img_down = k.img_gate_up && c.inter % 32 == 0 && TUNE(5) != 4;
    for (const auto& L : d->layers) k.img_down = k.img_down && quarters_ok(L.down);
    // bf16: the wide GEMM's image entry only exists with an image OUTPUT (gemm.hip mi355_linear_deferred_norm_img): without the
    // K-quarter down launch that reads it, gate_up goes back to norm launch + staged kernel instead of failing every step
    if (bf_act && !k.img_down) k.img_gate_up = false;
    // tensor parallelism with the in-step all-reduce attached: the column-parallel QKV shard runs as the same image launch -- the fused all-reduce
    // behind down_proj (and the first norm of the step) write the image it reads
    k.tp_img_qkv = tp && qkv_fusable && c.hidden % 32 == 0 && c.max_batch >= 1 && TUNE(5) != 2;
    for (const auto& L : d->layers) k.tp_img_qkv = k.tp_img_qkv && mi355_fullk64_qkv_ok(&L.qkv, c.hd) != 0;
    // ... the row-parallel down_proj shard as K quarters from the image the gate_up shard's SiLU epilogue writes: 2-4 slabs into the fused all-reduce
    // launch instead of up to 15
    k.tp_img_down = tp && c.inter % 32 == 0 && TUNE(5) != 4 && TUNE(5) != 2;
    for (const auto& L : d->layers) k.tp_img_down = k.tp_img_down && quarters_ok(L.down) && L.down.K == c.inter && L.gate_up.N == 2 * c.inter;
    // ... and the column-parallel gate_up shard as ONE launch from an image (gemm_splitk64.hip, direct form) instead of the staged split-K kernel +
    // fold: the fused all-reduce behind the O shard then writes its normed rows as that image (into xg_img: unused under TP otherwise)
    k.tp_img_gate = k.tp_img_down && c.hidden % 32 == 0 && TUNE(5) != 3;
    for (const auto& L : d->layers)
        k.tp_img_gate = k.tp_img_gate && L.gate_up.K % 128 == 0 && L.gate_up.K_pad == L.gate_up.K &&
                        mi355_gemm_splitk64_direct_plan(64, L.gate_up.N_pad / 16, L.gate_up.K_pad / 128, mi355_wfmt(&L.gate_up), L.gate_up.group_size) > 0;
    // the row-parallel O / down shards as ONE full-K launch each whose epilogue writes the rank's rows straight into the registered all-reduce buffer
    // (mi355_linear_publish_img), consumed by mi355_allreduce_fused_published_dt: no slabs, no fold + publish stage in front of the flag exchange
    k.tp_pub_o = k.tp_img_qkv && !(TUNE(8) & 1);
    k.tp_pub_down = k.tp_img_down && !(TUNE(8) & 2);
    for (const auto& L : d->layers) {
        k.tp_pub_o = k.tp_pub_o && mi355_fullk64_publish_ok(&L.o) != 0;
        // down: where K stays inside two or three chunks per wave (K <= 5760: tp 4 of Qwen2-7B, tp 8 of the 70B models); deeper shards keep the K quarters
        k.tp_pub_down = k.tp_pub_down && mi355_fullk64_publish_ok(&L.down) != 0 && (L.down.K_pad / 128 <= 45 || (TUNE(8) & 4));
    }
    // fuse_rows: crossover between the few-row full-K launches (dense activation loads) and the launches on activation images (same box: b = 4 1.94 vs
    // 2.05 ms, b = 5 2.16 vs 2.05, b = 8 2.28 vs 2.07, b = 12 2.64 vs 2.10; profiles/r04_batch_sweep_crossover.txt).  bf16 / W8 have no few-row launches
    // to cross over to (gemm_fullk.hip takes fp16 steps of W4 / fp16 weights; the staged kernels lose at every height): the image launches serve 1-64
    // rows.  Without the image path (other weight formats, TP) the earlier crossover to the staged kernels stays: 12
    k.fuse_rows = !(k.img_qkv && k.img_o) ? 12 : (bf_act || !(k.fuse_qkv && k.fuse_o && k.fuse_down)) ? 0 : 4;
    if (TUNE(6) > 0) k.fuse_rows = TUNE(6) == 99 ? 0 : TUNE(6);   // tuning build: crossover experiments (tools/batch_sweep.py --tune 6=N)
    // slab_rows: from how many rows the decode step takes the slab row of the table; 0 = never, the default.  The path sums K in another order (3 slabs of
    // 8 wave slices instead of 14 slices) and adds the new token to the softmax last, so its logits differ from the fused launch's in the last bits -- and a
    // greedy decode of many steps amplifies a last bit into other tokens.  A caller opts in with mi355_decoder_set_qkv_slab_rows; DESIGN 9 D has what it measured.
    k.slab_rows = 0;
    // tp_fuse_rows: from how many rows the TP step takes the image launches.  With the down shard as K quarters they win from ONE row (one rank of tp 2,
    // b = 1 / 2 / 4: 1.67 / 1.68 / 1.72 ms against 1.75 / 1.77 / 1.82 with the few-row QKV launch + 15 staged slabs;
    // profiles/r05_tp_small_batch_crossover.txt); without that plan the few-row QKV launch (row-major input) keeps its rows (the tp = 1 crossover)
    k.tp_fuse_rows = (bf_act || !k.fuse_qkv || k.tp_img_down) ? 0 : 4;
    if (TUNE(6) > 0) k.tp_fuse_rows = TUNE(6) == 99 ? 0 : TUNE(6);   // tuning build: the same switch
    d->post_norm_exp.clear();
    if (k.img_gate_up) {   // exponent of the deferred norm per layer: the largest |weight| of post_norm, read back once
        std::vector<uint16_t> g(c.hidden);
        for (const auto& L : d->layers) {
            if (hipMemcpy(g.data(), L.post_norm, (size_t)c.hidden * 2, hipMemcpyDeviceToHost) != hipSuccess) {
                mi355_set_error("decoder: cannot read the norm weights"); return MI355_ERR_HIP;
            }
            float mx = 0.f;
            for (uint16_t b : g) {   // 16-bit pattern -> |value|
                float v;
                if (bf_act) { const uint32_t u = (uint32_t)(b & 0x7FFF) << 16; memcpy(&v, &u, 4); if (!(v == v)) v = INFINITY; }
                else {
                    const int e = (b >> 10) & 31, m = b & 1023;
                    v = e == 0 ? ldexpf((float)m, -24) : (e == 31 ? INFINITY : ldexpf((float)(m | 1024), e - 25));
                }
                if (v > mx) mx = v;
            }
            int ex = 0;
            while (ex < 14 && ldexpf(1.f, ex) < mx) ++ex;
            if (!(mx < INFINITY) || ldexpf(1.f, ex) < mx) { k.img_gate_up = false; break; }   // inf / nan / beyond 2^14 in a norm weight: keep the norm launch
            // a bf16 residual stream may exceed the fp16 range of the image: eight more binary orders of headroom (|h| < 1.6e7), paid for with
            // precision only on elements below 2^-6 of a typical one
            d->post_norm_exp.push_back(bf_act ? (ex + 8 > 14 ? 14 : ex + 8) : ex);
        }
    }
    return MI355_OK;
}
} // namespace

extern "C" mi355_decoder_t* mi355_decoder_create(const mi355_model_config_t* cfg, const mi355_layer_weights_t* layers,
                                                 const mi355_model_weights_t* model, const mi355_step_buffers_t* bufs) {
    if (!cfg || !layers || !model || !bufs) { mi355_set_error("decoder_create: null argument"); return nullptr; }
    if (cfg->num_layers <= 0 || cfg->max_batch <= 0 || cfg->max_batch > 4096) {
        mi355_set_error("decoder_create: num_layers=%d max_batch=%d (1..4096)", cfg->num_layers, cfg->max_batch);
        return nullptr;
    }
    if (cfg->nh % cfg->nkv != 0 || cfg->nh / cfg->nkv > 16 || (cfg->hd != 64 && cfg->hd != 128)) {
        mi355_set_error("decoder_create: nh=%d nkv=%d hd=%d unsupported", cfg->nh, cfg->nkv, cfg->hd);
        return nullptr;
    }
    if (cfg->max_seq_len <= 0 || cfg->max_seq_len > cfg->max_pos || cfg->page <= 0 ||
        (long)cfg->max_blocks_per_seq * cfg->page < cfg->max_seq_len || cfg->num_blocks <= 0) {
        mi355_set_error("decoder_create: max_seq_len=%d must be <= max_pos=%d (rotation table) and <= max_blocks_per_seq*page=%ld",
                        cfg->max_seq_len, cfg->max_pos, (long)cfg->max_blocks_per_seq * cfg->page);
        return nullptr;
    }
    {   // activation dtype: one for the whole step
        const bool bf = cfg->act_dtype == MI355_ACT_BF16;
        bool ok = (cfg->act_dtype == MI355_ACT_F16 || bf) && (cfg->kv_dtype == MI355_KV_INT8 || bf == (cfg->kv_dtype == MI355_KV_BF16));
        auto lin_ok = [&](const mi355_weight_t& w) { return w.act_dtype == cfg->act_dtype; };
        ok = ok && lin_ok(model->lm_head);
        for (int l = 0; ok && l < cfg->num_layers; ++l)
            ok = lin_ok(layers[l].qkv) && lin_ok(layers[l].o) && lin_ok(layers[l].gate_up) && lin_ok(layers[l].down);
        if (!ok) {
            mi355_set_error("decoder_create: act_dtype=%d needs every linear in that dtype%s and a %s KV cache", cfg->act_dtype,
                            "", bf ? "bf16 or INT8" : "fp16 or INT8");
            return nullptr;
        }
    }
    const size_t need = carve_all(nullptr, *cfg, nullptr);
    if (!bufs->workspace || bufs->workspace_bytes < need) {
        mi355_set_error("decoder_create: workspace %zu < %zu", bufs->workspace_bytes, need);
        return nullptr;
    }
    if (!bufs->token_ids || !bufs->positions || !bufs->block_table || !bufs->logits || !bufs->hidden ||
        (cfg->tp_size > 1 && !bufs->ar_buf)) {
        mi355_set_error("decoder_create: missing step buffer");
        return nullptr;
    }
    mi355_decoder* d = new (std::nothrow) mi355_decoder();
    if (!d) return nullptr;
    d->cfg = *cfg; d->layers.assign(layers, layers + cfg->num_layers); d->model = *model; d->bufs = *bufs;
    carve_all(d, *cfg, bufs->workspace);
    d->xn = bufs->hidden; // the normed hidden state lives in the caller-visible buffer
    d->started = false;
    d->sampling_on = false; d->penalty_ws = nullptr; d->sample_ws = nullptr; d->sample_ws_bytes = 0;
    d->logprobs_on = false;
    d->gathered = nullptr; d->gather_stage = nullptr;
    d->kv_layout = MI355_KV_LAYOUT_NATIVE;
    d->B = 0; d->q_len = 1; d->cap_stream = nullptr; d->prof_on = false; d->ev_used = 0; d->ar = nullptr; d->vocab_offset = 0;
    d->has_ext = false; d->pairs_local = d->pairs_all = nullptr;
    d->side_stream = nullptr; d->ev_fork = d->ev_join = nullptr; d->overlap = false;
    d->pf_mask = MI355_PF_QKV_IN_FOLD; d->pf_pending = false;   // the one prefetch that needs no stream and measured positive (profiles/r04_touch_prefetch.txt)
    if (int e = plan_launches(d)) { delete d; return nullptr; }
    std::vector<int32_t> iota_h(cfg->max_batch);
    for (int i = 0; i < cfg->max_batch; ++i) iota_h[i] = i;
    if (hipMemset(d->oob_count, 0, 256) != hipSuccess ||
        hipMemcpy(d->iota, iota_h.data(), iota_h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        mi355_set_error("decoder_create: cannot initialise the workspace"); delete d; return nullptr;
    }
    return d;
}

namespace {
void drop_graphs(mi355_decoder* d) {   // captured steps bake the launch chain, the embedding path and the fork / join edges in
    for (auto& kv : d->graphs) hipGraphExecDestroy(kv.second);
    d->graphs.clear();
}
// the side stream and its two events: created once, ahead of any capture (not lazily inside one)
bool side_ready(mi355_decoder* d) {
    if (d->side_stream) return d->ev_fork && d->ev_join;
    const bool ok = hipStreamCreateWithFlags(&d->side_stream, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming) == hipSuccess;
    (void)hipGetLastError();
    return ok;
}
// in-place sum of `count` 16-bit values over the TP ranks through the attached transport (no-op without one: the segment caller
// all-reduces ar_buf itself between the calls)
int ext_all_reduce(mi355_decoder* d, void* buf, size_t count, hipStream_t st) {
    if (!d->has_ext) return MI355_OK;
    const int rc = (d->cfg.act_dtype == MI355_ACT_BF16 ? d->ext.all_reduce_bf16 : d->ext.all_reduce_f16)(d->ext.ctx, buf, count, (mi355_stream_t)st);
    if (rc != 0) { mi355_set_error("decoder: the attached transport's all-reduce failed (%d)", rc); return MI355_ERR_HIP; }
    return MI355_OK;
}

constexpr size_t kPfCap = (size_t)48 << 20;          // bytes of one linear a side-stream prefetch pulls at most
constexpr size_t kPfInLaunchCap = (size_t)8 << 20;   // MI355_PF_TP_INLAUNCH: bytes of the next shard one all-reduce launch requests (the
                                                     // peer reads of its reduction queue behind them: vmcnt returns in order)
// fork: from this point of `st` on, the side stream pulls up to kPfCap bytes of w into the Infinity Cache (plain event edges, so the
// pair is captured into the step graph like everything else)
int pf_fork(mi355_decoder* d, hipStream_t st, const mi355_weight_t* w) {
    if (hipEventRecord(d->ev_fork, st) != hipSuccess || hipStreamWaitEvent(d->side_stream, d->ev_fork, 0) != hipSuccess) {
        mi355_set_error("decoder: fork to the prefetch stream failed: %s", hipGetErrorString(hipGetLastError())); return MI355_ERR_HIP;
    }
    // the last dword of the oob block is never read by anyone: a harmless sink
    return mi355_prefetch(w->qweight, std::min(weight_bytes(w), kPfCap), d->oob_count + 32, d->side_stream);
}
// all-reduce on `st`, prefetch of the next GEMM's weights on the side stream, joined before the GEMM
template <class F>
int comm_with_prefetch(mi355_decoder* d, hipStream_t st, const mi355_weight_t* next_w, F&& comm) {
    const bool ov = d->overlap && (d->pf_mask & MI355_PF_TP_COMM) && next_w && next_w->qweight;
    if ((d->pf_mask & MI355_PF_TP_INLAUNCH) && d->ar && next_w && next_w->qweight) {
        // no second stream: the waves of the fused all-reduce launch that only wait for the peers' flags request the shard
        const int rc = mi355_allreduce_set_prefetch(d->ar, next_w->qweight, std::min(weight_bytes(next_w), kPfInLaunchCap));
        if (rc < 0) return rc;
    }
    if (ov) { const int rc = pf_fork(d, st, next_w); if (rc < 0) return rc; }
    const int rc = comm();
    if (rc < 0) return rc;
    if (ov && (hipEventRecord(d->ev_join, d->side_stream) != hipSuccess || hipStreamWaitEvent(st, d->ev_join, 0) != hipSuccess)) {
        mi355_set_error("decoder: join of the side stream failed: %s", hipGetErrorString(hipGetLastError())); return MI355_ERR_HIP;
    }
    return rc;
}
// tp = 1, weight prefetch one launch ahead: fork now, join (pf_join) in front of the linear that reads w
int pf_issue(mi355_decoder* d, hipStream_t st, const mi355_weight_t* w) {
    if (!w || !w->qweight || d->pf_pending || !side_ready(d)) return MI355_OK;
    const int rc = pf_fork(d, st, w);
    if (rc < 0) return rc;
    if (hipEventRecord(d->ev_join, d->side_stream) != hipSuccess) {
        mi355_set_error("decoder: prefetch stream event failed: %s", hipGetErrorString(hipGetLastError())); return MI355_ERR_HIP;
    }
    d->pf_pending = true;
    return MI355_OK;
}
// join: launches issued on `st` after this point wait for the prefetch in flight (it has normally long finished)
int pf_join(mi355_decoder* d, hipStream_t st) {
    if (!d->pf_pending) return MI355_OK;
    d->pf_pending = false;
    if (hipStreamWaitEvent(st, d->ev_join, 0) != hipSuccess) {
        mi355_set_error("decoder: join of the prefetch stream failed: %s", hipGetErrorString(hipGetLastError())); return MI355_ERR_HIP;
    }
    return MI355_OK;
}
#define PF_ISSUE(bits, w) do { if (pf & (bits)) if (int e__ = pf_issue(d, st, (w))) return e__; } while (0)

// does the attached context take published rows for a B-row call right now?  Host state of the context only (ready, not on the
// granule protocol, sizes): no caller changes that between begin and finish of a step, so one query per step
bool pub_ready(const mi355_decoder* d, int B) {
    mi355_publish_target_t t;
    return d->ar && mi355_allreduce_publish_target(d->ar, B, d->cfg.hidden, &t) == MI355_OK;
}

// The launch chain of a B-row step: the row of the table at the top of this file.  Consumers first; every layout flag follows from
// its consumer's selector and from nothing else.
int resolve_step(mi355_decoder* d, int B, int q_len) {
    const LaunchCaps& k = d->caps;
    StepPlan p;
    p.meet = d->cfg.tp_size == 1 ? MeetSel::LOCAL : d->ar ? MeetSel::FUSED_AR : MeetSel::EXT;
    const bool tp_mid = p.meet == MeetSel::FUSED_AR && B > k.tp_fuse_rows;   // TP step on the image launches (tp_img_* are tp > 1 only)
    const bool mid = B > k.fuse_rows;                                        // tp = 1 step on the image launches (img_* are tp = 1 only)
    const bool few = !(k.tp_img_qkv && tp_mid) && !mid;                      // the few-row full-K launches keep their rows
    const bool pub = tp_mid && (k.tp_pub_o || k.tp_pub_down) && pub_ready(d, B);
    const bool slabs = k.slab_qkv && k.slab_rows > 0 && mid && q_len == 1 && B >= k.slab_rows && d->kv_layout == MI355_KV_LAYOUT_NATIVE;
    p.qkv = slabs ? QkvSel::ATTN_SLABS : ((k.img_qkv && mid) || (k.tp_img_qkv && tp_mid)) ? QkvSel::IMG : (k.fuse_qkv && few) ? QkvSel::FULLK : QkvSel::SPLITK;
    p.resid_ssq = k.fuse_norm && few;
    p.gate_up = (k.img_o && k.img_gate_up && mid) ? GateSel::DEFERRED_NORM_IMG : p.resid_ssq ? GateSel::NORM_ON_LOAD
              : (k.tp_img_gate && tp_mid) ? GateSel::DIRECT_IMG : GateSel::DIRECT;
    p.o = (k.tp_pub_o && pub) ? OSel::PUBLISH
        : (k.img_o && mid) ? (p.gate_up == GateSel::DEFERRED_NORM_IMG ? OSel::IMG_PRENORM : OSel::IMG)
        : (k.fuse_o && few) ? OSel::FULLK : OSel::SPLITK;
    p.down = (k.fuse_down && few) ? DownSel::FULLK : (k.tp_pub_down && pub) ? DownSel::PUBLISH
           : ((p.gate_up == GateSel::DEFERRED_NORM_IMG && k.img_down) || (k.tp_img_down && tp_mid)) ? DownSel::QUARTERS : DownSel::SPLITK;
    p.xn_is_image = p.qkv == QkvSel::IMG || (p.qkv == QkvSel::ATTN_SLABS && k.slab_qkv_img);
    p.attn_is_image = p.o == OSel::PUBLISH || p.o == OSel::IMG_PRENORM || p.o == OSel::IMG;
    p.gate_in_is_image = p.gate_up == GateSel::DEFERRED_NORM_IMG || p.gate_up == GateSel::DIRECT_IMG;
    p.act_is_image = p.down == DownSel::PUBLISH || p.down == DownSel::QUARTERS;
    // can every producer write what its consumer reads?  plan_launches steps such configs down itself; this guards a planner change that forgets to
    const bool ar_tail = p.meet == MeetSel::FUSED_AR && (p.o == OSel::PUBLISH || p.o == OSel::SPLITK);   // the all-reduce launch writes either layout
    const char* bad =
        p.xn_is_image && p.meet == MeetSel::EXT ? "QKV on an image behind the external transport's row-major norm" :
        p.qkv == QkvSel::ATTN_SLABS && !(p.attn_is_image && p.meet == MeetSel::LOCAL && q_len == 1) ? "QKV slabs for the attention prologue without its image output, under TP or with q_len > 1" :
        p.resid_ssq && !(p.qkv == QkvSel::FULLK && p.o == OSel::FULLK && p.down == DownSel::FULLK) ? "norm on load without the full-K launches that leave the sums of squares" :
        (p.gate_up == GateSel::DEFERRED_NORM_IMG) != (p.o == OSel::IMG_PRENORM) ? "deferred norm in gate_up without the O launch that prepares it" :
        p.gate_up == GateSel::DIRECT_IMG && !ar_tail ? "gate_up on an image no launch writes" :
        p.act_is_image && p.gate_up == GateSel::NORM_ON_LOAD ? "down on an image behind a gate_up launch without image output" :
        !p.act_is_image && p.gate_up == GateSel::DEFERRED_NORM_IMG && d->cfg.act_dtype == MI355_ACT_BF16 ? "bf16: gate_up image entry only with an image output" : nullptr;
    if (bad) { mi355_set_error("decoder_begin: inconsistent launch plan for %d rows: %s", B, bad); return MI355_ERR_UNSUPPORTED; }
    d->plan = p;
    return MI355_OK;
}

// ---- where the partial sums of a row-parallel linear, the residual and the next RMSNorm meet (StepPlan::meet).  y: the normed rows, an image
// if y_image; next_w: the linear behind the norm (TP: its shard is prefetched under the exchange).  Here: ns fp32 slabs in d->partials
int meet_slabs(mi355_decoder* d, hipStream_t st, int ns, int n_pad, const void* norm_w, const mi355_weight_t* next_w, void* y, bool y_image,
               const mi355_touch_t* touch) {
    const auto& c = d->cfg; const int B = d->B;
    switch (d->plan.meet) {
    case MeetSel::LOCAL:
        if (y_image) RUN(MI355_KC_NORM, mi355_add_rmsnorm_img_touch(nullptr, d->partials, ns, n_pad, nullptr, d->resid, d->resid, norm_w, c.rms_eps, B, c.hidden, y, ADT, touch, st));
        else RUN(MI355_KC_NORM, mi355_add_rmsnorm_dt(nullptr, d->partials, ns, n_pad, nullptr, d->resid, d->resid, norm_w, c.rms_eps, B, c.hidden, y, ADT, st));
        break;
    case MeetSel::FUSED_AR:   // split-K reduce + all-reduce + residual + norm in one launch
        RUN(MI355_KC_COMM, comm_with_prefetch(d, st, next_w, [&]() {
            return (y_image ? mi355_allreduce_fused_img_dt : mi355_allreduce_fused_dt)(d->ar, nullptr, d->partials, ns, n_pad, nullptr, d->resid, d->resid,
                                                                                      norm_w, c.rms_eps, B, c.hidden, y, ADT, st); }));
        break;
    case MeetSel::EXT:        // local split-K reduce -> 16-bit tensor for the TP all-reduce; residual + norm open the next segment
        RUN(MI355_KC_NORM, mi355_add_rmsnorm_dt(nullptr, d->partials, ns, n_pad, nullptr, nullptr, d->bufs.ar_buf, nullptr, c.rms_eps, B, c.hidden, nullptr, ADT, st));
        RUN(MI355_KC_COMM, ext_all_reduce(d, d->bufs.ar_buf, (size_t)B * c.hidden, st));
        break;
    }
    return MI355_OK;
}
// the rank's rows already published in the all-reduce buffer (mi355_linear_publish_img): exchange + residual + norm
int meet_published(mi355_decoder* d, hipStream_t st, const void* norm_w, const mi355_weight_t* next_w, void* y, bool y_image) {
    RUN(MI355_KC_COMM, comm_with_prefetch(d, st, next_w, [&]() {
        return mi355_allreduce_fused_published_dt(d->ar, d->resid, d->resid, norm_w, d->cfg.rms_eps, d->B, d->cfg.hidden, y, y_image ? 1 : 0, ADT, st); }));
    return MI355_OK;
}
// external transport / segment caller: the all-reduced partial sums wait in ar_buf; residual + norm open the next segment
int meet_ext_tail(mi355_decoder* d, hipStream_t st, const void* norm_w) {
    RUN(MI355_KC_NORM, mi355_add_rmsnorm_dt(d->bufs.ar_buf, nullptr, 0, 0, nullptr, d->resid, d->resid, norm_w, d->cfg.rms_eps, d->B, d->cfg.hidden, d->xn, ADT, st));
    return MI355_OK;
}
} // namespace

extern "C" void mi355_decoder_destroy(mi355_decoder_t* d) {
    if (!d) return;
    drop_graphs(d);
    if (d->cap_stream) hipStreamDestroy(d->cap_stream);
    if (d->side_stream) hipStreamDestroy(d->side_stream);
    if (d->ev_fork) hipEventDestroy(d->ev_fork);
    if (d->ev_join) hipEventDestroy(d->ev_join);
    for (auto e : d->ev) hipEventDestroy(e);
    if (d->pairs_local) hipFree(d->pairs_local);
    delete d;
}

// Which QKV cell of the launch table the step in flight (or last begun) took: 0 image launch, 1 few-row full-K launch, 2 split-K + writer launch,
// 3 split-K slabs folded in the attention prologue; MI355_ERR_ARG before the first step.  Read-only: tests assert the plan they mean to exercise.
extern "C" int mi355_decoder_qkv_launch(const mi355_decoder_t* d) {
    if (!d || d->B <= 0) { mi355_set_error("decoder_qkv_launch: no step begun"); return MI355_ERR_ARG; }
    return (int)d->plan.qkv;
}

// From how many rows a decode step (q_len = 1) takes its QKV projection as split-K slabs folded in the attention prologue, where the configuration allows
// that path at all (plan_launches: slab_qkv); below, the fused QKV launch stays.  rows <= 0: never (the default).  Captured steps bake the chain in: dropped.
extern "C" int mi355_decoder_set_qkv_slab_rows(mi355_decoder_t* d, int32_t rows) {
    if (!d) { mi355_set_error("decoder_set_qkv_slab_rows: null decoder"); return MI355_ERR_ARG; }
    drop_graphs(d);
    d->caps.slab_rows = rows > 0 ? rows : 0;
    return MI355_OK;
}

extern "C" int mi355_decoder_begin(mi355_decoder_t* d, int32_t B, mi355_stream_t stream) {
    return mi355_decoder_begin_rows(d, B, 1, stream);
}

extern "C" int mi355_decoder_begin_rows(mi355_decoder_t* d, int32_t nseq, int32_t q_len, mi355_stream_t stream) {
    const int B = nseq * q_len;
    if (!d || nseq <= 0 || q_len <= 0 || B > d->cfg.max_batch || B > 64) {
        mi355_set_error("decoder_begin: %d sequences x %d rows exceed max_batch or the 64-row limit of the segmented step "
                        "(larger batches: mi355_decoder_step)", nseq, q_len);
        return MI355_ERR_ARG;
    }
    if (int e = resolve_step(d, B, q_len)) return e;
    hipStream_t st = (hipStream_t)stream;
    d->B = B; d->q_len = q_len; d->started = true;
    const auto& c = d->cfg; const StepPlan& p = d->plan;
    if (d->embed_split) {   // hidden-split table: this rank's columns, then the ranks' slices side by side
        const int n = c.hidden / c.tp_size;
        RUN(MI355_KC_OTHER, mi355_embedding(d->bufs.token_ids, B, d->model.embedding, n, d->model.vocab_full, d->act, st));
        RUN(MI355_KC_COMM, mi355_allgather_hidden(d->ar, d->act, d->resid, B, n, st));
    } else {
        RUN(MI355_KC_OTHER, mi355_embedding(d->bufs.token_ids, B, d->model.embedding, c.hidden, d->model.vocab_full, d->resid, st));
    }
    if (p.meet == MeetSel::EXT) return MI355_OK;   // the first segment norms its own rows
    if (p.xn_is_image)
        RUN(MI355_KC_NORM, mi355_add_rmsnorm_img(d->resid, nullptr, 0, 0, nullptr, nullptr, nullptr, d->layers[0].input_norm, c.rms_eps, B, c.hidden, d->xn_img, ADT, st));
    else
        RUN(MI355_KC_NORM, mi355_rmsnorm_dt(d->resid, d->layers[0].input_norm, c.rms_eps, B, c.hidden, d->xn, ADT, st));
    return MI355_OK;
}

extern "C" int mi355_decoder_attach_allreduce(mi355_decoder_t* d, mi355_allreduce_t* ar, int32_t vocab_offset) {
    if (!d || !ar || d->cfg.tp_size <= 1 || vocab_offset < 0) {
        mi355_set_error("decoder_attach_allreduce: needs a decoder created with tp_size > 1 and an opened context"); return MI355_ERR_ARG;
    }
    if ((d->sampling_on || d->logprobs_on) && vocab_offset != mi355_allreduce_rank(ar) * d->cfg.vocab) {
        mi355_set_error("decoder_attach_allreduce: a sampling / logprobs config is active: vocab_offset must be rank * vocab = %d, %d given",
                        mi355_allreduce_rank(ar) * d->cfg.vocab, vocab_offset);
        return MI355_ERR_ARG;
    }
    drop_graphs(d);   // graphs captured for the segmented path are stale now
    d->ar = ar; d->vocab_offset = vocab_offset;
    if (!d->side_stream) d->overlap = side_ready(d);
    return MI355_OK;
}

extern "C" int mi355_decoder_attach_collective(mi355_decoder_t* d, const mi355_collective_t* coll, int32_t vocab_offset) {
    if (!d || !coll || d->cfg.tp_size <= 1 || vocab_offset < 0 || !coll->all_reduce_f16 || !coll->all_gather ||
        coll->world != d->cfg.tp_size || coll->rank < 0 || coll->rank >= coll->world ||
        (d->cfg.act_dtype == MI355_ACT_BF16 && !coll->all_reduce_bf16)) {
        mi355_set_error("decoder_attach_collective: needs a decoder created with tp_size > 1 and a transport of that world size"); return MI355_ERR_ARG;
    }
    if (d->ar) { mi355_set_error("decoder_attach_collective: an all-reduce context is already attached"); return MI355_ERR_ARG; }
    if ((d->sampling_on || d->logprobs_on) && vocab_offset != coll->rank * d->cfg.vocab) {
        mi355_set_error("decoder_attach_collective: a sampling / logprobs config is active: vocab_offset must be rank * vocab = %d, %d given",
                        coll->rank * d->cfg.vocab, vocab_offset);
        return MI355_ERR_ARG;
    }
    drop_graphs(d);
    if (!d->pairs_local) {
        const size_t one = align256((size_t)d->cfg.max_batch * 8);
        if (hipMalloc(&d->pairs_local, one * (1 + (size_t)coll->world)) != hipSuccess) {
            mi355_set_error("decoder_attach_collective: %s", hipGetErrorString(hipGetLastError())); return MI355_ERR_HIP;
        }
        d->pairs_all = (char*)d->pairs_local + one;
    }
    d->ext = *coll; d->has_ext = true; d->vocab_offset = vocab_offset;
    return MI355_OK;
}

extern "C" int mi355_decoder_set_embedding_split(mi355_decoder_t* d, int32_t on) {
    if (!d || (on && (!d->ar || d->cfg.tp_size <= 1 || d->cfg.hidden % (8 * d->cfg.tp_size) != 0))) {
        mi355_set_error("decoder_set_embedding_split: needs an attached all-reduce context and hidden %% (8 tp) == 0"); return MI355_ERR_ARG;
    }
    drop_graphs(d);
    d->embed_split = on != 0;
    return MI355_OK;
}

extern "C" int mi355_decoder_set_weight_prefetch(mi355_decoder_t* d, int32_t mask) {
    if (!d || mask < 0) { mi355_set_error("decoder_set_weight_prefetch: bad argument"); return MI355_ERR_ARG; }
    drop_graphs(d);
    if ((mask & ~(MI355_PF_TP_INLAUNCH | MI355_PF_QKV_IN_FOLD)) != 0 && !side_ready(d)) {
        mi355_set_error("decoder_set_weight_prefetch: cannot create the prefetch stream: %s", hipGetErrorString(hipGetLastError())); return MI355_ERR_HIP;
    }
    d->pf_mask = mask;
    return MI355_OK;
}

extern "C" int mi355_decoder_layer_attn(mi355_decoder_t* d, int32_t l, mi355_stream_t stream) {
    if (!d || l < 0 || l >= d->cfg.num_layers || d->B <= 0) { mi355_set_error("decoder_layer_attn: layer=%d", l); return MI355_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const auto& c = d->cfg; const auto& L = d->layers[l]; const int B = d->B; const StepPlan& p = d->plan;
    if (p.meet == MeetSel::EXT) {
        if (l == 0) RUN(MI355_KC_NORM, mi355_rmsnorm_dt(d->resid, L.input_norm, c.rms_eps, B, c.hidden, d->xn, ADT, st));
        else if (int e = meet_ext_tail(d, st, L.input_norm)) return e;
    }
    int ns = 0;
    mi355_kv_layer_t kv = kv_of(d, l);
    const int pf = p.meet == MeetSel::LOCAL ? d->pf_mask : 0;   // (tp > 1: the side stream belongs to comm_with_prefetch)
    if (int e = pf_join(d, st)) return e;                        // this layer's QKV weights, requested behind the previous down GEMM
    switch (p.qkv) {
    case QkvSel::IMG:
        RUN(MI355_KC_GEMM_QUANT, mi355_qkv_rope_kv_write_img(d->xn_img, B, &L.qkv, L.qkv_bias, d->model.cos_sin, c.rope_dim, c.max_pos,
                                                             d->bufs.positions, d->bufs.block_table, c.max_blocks_per_seq, d->q_len, c.nh,
                                                             &kv, d->q_buf, d->oob_count, st));
        PF_ISSUE(MI355_PF_O | MI355_PF_O_LATE, &L.o);
        break;
    case QkvSel::FULLK: {
        // layer 0 reads the rows mi355_decoder_begin normed; later layers normalise the residual rows on load
        const mi355_fused_norm_t fn = {d->ssq, c.hidden / 16, ssq_pitch(c), L.input_norm, c.rms_eps};
        const bool on_load = p.resid_ssq && l > 0;
        RUN(MI355_KC_GEMM_QUANT, mi355_qkv_rope_kv_write(on_load ? d->resid : d->xn, B, &L.qkv, L.qkv_bias, on_load ? &fn : nullptr,
                                                         d->model.cos_sin, c.rope_dim, c.max_pos, d->bufs.positions,
                                                         d->bufs.block_table, c.max_blocks_per_seq, d->q_len, c.nh, &kv, d->q_buf,
                                                         d->oob_count, st));
        PF_ISSUE(MI355_PF_O | MI355_PF_O_LATE, &L.o);
        break;
    }
    case QkvSel::ATTN_SLABS:   // a plain split-K launch: bias, RoPE and the KV write wait in the attention launch, where a block owns whole heads
        if (p.xn_is_image) RUN(MI355_KC_GEMM_QUANT, ns = mi355_linear_partial_img(d->xn_img, B, &L.qkv, d->partials, kMaxSplits, st));
        else               RUN(MI355_KC_GEMM_QUANT, ns = mi355_linear_partial(d->xn, B, &L.qkv, d->partials, kMaxSplits, st));
        PF_ISSUE(MI355_PF_O | MI355_PF_O_LATE, &L.o);
        break;
    case QkvSel::SPLITK:
        RUN(MI355_KC_GEMM_QUANT, ns = mi355_linear_partial(d->xn, B, &L.qkv, d->partials, kMaxSplits, st));
        PF_ISSUE(MI355_PF_O, &L.o);          // under RoPE + attention
        if (!d->q_norm.empty())   // Qwen3: per-head Q / K RMSNorm in the writer, between the bias add and the rotation
            RUN(MI355_KC_ROPE_KV, mi355_rope_kv_write_rows_qk_norm(nullptr, d->partials, ns, L.qkv.N_pad, L.qkv_bias, d->q_norm[l], d->k_norm[l],
                                                                   c.rms_eps, d->model.cos_sin, c.rope_dim, c.max_pos, d->bufs.positions,
                                                                   d->bufs.block_table, c.max_blocks_per_seq, B, d->q_len, c.nh, &kv, d->q_buf,
                                                                   d->oob_count, st));
        else
            RUN(MI355_KC_ROPE_KV, mi355_rope_kv_write_rows(nullptr, d->partials, ns, L.qkv.N_pad, L.qkv_bias, d->model.cos_sin, c.rope_dim,
                                                           c.max_pos, d->bufs.positions, d->bufs.block_table, c.max_blocks_per_seq, B,
                                                           d->q_len, c.nh, &kv, d->q_buf, d->oob_count, st));
        PF_ISSUE(MI355_PF_O_LATE, &L.o);     // under attention only
        break;
    }
    // q_len > 1: rows of one sequence share a pass over its KV, causal mask inside the page walk (is_target_verify)
    if (p.qkv == QkvSel::ATTN_SLABS)   // q_buf is not written on this path: the launch takes q from the slabs (and nothing else reads q_buf)
        RUN(MI355_KC_ATTN, mi355_paged_attn_qkv_slabs_img(d->partials, ns, L.qkv.N_pad, L.qkv_bias, d->model.cos_sin, c.rope_dim, c.max_pos, &kv,
                                                          d->bufs.block_table, c.max_blocks_per_seq, d->bufs.positions, B, d->q_len, c.nh,
                                                          1.0f / sqrtf((float)c.hd), c.max_seq_len, d->attn_img, d->attn_ws, d->attn_ws_bytes,
                                                          d->oob_count, st));
    else
    RUN(MI355_KC_ATTN, (p.attn_is_image ? mi355_paged_attn_rows_img : mi355_paged_attn_rows)(
                           d->q_buf, &kv, d->bufs.block_table, c.max_blocks_per_seq, d->bufs.positions, B / d->q_len, d->q_len, c.nh,
                           1.0f / sqrtf((float)c.hd), c.max_seq_len, p.attn_is_image ? d->attn_img : d->attn_out, d->attn_ws, d->attn_ws_bytes, st));
    if (int e = pf_join(d, st)) return e;
    void* const gate_in = p.gate_in_is_image ? d->xg_img : d->xn;   // what this half leaves for gate_up (resid_ssq: the residual rows themselves)
    switch (p.o) {
    case OSel::PUBLISH:       // TP: O shard published in the all-reduce buffer -> exchange + residual + norm
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_publish_img(d->attn_img, B, &L.o, nullptr, d->ar, st));
        return meet_published(d, st, L.post_norm, &L.gate_up, gate_in, p.gate_in_is_image);
    case OSel::IMG_PRENORM:   // no norm launch: gate_up finishes the RMSNorm on its accumulators
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_residual_prenorm_img(d->attn_img, B, &L.o, nullptr, d->resid, d->resid, L.post_norm,
                                                                   d->post_norm_exp[l], d->xg_img, d->ssq64, ssq_pitch(c), st));
        return MI355_OK;
    case OSel::IMG:
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_residual_img(d->attn_img, B, &L.o, nullptr, d->resid, d->resid, nullptr, 0, st));
        break;
    case OSel::FULLK:         // h += fp16(attn W_o) in the GEMM's epilogue: no slabs; the norm moves into gate_up (or stays a launch)
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_residual(d->attn_out, B, &L.o, nullptr, d->resid, d->resid, p.resid_ssq ? d->ssq : nullptr, ssq_pitch(c), st));
        if (p.resid_ssq) return MI355_OK;
        break;
    case OSel::SPLITK:
        RUN(MI355_KC_GEMM_QUANT, ns = mi355_linear_partial(d->attn_out, B, &L.o, d->partials, kMaxSplits, st));
        PF_ISSUE(MI355_PF_GATE_UP, &L.gate_up);   // under the reduce + norm launch
        return meet_slabs(d, st, ns, L.o.N_pad, L.post_norm, &L.gate_up, gate_in, p.gate_in_is_image, nullptr);
    }
    PF_ISSUE(MI355_PF_GATE_UP, &L.gate_up);       // IMG, FULLK without the fused norm: the residual is complete, the norm stays a launch
    RUN(MI355_KC_NORM, mi355_rmsnorm_dt(d->resid, L.post_norm, c.rms_eps, B, c.hidden, d->xn, ADT, st));
    return MI355_OK;
}

extern "C" int mi355_decoder_layer_mlp(mi355_decoder_t* d, int32_t l, mi355_stream_t stream) {
    if (!d || l < 0 || l >= d->cfg.num_layers || d->B <= 0) { mi355_set_error("decoder_layer_mlp: layer=%d", l); return MI355_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const auto& c = d->cfg; const auto& L = d->layers[l]; const int B = d->B; const StepPlan& p = d->plan;
    if (p.meet == MeetSel::EXT) if (int e = meet_ext_tail(d, st, L.post_norm)) return e;
    const int pf = p.meet == MeetSel::LOCAL ? d->pf_mask : 0;
    if (int e = pf_join(d, st)) return e;
    void* const act = p.act_is_image ? d->act_img : d->act;   // gate_up's SiLU epilogue writes what the down launch reads
    const int epi = MI355_EPI_SILU_MUL | (p.act_is_image ? MI355_EPI_OUT_IMAGE : 0);
    switch (p.gate_up) {
    case GateSel::DEFERRED_NORM_IMG: {   // the O launch left gamma 2^-e h' and the sums of h'^2: RMSNorm finished on gate_up's accumulators
        const mi355_deferred_norm_t dn = {d->ssq64, c.hidden / 16, ssq_pitch(c), c.rms_eps, ldexpf(1.f, d->post_norm_exp[l])};
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_deferred_norm_img(d->xg_img, B, &dn, &L.gate_up, nullptr, act, epi, st));
        break;
    }
    case GateSel::NORM_ON_LOAD: {        // post-attention RMSNorm on load + gate_up + SiLU-gate in one launch
        const mi355_fused_norm_t fn = {d->ssq, c.hidden / 16, ssq_pitch(c), L.post_norm, c.rms_eps};
        RUN(MI355_KC_GEMM_QUANT, mi355_norm_linear(d->resid, B, &fn, &L.gate_up, nullptr, act, epi, st));
        break;
    }
    case GateSel::DIRECT_IMG:            // TP: the shard as one launch on the image the all-reduce behind the O shard wrote
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_direct_img(d->xg_img, B, &L.gate_up, nullptr, act, epi, st));
        break;
    case GateSel::DIRECT:
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_direct(d->xn, B, &L.gate_up, nullptr, act, epi, d->partials, d->partials_bytes, st));
        break;
    }
    int ns = 0;
    const bool last = l + 1 == c.num_layers;             // the final norm feeds lm_head: row-major, and always a launch
    const void* next_norm = last ? d->model.final_norm : d->layers[l + 1].input_norm;
    const mi355_weight_t* next_qkv = last ? nullptr : &d->layers[l + 1].qkv;
    const mi355_weight_t* next_w = last ? &d->model.lm_head : next_qkv;
    const bool y_image = p.xn_is_image && !last;
    void* const y = y_image ? d->xn_img : d->xn;
    PF_ISSUE(MI355_PF_QKV, next_qkv);                    // under the down GEMM (+ norm)
    switch (p.down) {
    case DownSel::FULLK: {
        const bool ssq = p.resid_ssq && !last;
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_residual(d->act, B, &L.down, nullptr, d->resid, d->resid, ssq ? d->ssq : nullptr, ssq_pitch(c), st));
        if (!ssq) RUN(MI355_KC_NORM, mi355_rmsnorm_dt(d->resid, next_norm, c.rms_eps, B, c.hidden, d->xn, ADT, st));
        return MI355_OK;
    }
    case DownSel::PUBLISH:   // TP: the down shard published in the all-reduce buffer
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_publish_img(d->act_img, B, &L.down, nullptr, d->ar, st));
        return meet_published(d, st, next_norm, next_w, y, y_image);
    case DownSel::QUARTERS:
        RUN(MI355_KC_GEMM_QUANT, ns = mi355_linear_partial_img(d->act_img, B, &L.down, d->partials, kMaxSplits, st));
        break;
    case DownSel::SPLITK:
        RUN(MI355_KC_GEMM_QUANT, ns = mi355_linear_partial(d->act, B, &L.down, d->partials, kMaxSplits, st));
        break;
    }
    PF_ISSUE(MI355_PF_QKV_LATE, next_qkv);               // under the reduce + norm launch only
    // tp = 1 image fold: it runs on B of the 256 CUs, its spare blocks touch the NEXT layer's QKV weights (MI355_PF_QKV_IN_FOLD, internal.h mi355_touch_t)
    mi355_touch_t tc; const mi355_touch_t* touch = nullptr;
    if (y_image && p.meet == MeetSel::LOCAL && (d->pf_mask & MI355_PF_QKV_IN_FOLD) &&
        mi355_qkv_touch_plan(next_qkv, c.hd, d->oob_count + 32, &tc) == MI355_OK) touch = &tc;
    return meet_slabs(d, st, ns, L.down.N_pad, next_norm, next_w, y, y_image, touch);
}

// Dynamic-NTK RoPE (rotary_position_embedding.h:889-951) in PREFILL: context_rope (:1000-1025) rotates every token of the batch with ONE base, that of
// `seq_len` = the longest prompt of the batch (fused_rope_kvcache_kernel.cu:219-260 passes the kernel's padded sequence length), whereas the decode writer
// uses the base of each position -- which is what the model's table holds.  The host builds the {cos, sin} rows [max_pos][rope_dim / 2][2] for the batch's
// base and hands them over for the prefill chunks that follow; NULL returns to the model's table.  No effect on decode steps.
extern "C" int mi355_decoder_set_prefill_rope_table(mi355_decoder_t* d, const float* cos_sin) {
    if (!d) { mi355_set_error("decoder_set_prefill_rope_table: null decoder"); return MI355_ERR_ARG; }
    d->prefill_cos_sin = cos_sin;
    return MI355_OK;
}

// Qwen3 dense models: per-head RMSNorm of Q and K between the QKV projection and RoPE (fused_qk_rmsnorm_v2).  A setter,
// not two more fields of mi355_layer_weights_t, so that the struct and every caller keep their layout.  The launch plan changes with it
// (plan_launches: the fused QKV launches go), hence only before anything was enqueued.
extern "C" int mi355_decoder_set_qk_norm(mi355_decoder_t* d, const void* const* q_norm, const void* const* k_norm) {
    if (!d || !q_norm || !k_norm) { mi355_set_error("decoder_set_qk_norm: null argument"); return MI355_ERR_ARG; }
    if (d->started || !d->graphs.empty()) {
        mi355_set_error("decoder_set_qk_norm: must be called before the first step, prefill or capture"); return MI355_ERR_ARG;
    }
    for (int l = 0; l < d->cfg.num_layers; ++l)
        if (!q_norm[l] || !k_norm[l]) { mi355_set_error("decoder_set_qk_norm: null weights of layer %d", l); return MI355_ERR_ARG; }
    d->q_norm.assign(q_norm, q_norm + d->cfg.num_layers);
    d->k_norm.assign(k_norm, k_norm + d->cfg.num_layers);
    return plan_launches(d);
}

// The intra-block layout of the caches (mi355_kv_layer_t.layout): every launch of the step, of prefill and of a captured graph takes its cache through
// kv_of, so the layout is fixed before the first of them.  No stage selector of the StepPlan depends on it: the same launches, other addresses.
extern "C" int mi355_decoder_set_kv_layout(mi355_decoder_t* d, int32_t layout) {
    if (!d) { mi355_set_error("decoder_set_kv_layout: null decoder"); return MI355_ERR_ARG; }
    if (d->started || !d->graphs.empty()) {
        mi355_set_error("decoder_set_kv_layout: must be called before the first step, prefill or capture"); return MI355_ERR_ARG;
    }
    if (const char* why = mi355_kv_layout_problem(layout, d->cfg.kv_dtype, d->cfg.hd, d->cfg.page)) {
        mi355_set_error("decoder_set_kv_layout: layout=%d kv_dtype=%d hd=%d page=%d: %s", layout, d->cfg.kv_dtype, d->cfg.hd, d->cfg.page, why);
        return MI355_ERR_ARG;
    }
    d->kv_layout = layout;
    return MI355_OK;
}

// ------------------------------------------------------------------ prefill
// One chunk of nseq x q_len prompt tokens through the same weights: large-M GEMMs (gemm_prefill.hip above 128 rows), the
// rows-mode KV writer, causal multi-row attention over the paged cache (earlier chunks of the same prompt are already
// there), fused residual + RMSNorm; logits only for the requested rows (the reference computes lm_head on the last token
// of each sequence, PyWrappedModel.cc:1003-1047).
namespace {
struct PrefillBufs { void *resid, *xn, *qkv, *q, *attn, *act, *tmp, *gemm_ws, *attn_ws, *last_h; size_t gemm_ws_bytes, attn_ws_bytes; };

// upper bound of the split-K slab workspace mi355_linear_forward may ask for on 64-row slabs of this model's linears
size_t linear_ws_bound(const mi355_model_config_t& c) {
    const int qkvdim = (c.nh + 2 * c.nkv) * c.hd;
    const int shapes[4][2] = {{c.hidden, qkvdim}, {c.nh * c.hd, c.hidden}, {c.hidden, 2 * c.inter}, {c.inter, c.hidden}};
    size_t need = 256;
    for (const auto& sh : shapes)
        for (int wbits : {4, 8, 16}) {
            mi355_weight_t w;
            w.qweight = &need; w.meta = &need; w.wbits = wbits; w.wkind = MI355_WKIND_INT; w.K = sh[0]; w.N = sh[1]; w.act_dtype = c.act_dtype;   // bf16 plans other block shapes (and splits) above 32 rows
            w.K_pad = (sh[0] + 127) & ~127; w.N_pad = (sh[1] + 15) & ~15; w.group_size = wbits == 4 ? 128 : 0;   // the split plan reads wbits, not wkind / group_size: FP8 and MXFP4 are covered by 8 and 4
            need = std::max(need, mi355_linear_workspace_bytes(64, &w));
        }
    return need;
}

size_t carve_prefill(const mi355_model_config_t& c, int T, int nseq, void* base, PrefillBufs* out) {
    Carve cv{(char*)base, 0};
    const size_t Ts = (size_t)T;
    const int qdim = c.nh * c.hd, qkvdim = (c.nh + 2 * c.nkv) * c.hd;
    PrefillBufs b;
    b.resid = cv.take(Ts * c.hidden * 2); b.xn = cv.take(Ts * c.hidden * 2); b.qkv = cv.take(Ts * qkvdim * 2);
    b.q = cv.take(Ts * qdim * 2); b.attn = cv.take(Ts * qdim * 2); b.act = cv.take(Ts * c.inter * 2); b.tmp = cv.take(Ts * c.hidden * 2);
    b.last_h = cv.take((size_t)nseq * c.hidden * 2 * 2);
    // 64-row slabs through the decode kernels (chunks below 128 rows) may split K into fp32 slabs: ask the planner
    b.gemm_ws_bytes = linear_ws_bound(c);
    b.gemm_ws = cv.take(b.gemm_ws_bytes);
    b.attn_ws_bytes = mi355_paged_attn_workspace_bytes(T, c.nh, c.hd, c.max_seq_len);
    b.attn_ws = cv.take(b.attn_ws_bytes);
    if (out) *out = b;
    return cv.off;
}

// a row-parallel linear's T rows in b.tmp: (all-reduce +) residual + RMSNorm(norm_w) -> b.xn
int prefill_meet(mi355_decoder* d, hipStream_t st, const PrefillBufs& b, int T, const void* norm_w) {
    const auto& c = d->cfg;
    if (c.tp_size > 1 && d->ar) {
        RUN(MI355_KC_COMM, mi355_allreduce_fused_dt(d->ar, b.tmp, nullptr, 0, 0, nullptr, b.resid, b.resid, norm_w, c.rms_eps, T, c.hidden, b.xn, ADT, st));
        return MI355_OK;
    }
    if (c.tp_size > 1) RUN(MI355_KC_COMM, ext_all_reduce(d, b.tmp, (size_t)T * c.hidden, st));
    RUN(MI355_KC_NORM, mi355_add_rmsnorm_dt(b.tmp, nullptr, 0, 0, nullptr, b.resid, b.resid, norm_w, c.rms_eps, T, c.hidden, b.xn, ADT, st));
    return MI355_OK;
}
} // namespace

extern "C" size_t mi355_decoder_prefill_workspace_bytes(mi355_decoder_t* d, int32_t max_tokens, int32_t max_seqs) {
    if (!d || max_tokens <= 0 || max_seqs <= 0) return 0;
    return carve_prefill(d->cfg, max_tokens, max_seqs, nullptr, nullptr);
}

extern "C" int mi355_decoder_prefill(mi355_decoder_t* d, const int32_t* token_ids, const int32_t* positions, const int32_t* block_table,
                                     int32_t nseq, int32_t q_len, const int32_t* logit_rows, float* logits_out, void* workspace,
                                     size_t workspace_bytes, mi355_stream_t stream) {
    if (!d || !token_ids || !positions || !block_table || nseq <= 0 || q_len <= 0 || !workspace) {
        mi355_set_error("decoder_prefill: bad arguments"); return MI355_ERR_ARG;
    }
    const auto& c = d->cfg;
    const int T = nseq * q_len;
    if (c.tp_size > 1 && !d->ar && !d->has_ext) {
        mi355_set_error("decoder_prefill: tp_size > 1 needs mi355_decoder_attach_allreduce or _attach_collective"); return MI355_ERR_ARG;
    }
    PrefillBufs b;
    const size_t need = carve_prefill(c, T, nseq, workspace, &b);
    if (need > workspace_bytes) { mi355_set_error("decoder_prefill: workspace %zu < %zu", workspace_bytes, need); return MI355_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const float scale = 1.0f / sqrtf((float)c.hd);
    d->started = true;
    if (d->embed_split) {
        const int n = c.hidden / c.tp_size;
        RUN(MI355_KC_OTHER, mi355_embedding(token_ids, T, d->model.embedding, n, d->model.vocab_full, b.tmp, st));
        RUN(MI355_KC_COMM, mi355_allgather_hidden(d->ar, b.tmp, b.resid, T, n, st));
    } else {
        RUN(MI355_KC_OTHER, mi355_embedding(token_ids, T, d->model.embedding, c.hidden, d->model.vocab_full, b.resid, st));
    }
    RUN(MI355_KC_NORM, mi355_rmsnorm_dt(b.resid, d->layers[0].input_norm, c.rms_eps, T, c.hidden, b.xn, ADT, st));
    for (int l = 0; l < c.num_layers; ++l) {
        const auto& L = d->layers[l];
        mi355_kv_layer_t kv = kv_of(d, l);
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_forward(b.xn, T, &L.qkv, L.qkv_bias, b.qkv, MI355_EPI_NONE, b.gemm_ws, b.gemm_ws_bytes, st));
        const float* cs = d->prefill_cos_sin ? d->prefill_cos_sin : d->model.cos_sin;
        if (!d->q_norm.empty())
            RUN(MI355_KC_ROPE_KV, mi355_rope_kv_write_rows_qk_norm(b.qkv, nullptr, 0, L.qkv.N, nullptr, d->q_norm[l], d->k_norm[l], c.rms_eps, cs, c.rope_dim,
                                                                   c.max_pos, positions, block_table, c.max_blocks_per_seq, T, q_len, c.nh, &kv, b.q,
                                                                   d->oob_count, st));
        else
            RUN(MI355_KC_ROPE_KV, mi355_rope_kv_write_rows(b.qkv, nullptr, 0, L.qkv.N, nullptr, cs, c.rope_dim, c.max_pos, positions,
                                                           block_table, c.max_blocks_per_seq, T, q_len, c.nh, &kv, b.q, d->oob_count, st));
        RUN(MI355_KC_ATTN, mi355_paged_attn_rows(b.q, &kv, block_table, c.max_blocks_per_seq, positions, nseq, q_len, c.nh, scale,
                                                 c.max_seq_len, b.attn, b.attn_ws, b.attn_ws_bytes, st));
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_forward(b.attn, T, &L.o, nullptr, b.tmp, MI355_EPI_NONE, b.gemm_ws, b.gemm_ws_bytes, st));
        if (int e = prefill_meet(d, st, b, T, L.post_norm)) return e;
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_forward(b.xn, T, &L.gate_up, nullptr, b.act, MI355_EPI_SILU_MUL, b.gemm_ws, b.gemm_ws_bytes, st));
        RUN(MI355_KC_GEMM_QUANT, mi355_linear_forward(b.act, T, &L.down, nullptr, b.tmp, MI355_EPI_NONE, b.gemm_ws, b.gemm_ws_bytes, st));
        const void* next_norm = (l + 1 < c.num_layers) ? d->layers[l + 1].input_norm : d->model.final_norm;
        if (int e = prefill_meet(d, st, b, T, next_norm)) return e;
    }
    if (logit_rows && logits_out) {   // gather the requested rows of the final normed hidden state, then lm_head on nseq rows
        RUN(MI355_KC_OTHER, mi355_embedding(logit_rows, nseq, b.xn, c.hidden, T, b.last_h, st));
        for (int r0 = 0; r0 < nseq; r0 += 64) {
            const int n = nseq - r0 < 64 ? nseq - r0 : 64;
            RUN(MI355_KC_GEMM_LMHEAD, mi355_linear_direct((const char*)b.last_h + (size_t)r0 * c.hidden * 2, n, &d->model.lm_head, nullptr,
                                                          logits_out + (size_t)r0 * c.vocab, MI355_EPI_OUT_F32, nullptr, 0, st));
        }
    }
    return MI355_OK;
}

namespace {
// vocab-split greedy through the external transport: (max, global index) per row, all-gathered, best per row
int ext_argmax(mi355_decoder* d, int B, hipStream_t st) {
    const auto& c = d->cfg;
    RUN(MI355_KC_OTHER, mi355_argmax_pairs(d->bufs.logits, B, c.vocab, c.vocab, d->vocab_offset, d->pairs_local, d->argmax_ws,
                                           d->argmax_ws_bytes, st));
    RUN(MI355_KC_COMM, d->ext.all_gather(d->ext.ctx, d->pairs_local, d->pairs_all, (size_t)B * 8, (mi355_stream_t)st) == 0
                           ? MI355_OK : (mi355_set_error("decoder: the attached transport's all-gather failed"), MI355_ERR_HIP));
    RUN(MI355_KC_OTHER, mi355_argmax_pick(d->pairs_all, d->ext.world, B, d->bufs.token_ids, d->bufs.positions, st));
    return MI355_OK;
}
// log-probabilities of the ids in token_ids under B rows of `logits` (V columns, dense), recorded per slot (mi355_decoder_set_logprobs): the two
// launches of logprobs.hip, nothing without a config or on verify rows
int logprob_tail(mi355_decoder* d, const float* logits, int V, int B, int q_len, const float* temperature, hipStream_t st) {
    if (!d->logprobs_on || q_len != 1) return MI355_OK;
    const mi355_logprobs_t& lp = d->logprobs;
    RUN(MI355_KC_OTHER, mi355_logprobs_segments(logits, B, V, V, temperature, lp.top_n, lp.workspace, lp.workspace_bytes, st));
    RUN(MI355_KC_OTHER, mi355_logprobs_rows(logits, B, V, V, temperature, d->bufs.token_ids, lp.top_n, lp.token_logprobs, nullptr,
                                            lp.top_ids, lp.top_logprobs, lp.top_n, lp.log_ld, lp.count, lp.cum_log_probs, lp.workspace,
                                            lp.workspace_bytes, st));
    return MI355_OK;
}
// greedy ids of B rows of logits -> token_ids (and positions + 1) for the next step
int greedy_tail(mi355_decoder* d, int B, int q_len, hipStream_t st) {
    const auto& c = d->cfg;
    if (d->ar)   // vocab-split lm_head: (max, index) pairs cross the ranks, not the logits
        RUN(MI355_KC_COMM, mi355_allreduce_argmax(d->ar, d->bufs.logits, B, c.vocab, c.vocab, d->vocab_offset, d->bufs.token_ids,
                                                  d->bufs.positions, d->argmax_ws, d->argmax_ws_bytes, st));
    else if (d->has_ext) return ext_argmax(d, B, st);
    else RUN(MI355_KC_OTHER, mi355_argmax_ex(d->bufs.logits, B, c.vocab, c.vocab, d->bufs.token_ids, d->bufs.positions, d->argmax_ws, d->argmax_ws_bytes, st));
    return logprob_tail(d, d->bufs.logits, c.vocab, B, q_len, nullptr, st);
}
// sampled ids of B rows of `logits` (V columns, dense) -> token_ids, positions + 1 and the history (mi355_decoder_set_sampling).  The
// penalties act in place: the rows hold the penalised logits afterwards.  The token drawn here sits at position positions + 1.
int sampled_tail(mi355_decoder* d, float* logits, int V, int B, hipStream_t st) {
    const mi355_sampling_t& s = d->sampling;
    if (s.repetition_penalty || s.presence_penalty || s.frequency_penalty)
        RUN(MI355_KC_OTHER, mi355_apply_penalties_history(logits, B, V, V, s.repetition_penalty, s.presence_penalty,
                                                          s.frequency_penalty, s.history, s.history_ld, s.history_len, d->penalty_ws, st));
    RUN(MI355_KC_OTHER, mi355_sample_logits_ex(logits, B, V, V, s.temperature, s.top_k, s.top_p, nullptr, s.seed,
                                               d->bufs.positions, 1, d->bufs.token_ids, nullptr, nullptr, 0, d->sample_ws, d->sample_ws_bytes, st));
    if (int e = logprob_tail(d, logits, V, B, 1, s.temperature, st)) return e;
    RUN(MI355_KC_OTHER, mi355_sample_feedback(d->bufs.token_ids, B, d->bufs.positions, s.history, s.history_len, s.history_ld, st));
    return MI355_OK;
}
// tp_size > 1 with a sampling / logprobs config: the ranks' [B][vocab] slices of bufs.logits side by side in d->gathered, [B][tp_size * vocab]
// (bufs.logits keeps the rank's raw slice).  Attached context: the peer-read gather, one MI355_KC_COMM op per launch; external transport: its
// all_gather of the contiguous block into the staging, then the reorder launch.
int gather_logits(mi355_decoder* d, int B, hipStream_t st) {
    const auto& c = d->cfg;
    if (d->ar) {
        const int n = mi355_allgather_logits_launches(d->ar, B, c.vocab);
        if (n < 0) return n;
        for (int part = 0; part < n; ++part)
            RUN(MI355_KC_COMM, mi355_allgather_logits_part(d->ar, d->bufs.logits, c.vocab, d->gathered, B, c.vocab, part, st));
        return MI355_OK;
    }
    RUN(MI355_KC_COMM, d->ext.all_gather(d->ext.ctx, d->bufs.logits, d->gather_stage, (size_t)B * c.vocab * 4, (mi355_stream_t)st) == 0
                           ? MI355_OK : (mi355_set_error("decoder: the attached transport's all-gather failed"), MI355_ERR_HIP));
    RUN(MI355_KC_OTHER, mi355_interleave_logits(d->gather_stage, d->gathered, c.tp_size, B, c.vocab, st));
    return MI355_OK;
}
int step_tail(mi355_decoder* d, int B, int q_len, hipStream_t st) {
    const auto& c = d->cfg;
    if (c.tp_size > 1 && q_len == 1 && (d->sampling_on || d->logprobs_on)) {   // only reachable with the gathered buffer set (the setters refuse otherwise)
        if (!d->gathered || (!d->ar && !d->has_ext)) { mi355_set_error("decoder: sampling / logprobs at tp_size %d without the gathered-logits buffer or a transport", c.tp_size); return MI355_ERR_ARG; }
        const int VF = c.tp_size * c.vocab;
        if (int e = gather_logits(d, B, st)) return e;
        if (d->sampling_on) return sampled_tail(d, d->gathered, VF, B, st);
        // greedy with log-probabilities: arg-max of the gathered row (lowest global index on ties: the id the cross-rank arg-max gives)
        RUN(MI355_KC_OTHER, mi355_argmax_ex(d->gathered, B, VF, VF, d->bufs.token_ids, d->bufs.positions, d->argmax_ws, d->argmax_ws_bytes, st));
        return logprob_tail(d, d->gathered, VF, B, 1, nullptr, st);
    }
    return d->sampling_on && q_len == 1 ? sampled_tail(d, d->bufs.logits, c.vocab, B, st) : greedy_tail(d, B, q_len, st);
}
// columns the sampled tail and the recorder see: the whole vocabulary under tensor parallelism (mi355_decoder_set_gathered_logits)
int tail_cols(const mi355_model_config_t& c) { return c.tp_size > 1 ? c.tp_size * c.vocab : c.vocab; }
size_t sampling_penalty_bytes(const mi355_model_config_t& c) { return align256((size_t)c.max_batch * tail_cols(c) * sizeof(int32_t)); }
size_t gathered_rows_bytes(const mi355_model_config_t& c) { return align256((size_t)c.max_batch * c.tp_size * c.vocab * sizeof(float)); }
// what a sampling / logprobs config needs at tp_size > 1, or 0: the gathered buffer, a transport, the rank's slice at rank * vocab of an evenly split vocabulary
int tp_tail_problem(mi355_decoder* d, const char* who, const char* what) {
    const auto& c = d->cfg;
    if (!d->gathered) {
        mi355_set_error("%s: tp_size %d: the lm_head is split over the vocabulary, %s tp_size 1", who, c.tp_size, what);
        return MI355_ERR_UNSUPPORTED;
    }
    if (!d->ar && !d->has_ext) { mi355_set_error("%s: tp_size %d needs mi355_decoder_attach_allreduce / _attach_collective first", who, c.tp_size); return MI355_ERR_ARG; }
    if (d->model.vocab_full != c.tp_size * c.vocab) {
        mi355_set_error("%s: vocab_full %d != tp_size %d x vocab %d: a vocabulary that does not split evenly is not served", who, d->model.vocab_full, c.tp_size, c.vocab);
        return MI355_ERR_UNSUPPORTED;
    }
    const int rank = d->ar ? mi355_allreduce_rank(d->ar) : d->ext.rank;
    if (d->vocab_offset != rank * c.vocab) {
        mi355_set_error("%s: vocab_offset %d of the attach call must be rank %d x vocab %d", who, d->vocab_offset, rank, c.vocab); return MI355_ERR_ARG;
    }
    return MI355_OK;
}
} // namespace

extern "C" size_t mi355_decoder_gathered_logits_bytes(const mi355_model_config_t* cfg) {
    if (!cfg || cfg->tp_size <= 1 || cfg->max_batch <= 0 || cfg->vocab <= 0) return 0;
    return 2 * gathered_rows_bytes(*cfg);   // the gathered rows, then the staging of an external transport's all_gather ([tp_size][max_batch][vocab])
}

extern "C" int mi355_decoder_set_gathered_logits(mi355_decoder_t* d, float* buf, size_t bytes) {
    if (!d) { mi355_set_error("decoder_set_gathered_logits: decoder is null"); return MI355_ERR_ARG; }
    if (d->cfg.tp_size <= 1) { mi355_set_error("decoder_set_gathered_logits: tp_size 1 has nothing to gather"); return MI355_ERR_ARG; }
    if (!buf) {
        if (d->sampling_on || d->logprobs_on) {
            mi355_set_error("decoder_set_gathered_logits: a sampling / logprobs config is active: clear it first"); return MI355_ERR_ARG;
        }
        drop_graphs(d); d->gathered = d->gather_stage = nullptr;
        return MI355_OK;
    }
    if ((reinterpret_cast<uintptr_t>(buf) & 255) != 0) { mi355_set_error("decoder_set_gathered_logits: the buffer must be 256-byte aligned"); return MI355_ERR_ARG; }
    if (d->cfg.vocab % 4 != 0) { mi355_set_error("decoder_set_gathered_logits: vocab %d per rank is not a multiple of 4", d->cfg.vocab); return MI355_ERR_UNSUPPORTED; }
    const size_t need = mi355_decoder_gathered_logits_bytes(&d->cfg);
    if (bytes < need) { mi355_set_error("decoder_set_gathered_logits: %zu bytes needed, %zu given", need, bytes); return MI355_ERR_WORKSPACE; }
    drop_graphs(d);
    d->gathered = buf; d->gather_stage = (float*)((char*)buf + gathered_rows_bytes(d->cfg));
    return MI355_OK;
}

extern "C" size_t mi355_decoder_sampling_workspace_bytes(const mi355_model_config_t* cfg) {
    if (!cfg || cfg->max_batch <= 0 || cfg->vocab <= 0) return 0;
    return sampling_penalty_bytes(*cfg) + align256(mi355_sample_logits_workspace_bytes(cfg->max_batch, tail_cols(*cfg)));
}

extern "C" int mi355_decoder_set_sampling(mi355_decoder_t* d, const mi355_sampling_t* s) {
    if (!d) { mi355_set_error("decoder_set_sampling: decoder is null"); return MI355_ERR_ARG; }
    if (!s) { drop_graphs(d); d->sampling_on = false; return MI355_OK; }
    if (d->cfg.tp_size > 1) if (int e = tp_tail_problem(d, "decoder_set_sampling", "sampling needs")) return e;
    if (!s->seed) { mi355_set_error("decoder_set_sampling: seed [max_batch] is null"); return MI355_ERR_ARG; }
    const bool pen = s->repetition_penalty || s->presence_penalty || s->frequency_penalty;
    if ((pen || s->history || s->history_len) && (!s->history || !s->history_len || s->history_ld <= 0)) {
        mi355_set_error("decoder_set_sampling: penalties / a history need history [max_batch][history_ld], history_len [max_batch] and history_ld > 0");
        return MI355_ERR_ARG;
    }
    const size_t need = mi355_decoder_sampling_workspace_bytes(&d->cfg);
    if (!s->workspace || s->workspace_bytes < need || (reinterpret_cast<uintptr_t>(s->workspace) & 255) != 0) {
        mi355_set_error("decoder_set_sampling: workspace of %zu bytes (256-byte aligned) needed, %zu given", need, s->workspace ? s->workspace_bytes : (size_t)0);
        return MI355_ERR_WORKSPACE;
    }
    drop_graphs(d);
    d->sampling = *s; d->sampling_on = true;
    d->penalty_ws = (int32_t*)s->workspace;
    d->sample_ws = (char*)s->workspace + sampling_penalty_bytes(d->cfg);
    d->sample_ws_bytes = need - sampling_penalty_bytes(d->cfg);
    return MI355_OK;
}

extern "C" size_t mi355_decoder_logprobs_workspace_bytes(const mi355_model_config_t* cfg, int32_t top_n) {
    if (!cfg || cfg->max_batch <= 0 || cfg->vocab <= 0) return 0;
    return align256(mi355_logprobs_workspace_bytes(cfg->max_batch, tail_cols(*cfg), top_n));
}

extern "C" int mi355_decoder_set_logprobs(mi355_decoder_t* d, const mi355_logprobs_t* lp) {
    if (!d) { mi355_set_error("decoder_set_logprobs: decoder is null"); return MI355_ERR_ARG; }
    if (!lp) { drop_graphs(d); d->logprobs_on = false; return MI355_OK; }
    if (d->cfg.tp_size > 1) if (int e = tp_tail_problem(d, "decoder_set_logprobs", "log-probabilities need")) return e;
    if (lp->top_n < 0 || lp->top_n > MI355_LOGPROBS_MAX_TOP) {
        mi355_set_error("decoder_set_logprobs: top_n %d outside [0, %d]", lp->top_n, MI355_LOGPROBS_MAX_TOP); return MI355_ERR_ARG;
    }
    if (lp->log_ld < 1 || !lp->token_logprobs || !lp->count) {
        mi355_set_error("decoder_set_logprobs: needs log_ld >= 1 (%d given), token_logprobs [max_batch][log_ld] and count [max_batch]", lp->log_ld);
        return MI355_ERR_ARG;
    }
    if (lp->top_n > 0 && (!lp->top_ids || !lp->top_logprobs)) {
        mi355_set_error("decoder_set_logprobs: top_n %d needs top_ids and top_logprobs [max_batch][log_ld][top_n]", lp->top_n); return MI355_ERR_ARG;
    }
    const size_t need = mi355_decoder_logprobs_workspace_bytes(&d->cfg, lp->top_n);
    if (!lp->workspace || lp->workspace_bytes < need || (reinterpret_cast<uintptr_t>(lp->workspace) & 255) != 0) {
        mi355_set_error("decoder_set_logprobs: workspace of %zu bytes (256-byte aligned) needed, %zu given", need, lp->workspace ? lp->workspace_bytes : (size_t)0);
        return MI355_ERR_WORKSPACE;
    }
    drop_graphs(d);
    d->logprobs = *lp; d->logprobs_on = true;
    return MI355_OK;
}

extern "C" int mi355_decoder_finish(mi355_decoder_t* d, int32_t sample, mi355_stream_t stream) {
    if (!d || d->B <= 0) { mi355_set_error("decoder_finish: no step in flight"); return MI355_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int B = d->B;
    if (int e = pf_join(d, st)) return e;
    if (d->plan.meet == MeetSel::EXT) if (int e = meet_ext_tail(d, st, d->model.final_norm)) return e;
    RUN(MI355_KC_GEMM_LMHEAD, mi355_linear_direct(d->xn, B, &d->model.lm_head, nullptr, d->bufs.logits, MI355_EPI_OUT_F32, nullptr, 0, st));
    return sample ? step_tail(d, B, d->q_len, st) : MI355_OK;
}

extern "C" int mi355_decoder_step(mi355_decoder_t* d, int32_t B, mi355_stream_t stream) {
    if (!d || (d->cfg.tp_size != 1 && !d->ar && !d->has_ext)) {
        mi355_set_error("decoder_step: tp_size > 1 needs mi355_decoder_attach_allreduce / _attach_collective (or the segment calls)");
        return MI355_ERR_ARG;
    }
    if (B > 64) {   // large batch: the generic path (large-M GEMMs, fp16 intermediates), one row per sequence
        if (B > d->cfg.max_batch) { mi355_set_error("decoder_step: B=%d > max_batch", B); return MI355_ERR_ARG; }
        const int rc = mi355_decoder_prefill(d, d->bufs.token_ids, d->bufs.positions, d->bufs.block_table, B, 1, d->iota, d->bufs.logits,
                                             d->wide_ws, d->wide_ws_bytes, stream);
        return rc < 0 ? rc : step_tail(d, B, 1, (hipStream_t)stream);
    }
    int rc = mi355_decoder_begin(d, B, stream);
    for (int l = 0; rc >= 0 && l < d->cfg.num_layers; ++l) {
        rc = mi355_decoder_layer_attn(d, l, stream);
        if (rc >= 0) rc = mi355_decoder_layer_mlp(d, l, stream);
    }
    if (rc >= 0) rc = mi355_decoder_finish(d, 1, stream);
    return rc < 0 ? rc : MI355_OK;
}

extern "C" int mi355_decoder_capture(mi355_decoder_t* d, int32_t B) {
    if (!d || B <= 0 || B > d->cfg.max_batch) { mi355_set_error("decoder_capture: B=%d", B); return MI355_ERR_ARG; }
    if (d->graphs.count(B)) return MI355_OK;
    hipError_t e = hipSuccess;
    if (!d->cap_stream && (e = hipStreamCreateWithFlags(&d->cap_stream, hipStreamNonBlocking)) != hipSuccess) {
        mi355_set_error("decoder_capture: stream create failed: %s", hipGetErrorString(e)); return MI355_ERR_HIP;
    }
    e = hipStreamBeginCapture(d->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { mi355_set_error("decoder_capture: begin: %s", hipGetErrorString(e)); return MI355_ERR_HIP; }
    const int rc = mi355_decoder_step(d, B, d->cap_stream);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(d->cap_stream, &g);
    if (rc < 0) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) { mi355_set_error("decoder_capture: end: %s", hipGetErrorString(e)); return MI355_ERR_HIP; }
    hipGraphExec_t ge = nullptr;
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) { mi355_set_error("decoder_capture: instantiate: %s", hipGetErrorString(e)); return MI355_ERR_HIP; }
    d->graphs[B] = ge;
    return MI355_OK;
}

// Host-side helper for drivers that capture the TP step (collectives included) with their framework's graph API: if that
// capture is invalidated half way (an un-capturable collective), the stream is left capturing and every later launch
// fails.  Ends whatever capture is active on `stream`, discarding the partial graph.  Not part of the public ABI.
extern "C" int mi355_abort_capture(mi355_stream_t stream) {
    (void)hipGetLastError();   // the status query itself fails on an invalidated capture: just try to end it
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture((hipStream_t)stream, &g);
    if (g) hipGraphDestroy(g);
    (void)hipGetLastError();
    return MI355_OK;
}

extern "C" int mi355_decoder_replay(mi355_decoder_t* d, int32_t B, int32_t nsteps, mi355_stream_t stream) {
    if (!d || !d->graphs.count(B)) { mi355_set_error("decoder_replay: no graph for B=%d", B); return MI355_ERR_ARG; }
    hipGraphExec_t ge = d->graphs[B];
    for (int i = 0; i < nsteps; ++i) {
        hipError_t e = hipGraphLaunch(ge, (hipStream_t)stream);
        if (e != hipSuccess) { mi355_set_error("decoder_replay: %s", hipGetErrorString(e)); return MI355_ERR_HIP; }
    }
    return MI355_OK;
}

extern "C" int64_t mi355_decoder_oob_count(mi355_decoder_t* d, mi355_stream_t stream) {
    if (!d) { mi355_set_error("decoder_oob_count: null decoder"); return MI355_ERR_ARG; }
    int32_t v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(&v, d->oob_count, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) {
        mi355_set_error("decoder_oob_count: %s", hipGetErrorString(hipGetLastError()));
        return MI355_ERR_HIP;
    }
    return v;
}

extern "C" int mi355_decoder_profile(mi355_decoder_t* d, int32_t B, int32_t nsteps, float* out_ms, int32_t* out_launches,
                                     mi355_stream_t stream) {
    if (!d || !out_ms || !out_launches || nsteps <= 0) { mi355_set_error("decoder_profile: bad args"); return MI355_ERR_ARG; }
    for (int k = 0; k < MI355_KC_COUNT; ++k) { out_ms[k] = 0.f; out_launches[k] = 0; }
    d->prof_on = true; d->ev_used = 0; d->ev_class.clear();
    int rc = MI355_OK;
    for (int i = 0; i < nsteps && rc >= 0; ++i) rc = mi355_decoder_step(d, B, stream);
    d->prof_on = false;
    hipStreamSynchronize((hipStream_t)stream);
    if (rc < 0) return rc;
    for (size_t i = 0; i < d->ev_class.size(); ++i) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, d->ev[2 * i], d->ev[2 * i + 1]);
        out_ms[d->ev_class[i]] += ms;
        out_launches[d->ev_class[i]] += 1;
    }
    return MI355_OK;
}
