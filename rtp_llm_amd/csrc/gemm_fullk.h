// Parameter block, epilogue kinds and the per-wave stamps shared by the full-K launches: gemm_fullk.hip (<= 16 rows and the
// generic shapes) and gemm_fullk64.hip (1-64 rows, W4 group-wise).
#pragma once
#include "gemm_common.h"

namespace {

struct RopeEpi {
    const float*   cos_sin;
    const int32_t* positions;
    const int32_t* block_table;
    int            max_blocks, nh, nkv, hd, page, max_pos, num_blocks, q_len;
    int32_t*       oob_count;
    void*          kv_base;
    f16*           q_out;
    // the cache's intra-block layout (mi355_kv_layer_t.layout) as strides, so that the epilogue is the same code for every layout: inside a head's
    // page * hd elements, K (tok, d) sits at tok * k_tok + (d / 8) * k_chunk + d % 8 and V (tok, d) at d * v_d + (tok / 8) * v_win + tok % 8
    int            k_tok, k_chunk, v_d, v_win;
};
struct FullKParams {
    GemmParams g;
    const f16* res_in;
    f16*       res_out;
    RopeEpi    r;
    // NORM: x is the un-normed residual row h; the kernel applies RMSNorm on the fly, x_n = gamma * fp16(h * rs), with
    // rs = rsqrt(sum_k h^2 / K + eps) rebuilt from the per-tile partial sums the producing launch left in ssq_in
    const float* ssq_in;     // [rows][ssq_ld], ssq_ld >= ssq_tiles: sum over the 16 columns of tile t of h[row]^2
    int          ssq_tiles, ssq_ld;
    const f16*   gamma;
    float        eps;
    float*       ssq_out;    // FK_RESID: the same partial sums of the rows this launch produces ([M][ssq_ld]), or null
    int          ilv;        // K slices of the waves interleaved chunk by chunk (see the kernel)
    // FK_RESID of gemm_fullk64.hip, deferred RMSNorm of the rows it produces: besides h' it stores g = fp16(gamma 2^-e h') as an
    // activation image for the next GEMM, which multiplies its accumulators by rsqrt(mean h'^2 + eps) 2^e (from ssq_out)
    f16*         xg_img;     // image of g ([M][N]), or null
    const f16*   xg_gamma;   // norm weight [N]
    float        xg_scale;   // 2^-e with e >= log2(max |gamma|): |g| <= |h'|, no overflow whatever the residual stream holds
    int          rowsplit;   // gemm_fullk64.hip: two blocks per tile pair, 32 rows each (block b: pair b / 2, row blocks 2 (b & 1) .. + 1)
    int          bf16;       // gemm_fullk64.hip: bias / residual / norm weight / q / KV cache are bf16 (the activation image and the MFMAs stay fp16)
    // FK_PUB (gemm_fullk64.hip, tensor parallelism; round 6): y = 16-bit(xW + bias) goes straight into THIS RANK'S REGISTERED ALL-REDUCE BUFFER
    // (csrc/allreduce.hip), in the slot and parity the next fused all-reduce launch of that context reads -- a row-parallel shard (O / down) then needs
    // neither split-K slabs nor the fold + publish stage in front of the flag exchange (mi355_allreduce_fused_published_dt).  Row m of a <= 64-row
    // call lives in slot m (one row per block), parity (epoch[m] + 1) & 1 of the context's device-resident call counters.
    const uint32_t* pub_epoch;
    void*           pub_data;
    uint32_t        pub_bytes, pub_parity_elems, pub_slot_elems;
    int             pub_plain;  // 1: plain stores (full-fence hand-over: the all-reduce launch's system-scope release fence publishes them); 0: write-through (sc0 sc1)
#ifdef MI355_FULLK_STAMPS   // tuning build with MI355_EXTRA_CFLAGS=-DMI355_FULLK_STAMPS only: the stamp stores change the schedule
    unsigned long long* stamps;   // tools/fullk_stamps.py: wall_clock64 per wave at entry / requests out (+ 1 / rms there) / first chunk done / loop done / slices met / exit
#endif
};
#ifdef MI355_FULLK_STAMPS
#define FK_STAMP(i) do { if (fp.stamps && lane == 0) fp.stamps[((size_t)blockIdx.x * 16 + wave) * 6 + (i)] = wall_clock64(); } while (0)
#else
#define FK_STAMP(i) do { } while (0)
#endif
enum { FK_PLAIN = 0, FK_RESID = 1, FK_ROPE = 2, FK_PUB = 3 };

// Launch head of gemm_fullk64_kernel (kernarg preload): what a K-slice wave needs before its first weight request is out -- the block's unit
// (rowsplit, hd), the helper / K-wave split (nw = K-slice waves of the block), the weight and meta descriptors (qw, meta, KC, N_pad, NT, ilv) and the image (x, M).
// These travel as the kernel's LEADING SCALAR parameters, which arrive in SGPRs at wave start (14 dwords: the whole preload budget next to the kernarg
// segment pointer); a by-value struct is never preloaded, so the rest of FullKParams follows them unchanged and the kernel's first lines put the head back.
// h_hd is a COPY of r.hd for the block's tile numbers only and is not put back: the epilogue reads r.hd with its neighbours, and a dead slot inside that run
// made hipcc load the run wide over it at entry, reuse the dead register at once and wait for the load in front of the weight requests.
#define FULLK_HEAD_PARAMS const void* h_qw, const uint32_t* h_meta, const f16* h_x, int h_M, int h_KC, int h_N_pad, int h_NT, int h_ilv, int h_rowsplit, int h_hd, int h_nw
#define FULLK_HEAD_BIND(fp)                                                                                                              \
    do { (fp).g.qw = h_qw; (fp).g.meta = h_meta; (fp).g.x = h_x; (fp).g.M = h_M; (fp).g.KC = h_KC; (fp).g.N_pad = h_N_pad; (fp).g.NT = h_NT; \
         (fp).ilv = h_ilv; (fp).rowsplit = h_rowsplit; } while (0)
// the one place that splits a filled FullKParams into head + rest
template <class Kernel>
inline void launch_fullk_head(Kernel k, dim3 grid, dim3 block, size_t lds, hipStream_t st, const FullKParams& fp, int nw) {
    hipLaunchKernelGGL(k, grid, block, lds, st, fp.g.qw, fp.g.meta, fp.g.x, fp.g.M, fp.g.KC, fp.g.N_pad, fp.g.NT, fp.ilv, fp.rowsplit, fp.r.hd, nw, fp);
}

inline void set_kv_layout(RopeEpi& r, int layout, int hd, int page) {
    const bool kref = layout != MI355_KV_LAYOUT_NATIVE, vvec = layout == MI355_KV_LAYOUT_REF_VVEC;
    r.k_tok = kref ? 8 : hd;   r.k_chunk = kref ? page * 8 : 8;    // [page][hd]  |  [hd/8][page][8]
    r.v_d   = vvec ? 8 : page; r.v_win   = vvec ? hd * 8 : 8;      // [hd][page]  |  [page/8][hd][8]
}
// offset of the epilogue's K piece (4 channels from d0, d0 % 4 == 0: inside one 8-channel chunk, so one 8-byte store in every layout)
__device__ __forceinline__ int kv_k_offset(const RopeEpi& r, int tok, int d0) { return tok * r.k_tok + (d0 >> 3) * r.k_chunk + (d0 & 7); }
__device__ __forceinline__ int kv_v_offset(const RopeEpi& r, int tok, int d) { return d * r.v_d + (tok >> 3) * r.v_win + (tok & 7); }

} // namespace
