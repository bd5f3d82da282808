// Log-probabilities of fp32 logit rows, gfx950 (mi355_logprobs; the recorder of the step driver, mi355_decoder_set_logprobs): per row
// the log-probability of one token, the log-sum-exp and the top-N alternatives under the full-vocabulary softmax of the scaled logits
// x = logit * inv_t -- the expression of sample_fused.hip, so what is reported is the distribution the sampler draws from before its
// top-k / top-p cut.  Two launches, no memset node, no atomics:
//   pass A, grid (kSegs, rows): the fixed cut of a row of the sampling tail (kSegs segments, length a multiple of 4, 16-byte loads
//     where the row allows).  A block stages its segment as scaled values in LDS (kChunk entries at a time, NaN as -inf) and leaves
//     the segment's maximum m, s = sum exp(x - m), and its N best entries as KEYS, descending;
//   pass B, one block per row: M = max m_i, S = sum_i s_i exp(m_i - M) in segment order, lse = M + log S, the kSegs x N keys ranked
//     into the row's top-N, token value and records written (and, for the step driver, the per-slot recorder advanced).
// A KEY is 64 bits: the order-preserving integer image of the fp32 value above the complemented index, so that "value descending,
// equal values by ascending index" is one unsigned compare, keys are distinct, and 0 is free to mean "no entry" (-inf and NaN never
// get a key).  -0 is read as +0 on the way in, so equal values have equal images.  The value a record reports is decoded from the
// key, the token's value goes through the same canonical form: the same fp32 number, hence x - lse bit for bit.
// Every reduction has a fixed shape -- entry i of a chunk belongs to thread i % kT whatever the load path, waves fold by xor
// shuffles, the four waves and the kSegs segments in index order -- so a row's outputs depend on the row, its temperature and its
// id alone: not on the number of rows, the row index, the row stride or timing.
// A row with no finite-or-+inf entry at all (every entry -inf or NaN) has no distribution: lse = -inf, the token value is NaN
// (-inf - -inf), the top-N slots are all (-1, -inf).  Pass B is one small block per row: each of its threads folds the kSegs
// segment results itself (32 expf and a logf) instead of one thread broadcasting them.
#include "common.h"
#include "internal.h"

namespace {

constexpr int kSegs = 32;              // segments per row: the cut of sample_fused.hip
constexpr int kT = 256;                // threads of both launches
constexpr int kWaves = kT / 64;
constexpr int kChunk = 6144;           // entries of a segment staged in LDS at a time (24 KB): one chunk up to V = 196608
constexpr int kMaxTop = MI355_LOGPROBS_MAX_TOP;
typedef unsigned long long u64;

struct LpParams {
    const float*   logits;
    int            rows, V, ld, seg;   // seg: entries per segment, a multiple of 4
    const float*   temperature;
    int            top_n;
    float*         seg_ms;             // [rows][2][kSegs]: maxima, sums
    u64*           cand;               // [rows][kSegs][top_n]
    // pass B
    const int32_t* ids;
    float*         token_lp;           // [rows][log_ld]
    float*         lse_out;
    int32_t*       top_ids;            // [rows][log_ld][top_ld]
    float*         top_lp;
    int            top_ld, log_ld;     // log_ld = 1 without a recorder
    int32_t*       count;              // recorder: [rows] column the next call writes; NULL: column 0, always written
    float*         cum;                // recorder: [rows] += the token's value
};

__device__ __forceinline__ float inv_temp(const LpParams& p, int row) {   // as sample_fused.hip
    return p.temperature ? 1.0f / (p.temperature[row] + 1e-6f) : 1.0f;
}
// the one value of an entry every pass works on: NaN counts as -inf, -0 as +0
__device__ __forceinline__ float canon(float x) { return x != x ? -INFINITY : x + 0.0f; }
__device__ __forceinline__ u64 key_of(float x, int index) {
    if (!(x > -INFINITY)) return 0;
    const uint32_t u = __float_as_uint(x);
    const uint32_t ord = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ((u64)ord << 32) | (uint32_t)~(uint32_t)index;
}
__device__ __forceinline__ float key_value(u64 k) {
    const uint32_t ord = (uint32_t)(k >> 32);
    return __uint_as_float((ord & 0x80000000u) ? ord ^ 0x80000000u : ~ord);
}
__device__ __forceinline__ int key_index(u64 k) { return (int)~(uint32_t)k; }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        const u64 w = ((u64)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}
// result in every thread; the four waves meet in index order
__device__ __forceinline__ float block_max(float v, float* s_w) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = s_w[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t = fmaxf(t, s_w[w]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ float block_sum(float v, float* s_w) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = s_w[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += s_w[w];
    __syncthreads();
    return t;
}

// ---- pass A
__global__ __launch_bounds__(kT) void logprob_segments_kernel(const LpParams p) {
    __shared__ __attribute__((aligned(16))) float s_x[kChunk];
    __shared__ u64   s_list[2][kWaves][kMaxTop];   // a wave's best so far, descending, 0 = none; [cur] is read, [cur ^ 1] written
    __shared__ float s_w[kWaves];
    const int seg = blockIdx.x, row = blockIdx.y, tx = threadIdx.x, lane = tx & 63, wv = tx >> 6;
    const float* x = p.logits + (size_t)row * p.ld;
    const int lo = min(p.V, seg * p.seg), hi = min(p.V, lo + p.seg);
    const float inv_t = inv_temp(p, row);
    const bool vec = ((p.ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.logits) & 15) == 0);
    const int top_n = p.top_n;
    if (lane < kMaxTop) { s_list[0][wv][lane] = 0; s_list[1][wv][lane] = 0; }
    float m_run = -INFINITY, s_run = 0.f;
    int cur = 0;
    for (int c0 = lo; c0 < hi; c0 += kChunk) {      // lo and kChunk are multiples of 4: every chunk starts on a 16-byte boundary of an aligned row
        const int n = min(hi - c0, kChunk);
        int done = 0;
        if (vec) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x + c0);
            const int n4 = n >> 2;
#pragma unroll 4
            for (int j = tx; j < n4; j += kT) {
                const f32x4 v = x4[j];
                f32x4 o;
                o[0] = canon(v[0] * inv_t); o[1] = canon(v[1] * inv_t); o[2] = canon(v[2] * inv_t); o[3] = canon(v[3] * inv_t);
                *reinterpret_cast<f32x4*>(&s_x[4 * j]) = o;
            }
            done = n4 << 2;
        }
        for (int j = done + tx; j < n; j += kT) s_x[j] = canon(x[c0 + j] * inv_t);
        __syncthreads();
        float m = -INFINITY;
        for (int i = tx; i < n; i += kT) m = fmaxf(m, s_x[i]);
        const float m_new = fmaxf(m_run, block_max(m, s_w));
        float s = 0.f;
        if (m_new > -INFINITY)
            for (int i = tx; i < n; i += kT) s += expf(s_x[i] - m_new);
        s = block_sum(s, s_w);
        s_run = (m_run > -INFINITY ? s_run * expf(m_run - m_new) : 0.f) + s;   // one chunk: 0 + s
        m_run = m_new;
        if (top_n > 0) {
            // N rounds per wave over its entries of the chunk and its list so far: the best key below the previous pick
            u64 prev = ~0ull;
            for (int r = 0; r < top_n; ++r) {
                u64 best = 0;
                for (int i = tx; i < n; i += kT) {
                    const u64 k = key_of(s_x[i], c0 + i);
                    if (k < prev && k > best) best = k;
                }
                if (lane < kMaxTop) {
                    const u64 k = s_list[cur][wv][lane];
                    if (k < prev && k > best) best = k;
                }
                best = wave_max_u64(best);
                if (lane == 0) s_list[cur ^ 1][wv][r] = best;
                prev = best;
                if (best == 0) {                    // wave-uniform: nothing left, the rest of the list is empty
                    if (lane > r && lane < kMaxTop) s_list[cur ^ 1][wv][lane] = 0;
                    break;
                }
            }
            cur ^= 1;
        }
        __syncthreads();                            // s_x and the lists are rewritten by the next chunk
    }
    if (tx == 0) {
        float* ms = p.seg_ms + (size_t)row * 2 * kSegs;
        ms[seg] = m_run; ms[kSegs + seg] = s_run;
    }
    if (top_n > 0) {
        // the four lists by rank: keys are distinct, so the number of larger keys is the slot
        __syncthreads();
        const u64* all = &s_list[cur][0][0];
        u64* out = p.cand + ((size_t)row * kSegs + seg) * top_n;
        if (tx < kWaves * kMaxTop) {
            const u64 k = all[tx];
            int rank = 0, cnt = 0;
            for (int i = 0; i < kWaves * kMaxTop; ++i) { const u64 o = all[i]; rank += o > k ? 1 : 0; cnt += o != 0 ? 1 : 0; }
            if (k != 0 && rank < top_n) out[rank] = k;
            if (tx < top_n && tx >= cnt) out[tx] = 0;
        }
    }
}

// ---- pass B
__global__ __launch_bounds__(kT) void logprob_rows_kernel(const LpParams p) {
    __shared__ u64 s_k[kSegs * kMaxTop];
    const int row = blockIdx.x, tx = threadIdx.x;
    const float* ms = p.seg_ms + (size_t)row * 2 * kSegs;
    float M = ms[0];
#pragma unroll
    for (int s = 1; s < kSegs; ++s) M = fmaxf(M, ms[s]);
    float S = 0.f;
#pragma unroll
    for (int s = 0; s < kSegs; ++s) {
        const float m = ms[s];
        S += m > -INFINITY ? ms[kSegs + s] * expf(m - M) : 0.f;
    }
    const float lse = M + logf(S);
    // the column of this call: the recorder's, while it has room
    int col = 0;
    bool write = true;
    if (p.count) { col = p.count[row]; write = col >= 0 && col < p.log_ld; }
    const size_t slot = (size_t)row * p.log_ld + (write ? col : 0);
    if (tx == 0) {
        if (p.lse_out) p.lse_out[row] = lse;
        if (p.ids) {
            const int id = p.ids[row];
            float lp = __uint_as_float(0x7FC00000u);          // an id outside the row: NaN, nothing read
            if (id >= 0 && id < p.V) lp = canon(p.logits[(size_t)row * p.ld + id] * inv_temp(p, row)) - lse;
            if (write) p.token_lp[slot] = lp;
            if (p.cum) p.cum[row] += lp;
        }
    }
    const int top_n = p.top_n;
    if (top_n > 0 && write) {                                  // block-uniform
        const int total = kSegs * top_n;
        const u64* cand = p.cand + (size_t)row * total;
        for (int i = tx; i < total; i += kT) s_k[i] = cand[i];
        __syncthreads();
        int32_t* oi = p.top_ids + slot * p.top_ld;
        float*   ov = p.top_lp + slot * p.top_ld;
        for (int c = tx; c < total; c += kT) {                 // keys are distinct: the number of larger keys is the slot
            const u64 k = s_k[c];
            if (k == 0) continue;
            int rank = 0;
            for (int i = 0; i < total; ++i) rank += s_k[i] > k ? 1 : 0;
            if (rank < top_n) { oi[rank] = key_index(k); ov[rank] = key_value(k) - lse; }
        }
        if (tx < top_n) {                                      // slots beyond the entries the row has
            int cnt = 0;
            for (int i = 0; i < total; ++i) cnt += s_k[i] != 0 ? 1 : 0;
            if (tx >= cnt) { oi[tx] = -1; ov[tx] = -INFINITY; }
        }
    }
    if (p.count && write) {
        __syncthreads();                                       // every thread has read count[row]
        if (tx == 0) p.count[row] = col + 1;
    }
}

size_t ws_ms_bytes(int rows) { return (((size_t)rows * 2 * kSegs * sizeof(float)) + 255) & ~(size_t)255; }
size_t ws_total(int rows, int top_n) { return ws_ms_bytes(rows) + (size_t)rows * kSegs * top_n * sizeof(u64); }

int fill_common(LpParams& p, const char* who, const float* logits, int rows, int V, int ld, const float* temperature, int top_n,
                void* workspace, size_t workspace_bytes) {
    MI355_CHECK_ARG(logits, "%s: logits is null", who);
    MI355_CHECK_ARG(rows > 0 && rows <= 65535 && V > 0, "%s: rows=%d V=%d", who, rows, V);
    MI355_CHECK_ARG(ld >= V, "%s: ld %d < V %d", who, ld, V);
    MI355_CHECK_ARG(top_n >= 0 && top_n <= kMaxTop, "%s: top_n %d outside [0, %d]", who, top_n, kMaxTop);
    const size_t need = ws_total(rows, top_n);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
        mi355_set_error("%s: workspace of %zu bytes (8-byte aligned) needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
        return MI355_ERR_WORKSPACE;
    }
    p.logits = logits; p.rows = rows; p.V = V; p.ld = ld;
    p.seg = (((V + kSegs - 1) / kSegs) + 3) & ~3;
    p.temperature = temperature; p.top_n = top_n;
    p.seg_ms = (float*)workspace;
    p.cand = (u64*)((char*)workspace + ws_ms_bytes(rows));
    return MI355_OK;
}
int check_outputs(const float* logits, const int32_t* ids, int top_n, const float* token_logprobs, const int32_t* top_ids,
                  const float* top_logprobs, int top_ld) {
    MI355_CHECK_ARG(logits, "logprobs: logits is null");
    MI355_CHECK_ARG(top_n >= 0 && top_n <= kMaxTop, "logprobs: top_n %d outside [0, %d]", top_n, kMaxTop);
    MI355_CHECK_ARG(!ids || token_logprobs, "logprobs: ids without token_logprobs");
    MI355_CHECK_ARG(top_n == 0 || (top_ids && top_logprobs), "logprobs: top_n %d needs top_ids and top_logprobs", top_n);
    MI355_CHECK_ARG(top_n == 0 || top_ld >= top_n, "logprobs: top_ld %d < top_n %d", top_ld, top_n);
    return MI355_OK;
}

} // namespace

extern "C" size_t mi355_logprobs_workspace_bytes(int32_t rows, int32_t V, int32_t top_n) {
    (void)V;
    if (rows <= 0 || top_n < 0 || top_n > kMaxTop) return 0;
    return ws_total(rows, top_n);
}

extern "C" int mi355_logprobs_segments(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature, int32_t top_n,
                                       void* workspace, size_t workspace_bytes, mi355_stream_t stream) {
    if (rows == 0) return MI355_OK;
    LpParams p{};
    if (int e = fill_common(p, "logprobs", logits, rows, V, ld, temperature, top_n, workspace, workspace_bytes)) return e;
    hipLaunchKernelGGL(logprob_segments_kernel, dim3(kSegs, rows), dim3(kT), 0, (hipStream_t)stream, p);
    MI355_CHECK_LAUNCH("logprob_segments_kernel");
    return MI355_OK;
}

extern "C" int mi355_logprobs_rows(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature, const int32_t* ids,
                                   int32_t top_n, float* token_logprobs, float* lse_out, int32_t* top_ids, float* top_logprobs,
                                   int32_t top_ld, int32_t log_ld, int32_t* count, float* cum_log_probs, void* workspace,
                                   size_t workspace_bytes, mi355_stream_t stream) {
    if (rows == 0) return MI355_OK;
    LpParams p{};
    if (int e = fill_common(p, "logprobs", logits, rows, V, ld, temperature, top_n, workspace, workspace_bytes)) return e;
    if (int e = check_outputs(logits, ids, top_n, token_logprobs, top_ids, top_logprobs, top_ld)) return e;
    MI355_CHECK_ARG(log_ld >= 1, "logprobs: log_ld %d", log_ld);
    p.ids = ids; p.token_lp = token_logprobs; p.lse_out = lse_out; p.top_ids = top_ids; p.top_lp = top_logprobs;
    p.top_ld = top_ld; p.log_ld = log_ld; p.count = count; p.cum = cum_log_probs;
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(rows), dim3(kT), 0, (hipStream_t)stream, p);
    MI355_CHECK_LAUNCH("logprob_rows_kernel");
    return MI355_OK;
}

extern "C" int mi355_logprobs(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature, const int32_t* ids,
                              int32_t top_n, float* token_logprobs, float* lse_out, int32_t* top_ids, float* top_logprobs, int32_t top_ld,
                              void* workspace, size_t workspace_bytes, mi355_stream_t stream) {
    if (rows == 0) return MI355_OK;
    if (int e = check_outputs(logits, ids, top_n, token_logprobs, top_ids, top_logprobs, top_ld)) return e;   // before the first launch
    if (int e = mi355_logprobs_segments(logits, rows, V, ld, temperature, top_n, workspace, workspace_bytes, stream)) return e;
    return mi355_logprobs_rows(logits, rows, V, ld, temperature, ids, top_n, token_logprobs, lse_out, top_ids, top_logprobs, top_ld, 1,
                               nullptr, nullptr, workspace, workspace_bytes, stream);
}
