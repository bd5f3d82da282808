// The sampling tail of a decode step as one fused op on fp32 logit rows, gfx950: temperature, softmax, top-k / top-p filter and the
// inverse-CDF draw (mi355_sample_logits), the penalties over a device-side token history (mi355_apply_penalties_history) and the
// feedback of the drawn ids into the step's inputs (mi355_sample_feedback).  Everything a launch needs is read from device memory when
// it runs, so a captured step stays valid while the host rewrites the parameter arrays and the history grows.
//
// Same result as the chain mi355_apply_penalties(temperature) -> mi355_softmax_rows -> mi355_top_k_top_p_sample (sampling.hip), which
// walks a row 33 times with one block: here a row is cut into kSegs segments whatever the batch, the grid is (segment, row), and
// the segments meet across kernel boundaries only.  With x = logit * inv_t, m = max x and e = exp(x - m) (one fp32 expression,
// evaluated identically by every pass), an entry's KEY is the bit pattern of e (non-negative floats order like their bits) and its
// MASS is floor(e * 2^40) as an integer.  All sums of the filter and of the draw are sums of masses: integer addition is
// associative, so the result does not depend on how a row is cut, on the order in which blocks arrive (the row histograms are filled
// with integer atomics) or on the number of rows -- bitwise reproducible without any ordered float sum (and no float atomics).
// 2^40 leaves 2^-41 per entry, 2^-23 over a 152064-wide row, and fits 2^23 entries of mass 2^40 into 63 bits.
//
// Both thresholds come out of ONE three-level radix select over the key (11 + 10 + 10 bits): per level a histogram launch (count and
// mass per bin, of the entries under the prefixes chosen so far) and a one-block-per-row select launch that walks the bins from the top.
//   top-k : the key of the k-th largest entry (ties with it stay);
//   top-p : the smallest key v whose mass of strictly larger entries A(v) is <= p Z (Z = mass of the whole row, NOT renormalised after
//           top-k), and how many of its equals stay: the j-th occurrence in index order stays while A + j mass(v) <= p Z.
// The kept set is {key > T} + the first c entries with key == T in index order, T = the larger of the two thresholds.  Exact for
// every input: a flat row, a row of equal values and a nucleus of 10^5 entries all take the same three levels; nothing is compacted.
// Then one launch sums the kept mass per segment and the last one locates u * (kept mass) -- segment, thread, entry -- and writes the
// renormalised survivors.  A row with top_k == 1 skips all of it: its id is the arg-max of the raw logits, lowest index on ties.
#include "common.h"
#include "internal.h"

namespace {

constexpr int kSegs = 32;             // segments per row: fixed, so that the cut of a row never depends on the batch
constexpr int kT = 256;               // threads of the (segment, row) launches and of the select launch
constexpr int kBins0 = 2048, kBins = 1024;
constexpr float kMassScale = 1099511627776.0f;   // 2^40
typedef unsigned long long u64;

struct RowHist {                      // one level of one row; zero on entry (zero_fill launch ahead of the launches)
    uint32_t cnt_p[kBins0];
    uint32_t cnt_k[kBins0];
    u64      mass_p[kBins0];
};
struct RowState {
    float    m, inv_t, u;
    int32_t  greedy, amax, use_k, use_p, pad;
    uint32_t pk, pp, krem, T;
    u64      mabove, Z, mT;
    double   thr;
    long long c;                      // entries with key == T that stay (index order)
};
struct SegOut {
    float    max_x[kSegs];
    float    arg_v[kSegs];
    int32_t  arg_i[kSegs];
    uint32_t ties[kSegs];
    u64      strict[kSegs];
};

struct SampleParams {
    const float*    logits;
    int             rows, V, ld, seg;           // seg: entries per segment, a multiple of 4
    const float*    temperature;
    const int32_t*  top_k;
    const float*    top_p;
    const float*    uniform;
    const uint64_t* seed;
    const int32_t*  positions;
    int             pos_add;
    int32_t*        ids;
    float*          uniform_out;
    float*          probs_out;
    int             ld_out;
    RowHist*        hist;                       // [rows][3]
    RowState*       state;                      // [rows]
    SegOut*         segs;                       // [rows]
};

__device__ __forceinline__ bool row_vec(const SampleParams& p) {
    return ((p.ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.logits) & 15) == 0);
}
// the one expression every pass evaluates (the library is built with -ffp-contract=off: multiply, subtract and exp round separately,
// as the chain's temperature launch and softmax do)
__device__ __forceinline__ float weight_of(float raw, float inv_t, float m) {
    const float e = expf(raw * inv_t - m);   // the accurate one: the tail of an unfiltered row sits 60 below the maximum
    return e > 0.f ? e : 0.f;                   // NaN -> 0: never kept, never indexes past a histogram
}
__device__ __forceinline__ u64 mass_of(float e) { return (u64)(e * kMassScale); }

// f(j, raw) for every entry of [lo, hi) by the whole block, 16-byte loads, four in flight per thread (lo is a multiple of 4)
template <class F>
__device__ __forceinline__ void seg_pass(const float* __restrict__ x, int lo, int hi, bool vec, F&& f) {
    const int tx = threadIdx.x;
    int done = lo;
    if (vec && hi > lo) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x + lo);
        const int n4 = (hi - lo) >> 2;
#pragma unroll 4
        for (int j = tx; j < n4; j += kT) {
            const f32x4 v = x4[j];
            const int b = lo + 4 * j;
            f(b, v[0]); f(b + 1, v[1]); f(b + 2, v[2]); f(b + 3, v[3]);
        }
        done = lo + (n4 << 2);
    }
    for (int j = done + tx; j < hi; j += kT) f(j, x[j]);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}
// sum over the block, result in every thread (integers: any order gives the same bits)
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < kT / 64; ++w) t += s_w[w];
    __syncthreads();
    return t;
}
// exclusive prefix over the threads of the block (Hillis-Steele in LDS), total in *total
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* s_scan, u64* total) {
    const int tx = threadIdx.x;
    s_scan[tx] = v;
    __syncthreads();
    for (int off = 1; off < kT; off <<= 1) {
        const u64 add = (tx >= off) ? s_scan[tx - off] : 0;
        __syncthreads();
        s_scan[tx] += add;
        __syncthreads();
    }
    const u64 incl = s_scan[tx];
    *total = s_scan[kT - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ void arg_combine(float& v, int& i, float ov, int oi) {   // argmax_combine of elementwise.hip
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ bool greedy_row(const SampleParams& p, int row) { return p.top_k && p.top_k[row] == 1; }
__device__ __forceinline__ float inv_temp(const SampleParams& p, int row) {
    return p.temperature ? 1.0f / (p.temperature[row] + 1e-6f) : 1.0f;
}
__device__ __forceinline__ float row_max(const SegOut& so) {
    float m = so.max_x[0];
#pragma unroll
    for (int s = 1; s < kSegs; ++s) m = fmaxf(m, so.max_x[s]);
    return m;
}

// ---- launch 1: per segment, max of the scaled logits and arg-max of the raw ones
__global__ __launch_bounds__(kT) void seg_max_kernel(const SampleParams p) {
    __shared__ float s_m[kT / 64], s_v[kT / 64];
    __shared__ int   s_i[kT / 64];
    const int seg = blockIdx.x, row = blockIdx.y, tx = threadIdx.x;
    const float* x = p.logits + (size_t)row * p.ld;
    const int lo = min(p.V, seg * p.seg), hi = min(p.V, lo + p.seg);
    const float inv_t = inv_temp(p, row);
    float m = -INFINITY, bv = -INFINITY;
    int bi = 0x7fffffff;
    seg_pass(x, lo, hi, row_vec(p), [&](int j, float raw) {
        m = fmaxf(m, raw * inv_t);
        arg_combine(bv, bi, raw, j);
    });
    m = wave_max(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) arg_combine(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
    if ((tx & 63) == 0) { s_m[tx >> 6] = m; s_v[tx >> 6] = bv; s_i[tx >> 6] = bi; }
    __syncthreads();
    if (tx == 0) {
        for (int w = 1; w < kT / 64; ++w) { m = fmaxf(m, s_m[w]); arg_combine(bv, bi, s_v[w], s_i[w]); }
        SegOut& so = p.segs[row];
        so.max_x[seg] = m; so.arg_v[seg] = bv; so.arg_i[seg] = bi;
    }
}

// ---- histogram launch of level L: bins of 11 / 10 / 10 key bits under the prefixes the select launches chose
template <int L>
__global__ __launch_bounds__(kT) void hist_kernel(const SampleParams p) {
    constexpr int NB = L == 0 ? kBins0 : kBins;
    __shared__ uint32_t s_cp[NB], s_ck[NB];
    __shared__ u64      s_mp[NB];
    const int seg = blockIdx.x, row = blockIdx.y, tx = threadIdx.x;
    if (greedy_row(p, row)) return;
    const int lo = min(p.V, seg * p.seg), hi = min(p.V, lo + p.seg);
    if (lo >= hi) return;
    float m, inv_t;
    bool use_k = false, use_p = true;
    uint32_t pk = 0, pp = 0;
    if (L == 0) {
        m = row_max(p.segs[row]); inv_t = inv_temp(p, row);
    } else {
        const RowState& st = p.state[row];
        use_k = st.use_k != 0; use_p = st.use_p != 0;
        if (!use_k && !use_p) return;
        m = st.m; inv_t = st.inv_t; pk = st.pk; pp = st.pp;
        if (use_k && use_p && pk == pp) use_k = false;          // one histogram serves both (the select launch reads cnt_p)
    }
    for (int b = tx; b < NB; b += kT) { s_cp[b] = 0; s_ck[b] = 0; s_mp[b] = 0; }
    __syncthreads();
    const float* x = p.logits + (size_t)row * p.ld;
    seg_pass(x, lo, hi, row_vec(p), [&](int, float raw) {
        const float e = weight_of(raw, inv_t, m);
        const uint32_t key = __float_as_uint(e);
        if (L == 0) {
            const uint32_t b = min(key >> 20, (uint32_t)NB - 1);
            atomicAdd(&s_cp[b], 1u);
            atomicAdd(&s_mp[b], mass_of(e));
        } else {
            const uint32_t hi_bits = L == 1 ? key >> 20 : key >> 10;
            const uint32_t b = (L == 1 ? key >> 10 : key) & (NB - 1);
            if (use_p && hi_bits == pp) { atomicAdd(&s_cp[b], 1u); atomicAdd(&s_mp[b], mass_of(e)); }
            if (use_k && hi_bits == pk) atomicAdd(&s_ck[b], 1u);
        }
    });
    __syncthreads();
    RowHist& h = p.hist[(size_t)row * 3 + L];
    for (int b = tx; b < NB; b += kT) {
        if (s_cp[b]) { atomicAdd(&h.cnt_p[b], s_cp[b]); if (s_mp[b]) atomicAdd(&h.mass_p[b], s_mp[b]); }
        if (s_ck[b]) atomicAdd(&h.cnt_k[b], s_ck[b]);
    }
}

// Philox4x32-10 (Salmon et al., SC'11; Random123): counter (position, 0, 0, 0), key = the two words of the seed
__device__ __forceinline__ uint32_t philox_x0(uint64_t seed, uint32_t position) {
    uint32_t c0 = position, c1 = 0, c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// ---- select launch of level L, one block per row: walk the bins from the top
template <int L>
__global__ __launch_bounds__(kT) void select_kernel(const SampleParams p) {
    constexpr int NB = L == 0 ? kBins0 : kBins, PER = NB / kT, SHIFT = L == 0 ? 0 : 10;
    __shared__ u64 s_w[kT / 64];
    __shared__ u64 s_scan[kT];
    __shared__ int s_best;
    __shared__ uint32_t s_pk, s_pp, s_cnt_b;      // what this level chose, for the closing step of the last level
    __shared__ u64 s_mabove, s_mass_b;
    const int row = blockIdx.x, tx = threadIdx.x;
    RowState& st = p.state[row];
    const RowHist& h = p.hist[(size_t)row * 3 + L];
    if (L == 0) {
        const SegOut& so = p.segs[row];
        if (tx == 0) {
            float bv = so.arg_v[0]; int bi = so.arg_i[0];
            for (int s = 1; s < kSegs; ++s) arg_combine(bv, bi, so.arg_v[s], so.arg_i[s]);
            st.amax = bi < p.V ? bi : 0;
            st.greedy = greedy_row(p, row) ? 1 : 0;
            st.m = row_max(so); st.inv_t = inv_temp(p, row);
            float u;
            if (p.uniform) u = p.uniform[row];
            else u = (float)(philox_x0(p.seed[row], (uint32_t)(p.positions[row] + p.pos_add)) >> 8) * 5.9604644775390625e-08f;   // 2^-24
            st.u = u;
            if (p.uniform_out) p.uniform_out[row] = u;
        }
        if (greedy_row(p, row)) return;
    } else {
        if (st.greedy || (!st.use_k && !st.use_p)) return;
    }
    // the state of the level above (block-uniform reads; written below only after the last of them, behind a barrier)
    bool use_k, use_p;
    uint32_t pk = 0, pp = 0, krem = 0;
    u64 mabove = 0;
    double thr = 0.0;
    if (L == 0) {
        u64 z = 0;
        for (int b = tx; b < NB; b += kT) z += h.mass_p[b];
        const u64 Z = block_sum_u64(z, s_w);
        const int k = p.top_k ? p.top_k[row] : 0;
        use_k = k > 0 && k < p.V;
        krem = use_k ? (uint32_t)k : 0u;
        float tp = p.top_p ? p.top_p[row] : 1.0f;
        if (fabsf(tp) < 1e-7f) tp = 1.0f;
        use_p = fabsf(tp - 1.0f) >= 1e-7f;
        thr = fmax((double)tp * (double)Z, 0.0);
        if (tx == 0) { st.Z = Z; st.thr = thr; }
    } else {
        use_k = st.use_k != 0; use_p = st.use_p != 0; pk = st.pk; pp = st.pp; krem = st.krem; mabove = st.mabove; thr = st.thr;
    }
    const bool k_from_p = L == 0 || (use_k && use_p && pk == pp);
    const uint32_t* ck_src = k_from_p ? h.cnt_p : h.cnt_k;
    // thread tx owns the descending positions [tx PER, tx PER + PER): bin = NB - 1 - position
    uint32_t ck[PER], cp[PER];
    u64 mp[PER];
    u64 sum_k = 0, sum_m = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int b = NB - 1 - (tx * PER + i);
        ck[i] = use_k ? ck_src[b] : 0u; cp[i] = use_p ? h.cnt_p[b] : 0u; mp[i] = use_p ? h.mass_p[b] : 0;
        sum_k += ck[i]; sum_m += mp[i];
    }
    if (tx == 0) s_best = -1;
    u64 tot;
    u64 run_k = block_excl_scan(sum_k, s_scan, &tot);
    u64 run_m = mabove + block_excl_scan(sum_m, s_scan, &tot);
    __syncthreads();   // every read of st above is done
    int mine = -1;
    u64 mine_above = 0, mine_mass = 0;
    uint32_t mine_cnt = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int b = NB - 1 - (tx * PER + i);
        if (use_k && run_k < krem && krem <= run_k + ck[i]) {           // the k-th largest lies in this bin: exactly one (thread, i)
            st.pk = s_pk = (pk << SHIFT) | (uint32_t)b;
            st.krem = krem - (uint32_t)run_k;
        }
        if (use_p && cp[i] > 0 && (double)run_m <= thr) {               // its largest value has A = run_m <= p Z: that one stays
            mine = tx * PER + i; mine_above = run_m; mine_cnt = cp[i]; mine_mass = mp[i];
        }
        run_k += ck[i]; run_m += mp[i];
    }
    if (mine >= 0) atomicMax(&s_best, mine);
    __syncthreads();
    const int best = s_best;   // the LOWEST bin with a survivor (the candidates are a run from the top: run_m only grows)
    if (use_p && mine >= 0 && mine == best) {
        st.pp = s_pp = (pp << SHIFT) | (uint32_t)(NB - 1 - best);
        st.mabove = s_mabove = mine_above; s_cnt_b = mine_cnt; s_mass_b = mine_mass;
    }
    if (use_p && best < 0) use_p = false;   // cannot happen (the largest entry has A = 0 <= thr); never leave a stale prefix in use
    if (tx == 0) {
        if (L == 0) { st.use_k = use_k ? 1 : 0; if (!use_k) { st.pk = 0; st.krem = 0; } }
        if (L == 0 || !use_p) st.use_p = use_p ? 1 : 0;
    }
    if (L != 2) return;
    __syncthreads();
    if (tx != 0) return;
    // both thresholds are whole keys now
    uint32_t T = 0;
    long long c = 0x7fffffffffffffffLL;     // every equal of T stays
    if (use_p) {
        const uint32_t vb = s_pp, cnt = s_cnt_b;
        const u64 S = s_mabove, mv = cnt ? s_mass_b / cnt : 0;   // the bin is one value: equal masses
        long long cp_keep = cnt;
        if (mv > 0) {
            const double room = (thr - (double)S) / (double)mv;    // the j-th equal stays while S + j mv <= p Z
            cp_keep = room >= (double)cnt ? (long long)cnt : (long long)room + 1;
            if (cp_keep < 1) cp_keep = 1;
        }
        T = vb;
        if (cp_keep < (long long)cnt) c = cp_keep;
    }
    if (use_k) {
        const uint32_t tk = s_pk;
        if (!use_p || tk > T) { T = tk; c = 0x7fffffffffffffffLL; }
    }
    st.T = T; st.c = c; st.mT = mass_of(__uint_as_float(T));
}

// ---- kept mass per segment: strictly above T, and the number of equals of T
__global__ __launch_bounds__(kT) void seg_mass_kernel(const SampleParams p) {
    __shared__ u64 s_w[kT / 64];
    const int seg = blockIdx.x, row = blockIdx.y;
    const RowState& st = p.state[row];
    if (st.greedy) return;
    const int lo = min(p.V, seg * p.seg), hi = min(p.V, lo + p.seg);
    const float m = st.m, inv_t = st.inv_t;
    const bool filt = st.use_k || st.use_p;
    const uint32_t T = filt ? st.T : 0u;
    u64 strict = 0, ties = 0;
    seg_pass(p.logits + (size_t)row * p.ld, lo, hi, row_vec(p), [&](int, float raw) {
        const float e = weight_of(raw, inv_t, m);
        const uint32_t key = __float_as_uint(e);
        strict += key > T ? mass_of(e) : 0;
        ties += key == T ? 1 : 0;
    });
    strict = block_sum_u64(strict, s_w);
    ties = block_sum_u64(ties, s_w);
    if (threadIdx.x == 0) { p.segs[row].strict[seg] = strict; p.segs[row].ties[seg] = (uint32_t)ties; }
}

// ---- the draw: locate u * (kept mass) by segment, thread and entry, all in index order; renormalised survivors out
__global__ __launch_bounds__(kT) void draw_kernel(const SampleParams p) {
    __shared__ u64 s_scan[kT];
    const int seg = blockIdx.x, row = blockIdx.y, tx = threadIdx.x;
    const RowState& st = p.state[row];
    const int lo = min(p.V, seg * p.seg), hi = min(p.V, lo + p.seg);
    float* y = p.probs_out ? p.probs_out + (size_t)row * p.ld_out : nullptr;
    if (st.greedy) {
        if (seg == 0 && tx == 0) p.ids[row] = st.amax;
        if (y) for (int j = lo + tx; j < hi; j += kT) y[j] = j == st.amax ? 1.0f : 0.0f;
        return;
    }
    const bool filt = st.use_k || st.use_p;
    const uint32_t T = filt ? st.T : 0u;
    const long long c = filt ? st.c : 0x7fffffffffffffffLL;
    const u64 mT = filt ? st.mT : 0;
    const float m = st.m, inv_t = st.inv_t;
    const SegOut& so = p.segs[row];
    // kept mass of every segment: its equals of T carry the ranks [base, base + ties) of the row
    u64 K = 0, before = 0, mine_kept = 0;
    long long base = 0, my_base = 0;
    for (int s = 0; s < kSegs; ++s) {
        const long long t = so.ties[s];
        long long keep = c - base; keep = keep < 0 ? 0 : (keep > t ? t : keep);
        const u64 kept = so.strict[s] + (u64)keep * mT;
        if (s == seg) { before = K; my_base = base; mine_kept = kept; }
        K += kept; base += t;
    }
    u64 target = (u64)((double)st.u * (double)K);
    if (K > 0 && target >= K) target = K - 1;
    const bool holds = K > 0 && target >= before && target < before + mine_kept;   // exactly one segment
    if (K == 0 && seg == 0 && tx == 0) p.ids[row] = st.amax;                       // a row without any weight (all NaN)
    if (!holds && !y) return;
    // thread tx owns the contiguous entries [a, b) of the segment: the prefix over threads is the prefix over indices
    const int chunk = (((hi - lo + kT - 1) / kT) + 3) & ~3;
    const int a = min(hi, lo + tx * chunk), b = min(hi, a + chunk);
    const float* x = p.logits + (size_t)row * p.ld;
    const bool rank = c < base;                      // some equals of T are dropped: rank them
    u64 tot;
    long long r0 = my_base;
    if (rank) {
        u64 t = 0;
        for (int j = a; j < b; ++j) t += __float_as_uint(weight_of(x[j], inv_t, m)) == T ? 1 : 0;
        r0 += (long long)block_excl_scan(t, s_scan, &tot);
    }
    auto kept_mass = [&](float e, long long& r) -> u64 {       // in index order: r = rank of the next equal of T
        const uint32_t key = __float_as_uint(e);
        if (key > T) return mass_of(e);
        if (key == T) { const bool in = !rank || r < c; ++r; return in ? mass_of(e) : 0; }
        return 0;
    };
    const float den = fmaxf((float)((double)K * 9.094947017729282e-13), 1e-10f);   // 2^-40
    u64 local = 0;
    long long r = r0;
    for (int j = a; j < b; ++j) {
        const float e = weight_of(x[j], inv_t, m);
        const uint32_t key = __float_as_uint(e);
        const long long rb = r;
        const u64 w = kept_mass(e, r);
        local += w;
        if (y) y[j] = (key > T || (key == T && (!rank || rb < c))) ? e / den : 0.f;
    }
    if (!holds) return;                               // block-uniform
    const u64 excl = block_excl_scan(local, s_scan, &tot);
    const u64 t_loc = target - before;
    if (local > 0 && excl <= t_loc && t_loc < excl + local) {   // exactly one thread
        u64 run = excl;
        r = r0;
        int found = a;
        for (int j = a; j < b; ++j) {
            run += kept_mass(weight_of(x[j], inv_t, m), r);
            if (run > t_loc) { found = j; break; }
        }
        p.ids[row] = found;
    }
}

// ---- penalties over a device-side history (penalties_kernel of sampling.hip without the temperature, lengths read here)
struct HistoryPenaltyParams {
    float*         logits;
    int            V, ld;
    const float   *repetition, *presence, *frequency;
    const int32_t* history;
    int            history_ld;
    const int32_t* history_len;
    int32_t*       counts;         // [rows][V], zero on entry
};
constexpr int kPenThreads = 1024;

__global__ __launch_bounds__(kPenThreads) void history_penalties_kernel(const HistoryPenaltyParams p) {
    const int row = blockIdx.x, tx = threadIdx.x;
    float* x = p.logits + (size_t)row * p.ld;
    int32_t* cnt = p.counts + (size_t)row * p.V;
    const int32_t* hist = p.history + (size_t)row * p.history_ld;
    const int n = max(0, min(p.history_len[row], p.history_ld));
    const float rep = p.repetition ? p.repetition[row] : 1.0f, pres = p.presence ? p.presence[row] : 0.0f,
                freq = p.frequency ? p.frequency[row] : 0.0f;
    auto penalise = [&](int j, int c) {
        float logit = x[j];
        if (p.repetition) logit = logit < 0.0f ? logit * rep : logit / rep;
        if (p.presence) logit -= pres;
        if (p.frequency) logit -= freq * (float)c;
        x[j] = logit;
    };
    // count the ids of the history; the lane whose increment found a zero owns the id and penalises it once the counts are final:
    // work proportional to the history (beyond 32 entries per lane: a scan of the row)
    uint32_t mine = 0;
    int s = 0;
    for (int index = tx; index < n; index += kPenThreads, ++s) {
        const int tok = hist[index];
        if (tok >= p.V || tok < 0) continue;
        const int old = atomicAdd(&cnt[tok], 1);
        if (old == 0 && s < 32) mine |= 1u << s;
    }
    __syncthreads();
    if (n <= 32 * kPenThreads) {
        s = 0;
        for (int index = tx; index < n; index += kPenThreads, ++s) {
            if (!((mine >> s) & 1u)) continue;
            const int tok = hist[index];
            penalise(tok, __hip_atomic_load(&cnt[tok], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
    } else {
        for (int j = tx; j < p.V; j += kPenThreads) {
            const int c = __hip_atomic_load(&cnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c > 0) penalise(j, c);
        }
    }
}

// ---- feedback of a sampled step: positions + 1, and the drawn id appended to the history (saturating at history_ld)
__global__ __launch_bounds__(64) void sample_feedback_kernel(const int32_t* __restrict__ ids, int B, int32_t* __restrict__ positions,
                                                             int32_t* __restrict__ history, int32_t* __restrict__ history_len, int history_ld) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (positions) positions[b] += 1;
    if (history && history_len) {
        const int n = history_len[b];
        if (n >= 0 && n < history_ld) { history[(size_t)b * history_ld + n] = ids[b]; history_len[b] = n + 1; }
    }
}

// Zero `bytes` (a multiple of 4, 4-byte aligned) with a launch of its own.  Not hipMemsetAsync: as a memset NODE of a captured step that also holds
// the all-reduce launches of a tensor-parallel rank, it was observed to fill its range with a repeating 16-byte garbage pattern on every other
// replay (the eager step was right every time) -- the histograms and the penalty counts then start a step non-zero.  A kernel node has no such state.
__global__ __launch_bounds__(256) void zero_fill_kernel(uint32_t* __restrict__ p, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) p[i] = 0u;
}
bool zero_fill(void* ptr, size_t bytes, hipStream_t st) {
    const size_t n4 = bytes / 4;
    if (n4 == 0) return true;
    const size_t want = (n4 + 255) / 256;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, st, (uint32_t*)ptr, n4);
    return hipGetLastError() == hipSuccess;
}

struct WsLayout { size_t hist, state, segs, total; };
WsLayout ws_layout(int rows) {
    WsLayout w;
    w.hist = 0;
    w.state = (size_t)rows * 3 * sizeof(RowHist);
    w.segs = w.state + (((size_t)rows * sizeof(RowState) + 255) & ~(size_t)255);
    w.total = w.segs + (((size_t)rows * sizeof(SegOut) + 255) & ~(size_t)255);
    return w;
}

} // namespace

extern "C" size_t mi355_sample_logits_workspace_bytes(int32_t rows, int32_t V) {
    (void)V;
    return rows > 0 ? ws_layout(rows).total : 0;
}

extern "C" int mi355_sample_logits_ex(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature,
                                      const int32_t* top_k, const float* top_p, const float* uniform_samples, const uint64_t* seed,
                                      const int32_t* draw_positions, int32_t position_add, int32_t* ids, float* uniform_out,
                                      float* probs_out, int32_t ld_out, void* workspace, size_t workspace_bytes, mi355_stream_t stream) {
    if (rows == 0) return MI355_OK;
    MI355_CHECK_ARG(logits, "sample_logits: logits is null");
    MI355_CHECK_ARG(ids, "sample_logits: ids is null");
    MI355_CHECK_ARG(rows > 0 && rows <= 65535 && V > 0, "sample_logits: rows=%d V=%d", rows, V);
    MI355_CHECK_ARG(ld >= V, "sample_logits: ld %d < V %d", ld, V);
    MI355_CHECK_ARG(uniform_samples || (seed && draw_positions),
                    "sample_logits: needs uniform_samples, or seed and draw_positions for the Philox draw");
    MI355_CHECK_ARG(!probs_out || ld_out >= V, "sample_logits: ld_out %d < V %d", ld_out, V);
    const WsLayout w = ws_layout(rows);
    if (!workspace || workspace_bytes < w.total || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
        mi355_set_error("sample_logits: workspace of %zu bytes (8-byte aligned) needed, %zu given", w.total, workspace ? workspace_bytes : (size_t)0);
        return MI355_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)workspace;
    if (!zero_fill(base + w.hist, w.state - w.hist, st)) {
        mi355_set_error("sample_logits: the zero-fill launch failed");
        return MI355_ERR_HIP;
    }
    SampleParams p{};
    p.logits = logits; p.rows = rows; p.V = V; p.ld = ld;
    p.seg = (((V + kSegs - 1) / kSegs) + 3) & ~3;
    p.temperature = temperature; p.top_k = top_k; p.top_p = top_p; p.uniform = uniform_samples; p.seed = seed;
    p.positions = draw_positions; p.pos_add = position_add; p.ids = ids; p.uniform_out = uniform_out; p.probs_out = probs_out;
    p.ld_out = ld_out;
    p.hist = (RowHist*)(base + w.hist); p.state = (RowState*)(base + w.state); p.segs = (SegOut*)(base + w.segs);
    const dim3 grid(kSegs, rows), row_grid(rows), block(kT);
    hipLaunchKernelGGL(seg_max_kernel, grid, block, 0, st, p);
    hipLaunchKernelGGL(hist_kernel<0>, grid, block, 0, st, p);
    hipLaunchKernelGGL(select_kernel<0>, row_grid, block, 0, st, p);
    hipLaunchKernelGGL(hist_kernel<1>, grid, block, 0, st, p);
    hipLaunchKernelGGL(select_kernel<1>, row_grid, block, 0, st, p);
    hipLaunchKernelGGL(hist_kernel<2>, grid, block, 0, st, p);
    hipLaunchKernelGGL(select_kernel<2>, row_grid, block, 0, st, p);
    hipLaunchKernelGGL(seg_mass_kernel, grid, block, 0, st, p);
    hipLaunchKernelGGL(draw_kernel, grid, block, 0, st, p);
    MI355_CHECK_LAUNCH("sample_logits");
    return MI355_OK;
}

extern "C" int mi355_sample_logits(const float* logits, int32_t rows, int32_t V, int32_t ld, const float* temperature,
                                   const int32_t* top_k, const float* top_p, const float* uniform_samples, const uint64_t* seed,
                                   const int32_t* draw_positions, int32_t* ids, float* uniform_out, float* probs_out, int32_t ld_out,
                                   void* workspace, size_t workspace_bytes, mi355_stream_t stream) {
    return mi355_sample_logits_ex(logits, rows, V, ld, temperature, top_k, top_p, uniform_samples, seed, draw_positions, 0, ids,
                                  uniform_out, probs_out, ld_out, workspace, workspace_bytes, stream);
}

extern "C" int mi355_apply_penalties_history(float* logits, int32_t rows, int32_t V, int32_t ld, const float* repetition_penalty,
                                             const float* presence_penalty, const float* frequency_penalty, const int32_t* history,
                                             int32_t history_ld, const int32_t* history_len, int32_t* penalty_ws, mi355_stream_t stream) {
    if (rows == 0) return MI355_OK;
    MI355_CHECK_ARG(logits, "apply_penalties_history: logits is null");
    MI355_CHECK_ARG(rows > 0 && V > 0 && ld >= V, "apply_penalties_history: rows=%d V=%d ld=%d", rows, V, ld);
    if (!repetition_penalty && !presence_penalty && !frequency_penalty) return MI355_OK;
    MI355_CHECK_ARG(history && history_len && history_ld > 0,
                    "apply_penalties_history: penalties need history [rows][history_ld] and history_len [rows]");
    MI355_CHECK_ARG(penalty_ws, "apply_penalties_history: penalty_ws [rows][V] int32 is null");
    if (!zero_fill(penalty_ws, (size_t)rows * V * sizeof(int32_t), (hipStream_t)stream)) {
        mi355_set_error("apply_penalties_history: the zero-fill launch failed");
        return MI355_ERR_HIP;
    }
    HistoryPenaltyParams p{logits, V, ld, repetition_penalty, presence_penalty, frequency_penalty, history, history_ld, history_len, penalty_ws};
    hipLaunchKernelGGL(history_penalties_kernel, dim3(rows), dim3(kPenThreads), 0, (hipStream_t)stream, p);
    MI355_CHECK_LAUNCH("history_penalties_kernel");
    return MI355_OK;
}

extern "C" int mi355_sample_feedback(const int32_t* ids, int32_t B, int32_t* positions, int32_t* history, int32_t* history_len,
                                     int32_t history_ld, mi355_stream_t stream) {
    MI355_CHECK_ARG(ids && B > 0, "sample_feedback: B=%d", B);
    hipLaunchKernelGGL(sample_feedback_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, ids, B, positions, history, history_len, history_ld);
    MI355_CHECK_LAUNCH("sample_feedback_kernel");
    return MI355_OK;
}

