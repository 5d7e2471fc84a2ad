// The sampler's arithmetic, one row per workgroup, as __device__ row functions: the ONE greedy rule and the ONE top-k / top-p rule of the
// tree (DESIGN.md "sampler").  k_sample.hip instantiates them with a launch's uniform arguments (K13: sample_greedy_kernel,
// sample_topk_topp_kernel), k_sample_rows.hip with every row's own arguments through a row list.  A row function sees the row's pointer,
// the row's temperature (already defaulted: row_temperature), its k / p / random number and the two places its answer goes; for equal
// arguments it gives equal token and logprob bits from either file.  A third row function, top_logprobs_row (k_logprobs.hip), reports the
// first n tokens of the same ranking with the same full-vocabulary logprob; it decides nothing and shares radix_pass with the top-k rule.
// A fourth, prompt_logprob_row (k_prompt_logprobs.hip), scores one given token of a row of RAW logits: its logprob from the same two sweeps as
// top_logprobs_row at temperature 1, and its rank in the same order.
#pragma once
#include "kernels.h"

namespace pplhip {

// t NULL or <= 0: 1
__device__ __forceinline__ float row_temperature(const float* __restrict__ temperatures, int b) {
    return (temperatures && temperatures[b] > 0.f) ? temperatures[b] : 1.0f;
}

struct ArgMax {
    float v;
    int i;
};
__device__ __forceinline__ ArgMax am_better(ArgMax a, ArgMax b) {  // larger value, ties -> lower index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ArgMax wave_argmax(ArgMax a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax b;
        b.v = __shfl_xor(a.v, o, 64);
        b.i = __shfl_xor(a.i, o, 64);
        a = am_better(a, b);
    }
    return a;
}

// greedy (top_k == 1): token = first argmax of x = logits/temperature; logprob = x[token] - logsumexp(x)
// Round 4: 1024 threads and 16-byte loads, four of them in flight per thread (the 256-thread scalar form took 47 us for ONE row of 32000
// logits -- 2 % of a batch-1 decode step -- in 250 dependent load rounds; now ~8).  Same arithmetic: first maximum (lowest index on
// ties), then the sum of exp(x - max) in a fixed order per thread and a fixed tree across threads.
// A block of SG_THREADS threads; vec: the row may be read in 16-byte pieces (row stride % 4 == 0 and a 16-byte aligned base).
constexpr int SG_THREADS = 1024, SG_WAVES = SG_THREADS / 64;
__device__ __forceinline__ void sample_greedy_row(const float* __restrict__ row, bool vec, float t, int vocab, int32_t* __restrict__ out_tok,
                                                  float* __restrict__ out_lp) {
    __shared__ float sv[SG_WAVES];
    __shared__ int si[SG_WAVES];
    __shared__ float ss[SG_WAVES];
    const float invt = 1.0f / t;
    const int nv = vec ? vocab >> 2 : 0;   // float4 chunks; the tail (and unaligned rows) element by element
    ArgMax am{-INFINITY, 0x7fffffff};
    for (int c0 = threadIdx.x; c0 < nv; c0 += 4 * SG_THREADS) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * SG_THREADS;
            v[u] = c < nv ? reinterpret_cast<const float4*>(row)[c] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = (c0 + u * SG_THREADS) * 4;
            am = am_better(am, ArgMax{v[u].x * invt, i});
            am = am_better(am, ArgMax{v[u].y * invt, i + 1});
            am = am_better(am, ArgMax{v[u].z * invt, i + 2});
            am = am_better(am, ArgMax{v[u].w * invt, i + 3});
        }
    }
    for (int i = nv * 4 + threadIdx.x; i < vocab; i += SG_THREADS) am = am_better(am, ArgMax{row[i] * invt, i});
    am = wave_argmax(am);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = am.v; si[threadIdx.x >> 6] = am.i; }
    __syncthreads();
    am = ArgMax{sv[0], si[0]};
    for (int w = 1; w < SG_WAVES; ++w) am = am_better(am, ArgMax{sv[w], si[w]});
    float se = 0.f;
    for (int c0 = threadIdx.x; c0 < nv; c0 += 4 * SG_THREADS) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * SG_THREADS;
            v[u] = c < nv ? reinterpret_cast<const float4*>(row)[c] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            se += (__expf(v[u].x * invt - am.v) + __expf(v[u].y * invt - am.v)) + (__expf(v[u].z * invt - am.v) + __expf(v[u].w * invt - am.v));
    }
    for (int i = nv * 4 + threadIdx.x; i < vocab; i += SG_THREADS) se += __expf(row[i] * invt - am.v);
    se = wave_sum(se);
    if ((threadIdx.x & 63) == 0) ss[threadIdx.x >> 6] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        se = 0.f;
        for (int w = 0; w < SG_WAVES; ++w) se += ss[w];
        *out_tok = am.i;
        *out_lp = -logf(se);  // x[token] - (max + log sum) with x[token] == max
    }
}

// top-k / top-p.  Specification (DESIGN.md "sampler", restated by ref_sample): candidates = the k largest x = logits / temperature
// (ties: lower index first), k = top_k clamped to [1, TOPK_MAX]; p = softmax over the candidates; keep the shortest prefix of the
// sorted candidates whose cumulative p reaches top_p (at least one); pick the first kept candidate whose cumulative mass exceeds
// rand * kept mass.  top_k <= 0 (the usual "pure top-p" request): the candidates are the TOPK_MAX most probable tokens and p is
// the softmax over the WHOLE vocabulary (the nucleus is cut at TOPK_MAX candidates; the oracle does the same).  A per-request
// parameter never fails the batch.
// Work per row (one 256-thread block): max + total mass (2 passes over the row, which stays L2-resident), a 4 x 8-bit radix
// selection of the k-th largest value on order-preserving keys (4 passes; + 3 passes over the indices only when equal values
// straddle the cut), one gather pass, a bitonic sort of <= 1024 candidates in LDS and block-wide scans for the two cumulative
// decisions: ~7 row passes whatever k is.  (Round 2 ran one whole-row arg-max pass PER candidate: 50 passes at top_k = 50, up
// to 1024 in pure top-p mode -- ADVICE r2.)
constexpr int TOPK_MAX = 1024;
constexpr int ST_THREADS = 256;   // the block of sample_topk_topp_row (its loops and scans are written for this width)

__device__ __forceinline__ uint32_t order_key(float x) {  // larger float <=> larger key
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// block-wide inclusive scan of one int per thread (256 threads = 4 waves); `wsum` = 4 ints of LDS
__device__ __forceinline__ int block_scan_incl(int v, int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    __syncthreads();
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    for (int i = 0; i < w; ++i) v += wsum[i];
    return v;
}

// One radix-selection pass over `vocab` elements.  key(i) -> uint32, live(i) -> bool (element still matches the digits fixed so
// far).  Counts the digit `(key >> shift) & 255` of the live elements (run-length aggregated per thread: logits of one row share
// their top byte, a plain atomic per element would serialise on one LDS word), then finds the digit that holds the `need`-th
// element counting from the top (DESC) or from the bottom (ascending).  Returns the digit; `need` becomes the rank inside it and
// `*count` the number of live elements that share it.
template <bool DESC, typename KeyFn>
__device__ __forceinline__ int radix_pass(int vocab, int shift, KeyFn key_live, int& need, int* count, int* hist, int* wsum, int* sel) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    int run_bin = -1, run = 0;
    for (int i = threadIdx.x; i < vocab; i += 256) {
        uint32_t k;
        if (!key_live(i, k)) continue;
        const int bin = (int)((k >> shift) & 255u);
        if (bin == run_bin) { ++run; continue; }
        if (run) atomicAdd(&hist[run_bin], run);
        run_bin = bin; run = 1;
    }
    if (run) atomicAdd(&hist[run_bin], run);
    __syncthreads();
    const int my_bin = DESC ? 255 - (int)threadIdx.x : (int)threadIdx.x;
    const int c = hist[my_bin];
    const int incl = block_scan_incl(c, wsum);
    if (incl - c < need && need <= incl) { sel[0] = my_bin; sel[1] = need - (incl - c); sel[2] = c; }
    __syncthreads();
    const int bin = sel[0];
    need = sel[1];
    *count = sel[2];
    __syncthreads();
    return bin;
}

// Inclusive scan of a[0 .. n2) in LDS, n2 <= TOPK_MAX a power of two, by a block of ST_THREADS threads (Hillis-Steele; every round reads
// all its operands into registers, then a barrier, then adds: no second buffer needed).  The caller's barrier stands behind the writes of
// `a`; the last round's barrier stands behind the scan.
__device__ __forceinline__ void lds_scan_incl(float* a, int n2) {
    const int tid = threadIdx.x;
    for (int o = 1; o < n2; o <<= 1) {
        float add[TOPK_MAX / 256];
#pragma unroll
        for (int j = 0; j < TOPK_MAX / 256; ++j) {
            const int i = tid + j * 256;
            add[j] = (i < n2 && i >= o) ? a[i - o] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TOPK_MAX / 256; ++j) {
            const int i = tid + j * 256;
            if (i < n2) a[i] += add[j];
        }
        __syncthreads();
    }
}

// Bitonic sort of the n2 (a power of two <= TOPK_MAX) pairs (v[i], idx[i]) in LDS by a block of ST_THREADS threads; first(va, ia, vb, ib):
// a ranks before b, a strict total order of the pairs.  The caller's barrier stands behind the writes, the last step's behind the sort.
template <typename First>
__device__ __forceinline__ void lds_bitonic_sort(float* v, int* idx, int n2, First first) {
    const int tid = threadIdx.x;
    for (int size = 2; size <= n2; size <<= 1)
        for (int str = size >> 1; str > 0; str >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += 256) {
                const int lo = ((p / str) * str * 2) + (p % str), hi = lo + str;
                const bool desc = ((lo & size) == 0);  // this sub-sequence ends up "best first"
                const float va = v[lo], vb = v[hi];
                const int ia = idx[lo], ib = idx[hi];
                if (first(va, ia, vb, ib) != desc) { v[lo] = vb; v[hi] = va; idx[lo] = ib; idx[hi] = ia; }
            }
            __syncthreads();
        }
}

// The body of sample_topk_topp_row (TRUNC false: min_p and typ are not read) and of sample_trunc_row (TRUNC true), which share the candidates,
// their masses, the scan and the top-p cut.  Everything that sample_trunc_row adds stands under `if constexpr (TRUNC)`, so the other
// instantiation is the function it was before the two were one: the same floating-point operations on the same operands in the same order
// (the build has no fast-math and -ffp-contract=off, so the compiler may move them but not change them; the sort and the scan only moved
// into lds_bitonic_sort / lds_scan_incl), hence the same token and logprob bits -- tests/test_gpu_sampler_exact.py and
// tests/test_gpu_sample_rows.py hold it to that.
// A block of ST_THREADS threads; t: the row's temperature, top_k / tp / rnd: its k, top_p and random number in [0, 1); min_p / typ: as
// row_min_p / row_typical_p give them (0: off)
template <bool TRUNC>
__device__ __forceinline__ void sample_candidates_row(const float* __restrict__ row, float t, int top_k, float tp, float min_p, float typ,
                                                      float rnd, int vocab, int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    __shared__ float sf[4];
    __shared__ int wsum[4], sel[4], hist[256];
    __shared__ float cv[TOPK_MAX];   // candidate values x = logit / temperature
    __shared__ float cum[TOPK_MAX];  // inclusive cumulative mass of the sorted candidates
    __shared__ int ci[TOPK_MAX];
    const int tid = threadIdx.x;
    const float invt = 1.0f / t;
    const bool full = top_k <= 0;
    int k = full ? TOPK_MAX : (top_k < TOPK_MAX ? top_k : TOPK_MAX);
    if (k > vocab) k = vocab;

    // row maximum and total mass
    float mx = -INFINITY;
    for (int i = tid; i < vocab; i += 256) mx = fmaxf(mx, row[i] * invt);
    mx = wave_max(mx);
    if ((tid & 63) == 0) sf[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sf[0], sf[1]), fmaxf(sf[2], sf[3]));
    __syncthreads();
    float se = 0.f;
    for (int i = tid; i < vocab; i += 256) se += __expf(row[i] * invt - mx);
    se = wave_sum(se);
    if ((tid & 63) == 0) sf[tid >> 6] = se;
    __syncthreads();
    se = sf[0] + sf[1] + sf[2] + sf[3];
    __syncthreads();

    // the k-th largest key, most significant byte first
    uint32_t prefix = 0, mask = 0;
    int need = k, n_eq = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        const int bin = radix_pass<true>(vocab, shift,
            [&](int i, uint32_t& kk) { kk = order_key(row[i] * invt); return (kk & mask) == prefix; }, need, &n_eq, hist, wsum, sel);
        prefix |= (uint32_t)bin << shift;
        mask |= 255u << shift;
    }
    // `need` of the `n_eq` elements whose key equals the cut value are candidates: the ones with the lowest indices
    int idx_cut = 0x7fffffff;
    if (need < n_eq) {
        uint32_t ip = 0, im = 0;
        int dummy = 0;
#pragma unroll 1
        for (int shift = 24; shift >= 0; shift -= 8) {
            const int bin = radix_pass<false>(vocab, shift,
                [&](int i, uint32_t& kk) { kk = (uint32_t)i; return order_key(row[i] * invt) == prefix && ((uint32_t)i & im) == ip; },
                need, &dummy, hist, wsum, sel);
            ip |= (uint32_t)bin << shift;
            im |= 255u << shift;
        }
        idx_cut = (int)ip;
    }
    // gather the k candidates, pad to a power of two, sort by (value descending, index ascending)
    if (tid == 0) { sel[2] = 0; sel[3] = 0; }
    __syncthreads();
    for (int i = tid; i < vocab; i += 256) {
        const float x = row[i] * invt;
        const uint32_t kk = order_key(x);
        if (kk > prefix || (kk == prefix && i <= idx_cut)) {
            const int slot = atomicAdd(&sel[3], 1);
            if (slot < TOPK_MAX) { cv[slot] = x; ci[slot] = i; }
        }
    }
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    __syncthreads();
    for (int i = k + tid; i < n2; i += 256) { cv[i] = -INFINITY; ci[i] = 0x7fffffff; }
    __syncthreads();
    lds_bitonic_sort(cv, ci, n2, [](float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); });
    // masses exp(x - max) of the sorted candidates and their inclusive scan
    float xv[TOPK_MAX / 256];
    float ev[TRUNC ? TOPK_MAX / 256 : 1];   // sample_trunc_row keeps the masses too
#pragma unroll
    for (int j = 0; j < TOPK_MAX / 256; ++j) {
        const int i = tid + j * 256;
        xv[j] = i < k ? cv[i] : -INFINITY;  // keep the candidate's x for the logprob
    }
    __syncthreads();
    int with_mass = 0;
#pragma unroll
    for (int j = 0; j < TOPK_MAX / 256; ++j) {
        const int i = tid + j * 256;
        if (i < n2) {
            const float e = i < k ? expf(xv[j] - mx) : 0.f;
            cum[i] = e;
            with_mass += e > 0.f;
            if constexpr (TRUNC) ev[j] = e;
        } else if constexpr (TRUNC) {
            ev[j] = 0.f;
        }
    }
    if (with_mass) atomicAdd(&sel[2], with_mass);
    __syncthreads();
    lds_scan_incl(cum, n2);
    // Candidates without mass (masked logits: -inf) sort last and are never the answer: the decisions below run over the km candidates that
    // carry mass.  (Every entry of the scan is summed in a tree of its own, so the sums are not monotone to the last bit: a massless entry
    // could exceed a target of rand ~ 1 that the last entry with mass just missed.)
    const int km = sel[2] > 0 ? sel[2] : 1;
    // keep = 1 + first i with cum[i] / tot >= tp (all km when none); tot = whole-row mass in pure top-p mode
    const float tot = full ? se : cum[km - 1];
    if (tid == 0) { sel[0] = km - 1; sel[1] = 0x7fffffff; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TOPK_MAX / 256; ++j) {
        const int i = tid + j * 256;
        if (i < km && cum[i] / tot >= tp) atomicMin(&sel[0], i);
    }
    __syncthreads();
    int keep = sel[0] + 1;
    int pick = -1;
    if constexpr (TRUNC) {
        // min_p: keep_m = the number of candidates with mass e >= min_p (e_0 = expf(0) = 1 exactly: "p >= min_p * p_max"; a prefix of the
        // sorted list, at least one; min_p == 0 counts all km); keep = min(keep_p, keep_m)
        if (tid == 0) sel[3] = 0;   // (the gather's counter, free since the gather)
        __syncthreads();
        int n_m = 0;
#pragma unroll
        for (int j = 0; j < TOPK_MAX / 256; ++j) n_m += (tid + j * 256 < km && ev[j] >= min_p);
        if (n_m) atomicAdd(&sel[3], n_m);
        __syncthreads();
        const int keep_m = sel[3] > 0 ? sel[3] : 1;
        if (keep_m < keep) keep = keep_m;
        if (typ > 0.f) {   // (uniform over the block)
            // typical_p over the `keep` survivors, renormalised: q = e / S, lq = ln q, H = -sum q lq, s = |-lq - H|
            __shared__ float sk[TOPK_MAX];   // the keys s, sorted ascending; then the scan of q in that order
            __shared__ int sr[TOPK_MAX];     // the rank each key came from
            const float S = cum[keep - 1];
            const float lS = logf(S);
            __syncthreads();                 // everybody has S: cum becomes q by rank
            float lq[TOPK_MAX / 256];
            float h = 0.f;                   // per thread its <= 4 terms in order, then the tree of wave_sum, then (w0 + w1) + (w2 + w3)
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                lq[j] = 0.f;
                if (i < keep) {
                    lq[j] = (xv[j] - mx) - lS;
                    const float q = ev[j] / S;
                    cum[i] = q;
                    h += q * lq[j];
                }
            }
            h = wave_sum(h);
            if ((tid & 63) == 0) sf[tid >> 6] = h;
            if (tid == 0) { sel[0] = keep - 1; sel[2] = -1; }   // (km and keep_p are in registers)
            __syncthreads();
            const float H = -((sf[0] + sf[1]) + (sf[2] + sf[3]));
            int n2t = 1;
            while (n2t < keep) n2t <<= 1;
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                if (i < n2t) {
                    sk[i] = i < keep ? fabsf(-lq[j] - H) : INFINITY;
                    sr[i] = i < keep ? i : 0x7fffffff;
                }
            }
            __syncthreads();
            lds_bitonic_sort(sk, sr, n2t, [](float va, int ia, float vb, int ib) { return va < vb || (va == vb && ia < ib); });
            // cq = the scan of q in s order; n_t = 1 + first j with cq[j] >= typ (keep when none)
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                if (i < n2t) {   // (the first `keep` entries are the survivors, their keys being finite; the bound holds for a NaN row too)
                    const int r = sr[i];
                    sk[i] = (i < keep && (unsigned)r < (unsigned)keep) ? cum[r] : 0.f;
                }
            }
            __syncthreads();
            lds_scan_incl(sk, n2t);
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                if (i < keep && sk[i] >= typ) atomicMin(&sel[0], i);
            }
            __syncthreads();
            const int n_t = sel[0] + 1;
            // membership by rank, then the masses of the members in RANK order and their scan: the pick is a function of the set alone
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                if (i < n2t) cum[i] = 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                if (i < n_t) {
                    const int r = sr[i];
                    if ((unsigned)r < (unsigned)keep) cum[r] = 1.f;
                }
            }
            __syncthreads();
            bool member[TOPK_MAX / 256];
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                member[j] = i < keep && cum[i] != 0.f;
                if (i < n2t) cum[i] = member[j] ? ev[j] : 0.f;
            }
            __syncthreads();
            lds_scan_incl(cum, n2t);
            const float target = rnd * cum[keep - 1];
#pragma unroll
            for (int j = 0; j < TOPK_MAX / 256; ++j) {
                const int i = tid + j * 256;
                if (member[j]) {
                    if (cum[i] > target) atomicMin(&sel[1], i);
                    atomicMax(&sel[2], i);   // the last member: the answer when no sum exceeds the target
                }
            }
            __syncthreads();
            pick = sel[1] < keep ? sel[1] : (sel[2] > 0 ? sel[2] : 0);
        }
    }
    if (pick < 0) {
        const float target = rnd * cum[keep - 1];
#pragma unroll
        for (int j = 0; j < TOPK_MAX / 256; ++j) {
            const int i = tid + j * 256;
            if (i < keep && cum[i] > target) atomicMin(&sel[1], i);
        }
        __syncthreads();
        pick = sel[1] < keep ? sel[1] : keep - 1;
    }
#pragma unroll
    for (int j = 0; j < TOPK_MAX / 256; ++j)
        if (tid + j * 256 == pick) {
            *out_tok = ci[pick];
            *out_lp = xv[j] - (mx + logf(se));
        }
}

__device__ __forceinline__ void sample_topk_topp_row(const float* __restrict__ row, float t, int top_k, float tp, float rnd, int vocab,
                                                     int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    sample_candidates_row<false>(row, t, top_k, tp, 0.f, 0.f, rnd, vocab, out_tok, out_lp);
}

// min_p / typical_p truncation (DESIGN.md "numerics", min_p / typical_p row): the candidates, masses, scan and top-p cut of
// sample_topk_topp_row; then keep = min(keep_p, #{e >= min_p}); then, with typical_p on, the survivors renormalised and ordered by
// |-ln q - H| (ties by rank), cut where their mass reaches typical_p, and the pick over the members in rank order.  The logprob is the
// full-vocabulary one of the other row functions.  Every loop runs to k, km, keep, n2 or n2t <= TOPK_MAX.  A block of ST_THREADS threads;
// LDS: the three 4 KiB arrays of sample_topk_topp_row and two more.
__device__ __forceinline__ void sample_trunc_row(const float* __restrict__ row, float t, int top_k, float tp, float min_p, float typ, float rnd,
                                                 int vocab, int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    sample_candidates_row<true>(row, t, top_k, tp, row_min_p(min_p), row_typical_p(typ), rnd, vocab, out_tok, out_lp);
}

// top-N logprobs (DESIGN.md "numerics", top-N logprobs row): the first n entries of the ranking "x = logits / temperature descending, ties
// by ascending index" (am_better's order) with logprob x - logsumexp(x) over the WHOLE vocabulary, the number both samplers report for
// their token.  Entries j >= vocab are padded (token -1, logprob -inf); the slots behind n are not written.
// Work per row (one block of TL_THREADS = ST_THREADS threads, the width radix_pass is written for): maximum and mass in the greedy row's
// style (16-byte loads, four in flight per thread, when `vec`), the four radix rounds for the key of rank n (+ the index rounds only when
// equal keys straddle the cut), one gather of <= 20 candidates into LDS, a 32-entry bitonic sort by shuffles in wave 0, one thread per
// entry for the answer.  -0 ranks as +0 (the float comparison of am_better calls them equal): rank_key folds the two before order_key.
constexpr int TL_THREADS = ST_THREADS, TL_WAVES = TL_THREADS / 64;
static_assert(TL_THREADS == 256, "radix_pass and block_scan_incl are written for 256 threads");

__device__ __forceinline__ uint32_t rank_key(float x) {
    return order_key(x == 0.f ? 0.f : x);
}

// the maximum sweep of a TL_THREADS block over x = row * invt (16-byte loads, four in flight per thread, over the first nv float4 chunks; the
// rest element by element); sf: TL_WAVES floats of LDS, free again when it returns.  A maximum does not depend on the order it is taken in.
__device__ __forceinline__ float tl_row_max(const float* __restrict__ row, int nv, float invt, int vocab, float* sf) {
    const int tid = threadIdx.x;
    const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    float mx = -INFINITY;
    for (int c0 = tid; c0 < nv; c0 += 4 * TL_THREADS) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * TL_THREADS;
            v[u] = c < nv ? reinterpret_cast<const float4*>(row)[c] : none;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) mx = fmaxf(mx, fmaxf(fmaxf(v[u].x * invt, v[u].y * invt), fmaxf(v[u].z * invt, v[u].w * invt)));
    }
    for (int i = nv * 4 + tid; i < vocab; i += TL_THREADS) mx = fmaxf(mx, row[i] * invt);
    mx = wave_max(mx);
    if ((tid & 63) == 0) sf[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sf[0], sf[1]), fmaxf(sf[2], sf[3]));
    __syncthreads();
    return mx;
}

__device__ __forceinline__ void top_logprobs_row(const float* __restrict__ row, bool vec, float t, int n, int vocab,
                                                 int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    __shared__ float sf[TL_WAVES];
    __shared__ int wsum[4], sel[4], hist[256];
    __shared__ float cv[32];
    __shared__ int ci[32];
    const int tid = threadIdx.x;
    const float invt = 1.0f / t;
    const int k = n < vocab ? n : vocab;
    const int nv = vec ? vocab >> 2 : 0;   // float4 chunks; the tail (and unaligned rows) element by element
    const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);

    const float mx = tl_row_max(row, nv, invt, vocab, sf);
    // the mass: per thread its chunks in order, (x + y) + (z + w) inside a chunk, then its tail elements; then a tree over the block
    float se = 0.f;
    for (int c0 = tid; c0 < nv; c0 += 4 * TL_THREADS) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * TL_THREADS;
            v[u] = c < nv ? reinterpret_cast<const float4*>(row)[c] : none;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            se += (__expf(v[u].x * invt - mx) + __expf(v[u].y * invt - mx)) + (__expf(v[u].z * invt - mx) + __expf(v[u].w * invt - mx));
    }
    for (int i = nv * 4 + tid; i < vocab; i += TL_THREADS) se += __expf(row[i] * invt - mx);
    se = wave_sum(se);
    if ((tid & 63) == 0) sf[tid >> 6] = se;
    __syncthreads();
    se = (sf[0] + sf[1]) + (sf[2] + sf[3]);   // with the wave's six steps: log2(TL_THREADS) tree steps
    const float lse = mx + logf(se);

    // the key of rank k, most significant byte first
    uint32_t prefix = 0, mask = 0;
    int need = k, n_eq = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        const int bin = radix_pass<true>(vocab, shift,
            [&](int i, uint32_t& kk) { kk = rank_key(row[i] * invt); return (kk & mask) == prefix; }, need, &n_eq, hist, wsum, sel);
        prefix |= (uint32_t)bin << shift;
        mask |= 255u << shift;
    }
    // `need` of the `n_eq` elements whose key equals the cut are entries: the ones with the lowest indices
    int idx_cut = 0x7fffffff;
    if (need < n_eq) {
        uint32_t ip = 0, im = 0;
        int dummy = 0;
#pragma unroll 1
        for (int shift = 24; shift >= 0; shift -= 8) {
            const int bin = radix_pass<false>(vocab, shift,
                [&](int i, uint32_t& kk) { kk = (uint32_t)i; return rank_key(row[i] * invt) == prefix && ((uint32_t)i & im) == ip; },
                need, &dummy, hist, wsum, sel);
            ip |= (uint32_t)bin << shift;
            im |= 255u << shift;
        }
        idx_cut = (int)ip;
    }
    // gather the k entries (any order), pad to 32, sort by (x descending, index ascending)
    if (tid < 32) { cv[tid] = -INFINITY; ci[tid] = 0x7fffffff; }
    if (tid == 0) sel[3] = 0;
    __syncthreads();
    for (int i = tid; i < vocab; i += TL_THREADS) {
        const float x = row[i] * invt;
        const uint32_t kk = rank_key(x);
        if (kk > prefix || (kk == prefix && i <= idx_cut)) {
            const int slot = atomicAdd(&sel[3], 1);
            if (slot < 32) { cv[slot] = x; ci[slot] = i; }
        }
    }
    __syncthreads();
    if (tid < 64) {   // wave 0; lanes 32..63 sort a copy of their own, which nobody reads
        ArgMax a{cv[tid & 31], ci[tid & 31]};
#pragma unroll
        for (int size = 2; size <= 32; size <<= 1)
#pragma unroll
            for (int str = size >> 1; str > 0; str >>= 1) {
                ArgMax b;
                b.v = __shfl_xor(a.v, str, 64);
                b.i = __shfl_xor(a.i, str, 64);
                const bool a_first = a.v > b.v || (a.v == b.v && a.i < b.i);   // a ranks before b
                const bool want_first = ((tid & str) == 0) == ((tid & size) == 0);  // this lane keeps the better of the pair
                a = (a_first == want_first) ? a : b;
            }
        if (tid < n) {
            out_tok[tid] = tid < k ? a.i : -1;
            out_lp[tid] = tid < k ? a.v - lse : -INFINITY;
        }
    }
}

// prompt logprobs (DESIGN.md "numerics", prompt logprobs row): one prompt position.  `row` holds the RAW fp32 logits of the position (the
// model's own distribution: no temperature, no penalty, no logit rule -- the opposite of top_logprobs_row, which reports what the sampler
// sees), `target` the prompt token that follows it.  *out_lp = x[target] - lse with the lse of top_logprobs_row at temperature 1: the same
// maximum sweep (tl_row_max) and the same mass sweep in the same order -- per thread its 16-byte pieces in order, (x + y) + (z + w) inside a
// piece, then its tail elements, six shuffle steps, (w0 + w1) + (w2 + w3) -- so where the target is among that function's entries for the
// same row the two logprobs are equal bit for bit.  *out_rank = #{v : x[v] > x[t]} + #{v < t : x[v] == x[t]}, am_better's order (rank 0 is
// the greedy token; float comparison, so -0 ties with +0), counted in the mass sweep and summed over the block in integers: exact.
// Two row passes; a block of TL_THREADS threads.
__device__ __forceinline__ void prompt_logprob_row(const float* __restrict__ row, bool vec, int target, int vocab, float* __restrict__ out_lp,
                                                   int32_t* __restrict__ out_rank) {
    __shared__ float sf[TL_WAVES];
    __shared__ int sc[TL_WAVES];
    const int tid = threadIdx.x;
    const int nv = vec ? vocab >> 2 : 0;
    const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    const float xt = row[target];
    const float mx = tl_row_max(row, nv, 1.0f, vocab, sf);
    float se = 0.f;
    int ahead = 0;
    for (int c0 = tid; c0 < nv; c0 += 4 * TL_THREADS) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * TL_THREADS;
            v[u] = c < nv ? reinterpret_cast<const float4*>(row)[c] : none;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            se += (__expf(v[u].x - mx) + __expf(v[u].y - mx)) + (__expf(v[u].z - mx) + __expf(v[u].w - mx));
            const int c = c0 + u * TL_THREADS, i = c * 4;
            if (c < nv) {   // (the -inf filler of a missing piece would tie with a target at -inf)
                ahead += (v[u].x > xt || (v[u].x == xt && i < target)) + (v[u].y > xt || (v[u].y == xt && i + 1 < target)) +
                         (v[u].z > xt || (v[u].z == xt && i + 2 < target)) + (v[u].w > xt || (v[u].w == xt && i + 3 < target));
            }
        }
    }
    for (int i = nv * 4 + tid; i < vocab; i += TL_THREADS) {
        const float x = row[i];
        se += __expf(x - mx);
        ahead += x > xt || (x == xt && i < target);
    }
    se = wave_sum(se);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
    if ((tid & 63) == 0) { sf[tid >> 6] = se; sc[tid >> 6] = ahead; }
    __syncthreads();
    if (tid == 0) {
        se = (sf[0] + sf[1]) + (sf[2] + sf[3]);
        const float lse = mx + logf(se);
        *out_lp = xt - lse;
        *out_rank = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    }
    __syncthreads();   // a caller may go on with top_logprobs_row on the same row
}

}  // namespace pplhip
