// RoPE + KV write with a prologue on the projected rows (Qwen2 / Qwen3): an additive bias on every q, k and v column, then an RMSNorm
// over every q and k head row, both in front of the rotation -- in the pass that touches every q / k / v element once anyway.
//   bias : a = fp16(fp32(y) + fp32(bias[col])), y the fp16 row or the slabs' value (slab_load8); bias fp16 [(H + 2 Hkv) D]
//   norm : n[i] = fp16(fp32(a[i]) / sqrt(mean_i(a[i]^2) + eps) * fp32(w[i])) over the D channels of a q or k head row, w = q_norm or
//          k_norm, fp16 [D], shared by the heads: the (Skip)RMSNorm rule of k_elem.hip on a head row.  Never v.
// then rotation, the in-place q store and the cache write exactly as rope_kv_write_kernel (k_rope_kv.hip) does them, in all four formats.
//
// Same work split as that kernel: one item = one (head, 8 channels + their RoPE partners) of a token, 1-4 blocks per token, the request
// found by every thread for itself, the rows from fp16 or from unreduced split-K slabs.  New:
//   bias : two more 16-byte loads per q / k item, one per v item.
//   norm : an item holds 16 of its head row's D channels; the D/16 items of the row are consecutive lanes of one wave, aligned to their
//          count (256 and the items of a head are powers of two: item w sits on lane w % 64) -- the lanes the fp8 row maximum meets in.
//          Each sums its 16 squares in channel order, then the group adds them in an xor butterfly: both partners of a step add the same
//          two numbers, so every lane of the group holds the same bits and a repeated call gives them again.  The norm weights are
//          requested before the butterfly.  No LDS, no barrier.
// The kernel is instantiated per cache format and per (bias, norm): the bias-only form carries no reduction and no weight loads.  With
// neither, the launcher launches rope_kv_write_kernel itself.
#include <stdlib.h>
#include "k_rope_kv_dev.h"

namespace pplhip {

// sum over the n lanes (a power of two, aligned) of an item group, the same bits on each of them
__device__ __forceinline__ float group_sum(float v, int n) {
    for (int o = 1; o < n; o <<= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}
// x[i] = fp16(x[i] + bias[col + i]), 8 columns
__device__ __forceinline__ void add_bias8(const uint16_t* __restrict__ bias, int col, float* x) {
    float b[8];
    unpack8(*reinterpret_cast<const uint4*>(bias + col), b);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = round_h(__fadd_rn(x[i], b[i]));
}

template <int QBIT, bool BIAS, bool NORM>
__global__ __launch_bounds__(256) void rope_kv_prologue_kernel(uint16_t* __restrict__ qkv, const float* __restrict__ cos_sin, KvAddr kv,
                                                               const int64_t* __restrict__ seq_starts, const int64_t* __restrict__ start_pos,
                                                               const int64_t* __restrict__ cache_indices, int64_t max_pages, int64_t B,
                                                               int64_t t0, int H, int Hkv, int D, SplitSlabs sl, QkvPrologue pr) {
    const int64_t t = t0 + blockIdx.x;
    // request of row t: last b with seq_starts[b] <= t (rope_kv_write_kernel's lookup)
    int64_t b;
    {
        const int64_t g = t < B ? t : B - 1;
        int64_t lo = 0, hi = B - 1;
        if (seq_starts[g] <= t && t < seq_starts[g + 1]) {
            lo = g;
        } else {
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (seq_starts[mid] <= t) lo = mid; else hi = mid - 1;
            }
        }
        b = lo;
    }
    const int64_t pos = start_pos[b] + (t - seq_starts[b]);
    const int64_t slot = kv_slot(kv, cache_indices, max_pages, b, pos);
    const int half = D / 2;
    const int bph = half / 8;                  // rope work items per head
    const int n_rope = (H + Hkv) * bph;
    const int n_v = Hkv * (D / 8);
    const int v0 = QBIT == KV_FP8 ? (n_rope + D / 8 - 1) / (D / 8) * (D / 8) : (QBIT == KV_I4G32 ? (n_rope + 3) / 4 * 4 : n_rope);
    uint16_t* row = qkv + t * (int64_t)(H + 2 * Hkv) * D;
    const float* cs = cos_sin + pos * D;       // cos[0..half) then sin[0..half)
    for (int w = blockIdx.y * 256 + threadIdx.x; w < v0 + n_v; w += 256 * gridDim.y) {
        if (w < n_rope) {
            const int head = w / bph, i0 = (w - head * bph) * 8;
            uint16_t* x = row + (int64_t)head * D;
            float a[8], bb[8], c[8], s[8], ra[8], rb[8];
            if (sl.splits) {
                slab_load8(sl, t - t0, head * D + i0, a);
                slab_load8(sl, t - t0, head * D + i0 + half, bb);
            } else {
                unpack8(*reinterpret_cast<const uint4*>(x + i0), a);
                unpack8(*reinterpret_cast<const uint4*>(x + i0 + half), bb);
            }
            uint4 wa = {}, wb = {};            // the head row's norm weights, in flight under the bias add and the reduction
            if constexpr (NORM) {
                const uint16_t* nw = head < H ? pr.q_norm : pr.k_norm;
                wa = *reinterpret_cast<const uint4*>(nw + i0);
                wb = *reinterpret_cast<const uint4*>(nw + i0 + half);
            }
            *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(cs + i0);
            *reinterpret_cast<float4*>(c + 4) = *reinterpret_cast<const float4*>(cs + i0 + 4);
            *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(cs + half + i0);
            *reinterpret_cast<float4*>(s + 4) = *reinterpret_cast<const float4*>(cs + half + i0 + 4);
            if constexpr (BIAS) {
                add_bias8(pr.bias, head * D + i0, a);
                add_bias8(pr.bias, head * D + i0 + half, bb);
            }
            if constexpr (NORM) {
                float ss = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) ss = __fadd_rn(ss, __fmul_rn(a[i], a[i]));
#pragma unroll
                for (int i = 0; i < 8; ++i) ss = __fadd_rn(ss, __fmul_rn(bb[i], bb[i]));
                ss = group_sum(ss, bph);       // (head is uniform over the item group)
                const float inv = 1.0f / sqrtf(ss / (float)D + pr.eps);
                float wfa[8], wfb[8];
                unpack8(wa, wfa);
                unpack8(wb, wfb);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    a[i] = round_h(__fmul_rn(__fmul_rn(a[i], inv), wfa[i]));
                    bb[i] = round_h(__fmul_rn(__fmul_rn(bb[i], inv), wfb[i]));
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                ra[i] = round_h(__fsub_rn(__fmul_rn(a[i], c[i]), __fmul_rn(bb[i], s[i])));
                rb[i] = round_h(__fadd_rn(__fmul_rn(bb[i], c[i]), __fmul_rn(a[i], s[i])));
            }
            if (head < H) {  // q: in place
                *reinterpret_cast<uint4*>(x + i0) = pack8(ra);
                *reinterpret_cast<uint4*>(x + i0 + half) = pack8(rb);
            } else if constexpr (QBIT == KV_FP8) {
                float mx = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fmaxf(fabsf(ra[i]), fabsf(rb[i])));
                const int e = fp8_row_exp(group_max(mx, bph));
                store_fp8_row8(kv, 0, head - H, slot, i0, ra, e);
                store_fp8_row8(kv, 0, head - H, slot, i0 + half, rb, e);
            } else if constexpr (QBIT == KV_I4G32) {
                float ma = 0.f, mb = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) { ma = fmaxf(ma, fabsf(ra[i])); mb = fmaxf(mb, fabsf(rb[i])); }
                if (D == 32) ma = mb = group_max(fmaxf(ma, mb), 2);
                else { ma = group_max(ma, 4); mb = group_max(mb, 4); }
                store_i4_group8(kv, 0, head - H, slot, i0, ra, ma);
                store_i4_group8(kv, 0, head - H, slot, i0 + half, rb, mb);
            } else {
                store_group8<QBIT>(kv, 0, head - H, slot, i0, ra);
                store_group8<QBIT>(kv, 0, head - H, slot, i0 + half, rb);
            }
        } else if (w >= v0) {  // v: the bias only
            const int wv = w - v0;
            const int head = wv / (D / 8), i0 = (wv - head * (D / 8)) * 8;
            const int col = (H + Hkv + head) * D + i0;
            float v[8];
            if (sl.splits) slab_load8(sl, t - t0, col, v);
            else unpack8(*reinterpret_cast<const uint4*>(row + col), v);
            if constexpr (BIAS) add_bias8(pr.bias, col, v);
            if constexpr (QBIT == KV_FP8) {
                float mx = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(v[i]));
                store_fp8_row8(kv, 1, head, slot, i0, v, fp8_row_exp(group_max(mx, D / 8)));
            } else if constexpr (QBIT == KV_I4G32) {
                float mx = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(v[i]));
                store_i4_group8(kv, 1, head, slot, i0, v, group_max(mx, 4));
            } else {
                store_group8<QBIT>(kv, 1, head, slot, i0, v);
            }
        }
    }
}

template <int QBIT>
static void launch_form(const dim3& grid, hipStream_t s, uint16_t* qkv, const float* cos_sin, const KvAddr& kv, const int64_t* seq_starts,
                        const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t t0, int H, int Hkv, int D,
                        const SplitSlabs& sl, const QkvPrologue& pr) {
#define PPLHIP_PROLOGUE(BIAS, NORM)                                                                                                       \
    hipLaunchKernelGGL((rope_kv_prologue_kernel<QBIT, BIAS, NORM>), grid, dim3(256), 0, s, qkv, cos_sin, kv, seq_starts, start_pos,      \
                       cache_indices, max_pages, B, t0, H, Hkv, D, sl, pr)
    if (pr.bias && pr.q_norm) PPLHIP_PROLOGUE(true, true);
    else if (pr.bias) PPLHIP_PROLOGUE(true, false);
    else PPLHIP_PROLOGUE(false, true);
#undef PPLHIP_PROLOGUE
}

hipError_t launch_rope_kv_prologue(hipStream_t s, uint16_t* qkv, const float* cos_sin, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                   const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t t0, int64_t T,
                                   int H, int Hkv, int D, const SplitSlabs* qkv_slabs, const QkvPrologue& pr) {
    if (!pr.bias && !pr.q_norm && !pr.k_norm)   // nothing in front of the rotation: the ordinary kernel, the bits it always gave
        return launch_rope_kv_write(s, qkv, cos_sin, kv, kv_fmt, seq_starts, start_pos, cache_indices, max_pages, B, t0, T, H, Hkv, D, qkv_slabs);
    if (!pr.q_norm != !pr.k_norm) return hipErrorInvalidValue;   // the norm is on q and k heads together
    // the norm's item group is the D/16 lanes of a head row: a power of two of them, inside one wave
    if (pr.q_norm && (D < 32 || D > 1024 || (D & (D - 1)) || !(pr.eps >= 0.f))) return hipErrorInvalidValue;
    if (((uintptr_t)pr.bias | (uintptr_t)pr.q_norm | (uintptr_t)pr.k_norm) & 15) return hipErrorInvalidValue;   // 16-byte loads
    if (T == 0) return hipSuccess;
    SplitSlabs sl;
    if (qkv_slabs && qkv_slabs->splits > 0) {
        sl = *qkv_slabs;
        if (sl.N != (H + 2 * Hkv) * D || sl.M != T) return hipErrorInvalidValue;
    }
    if (D % 16 || (kv_fmt != KV_FP16 && kv_fmt != KV_I8G8 && kv_fmt != KV_FP8 && kv_fmt != KV_I4G32)) return hipErrorInvalidValue;
    if (kv_fmt == KV_I4G32 && D != 32 && D != 64 && D != 128) return hipErrorInvalidValue;
    // launch_rope_kv_write's grid: one item per thread on up to 4 blocks per token, 2 when the launch fills the chip many times over
    const int items = (H + Hkv) * (D / 16) + Hkv * (D / 8);
    static const int forced_y = getenv("PPLHIP_ROPE_BLOCKS_PER_TOKEN") ? atoi(getenv("PPLHIP_ROPE_BLOCKS_PER_TOKEN")) : 0;
    int gy = (items + 255) / 256;
    if (gy > 4) gy = 4;
    if (T >= 4096 && gy > 2) gy = 2;
    if (forced_y > 0) gy = forced_y;
    const dim3 grid((unsigned)T, (unsigned)gy);
    if (kv_fmt == KV_I4G32) launch_form<KV_I4G32>(grid, s, qkv, cos_sin, kv, seq_starts, start_pos, cache_indices, max_pages, B, t0, H, Hkv, D, sl, pr);
    else if (kv_fmt == KV_FP8) launch_form<KV_FP8>(grid, s, qkv, cos_sin, kv, seq_starts, start_pos, cache_indices, max_pages, B, t0, H, Hkv, D, sl, pr);
    else if (kv_fmt == KV_I8G8) launch_form<KV_I8G8>(grid, s, qkv, cos_sin, kv, seq_starts, start_pos, cache_indices, max_pages, B, t0, H, Hkv, D, sl, pr);
    else launch_form<KV_FP16>(grid, s, qkv, cos_sin, kv, seq_starts, start_pos, cache_indices, max_pages, B, t0, H, Hkv, D, sl, pr);
    return hipGetLastError();
}

}  // namespace pplhip
