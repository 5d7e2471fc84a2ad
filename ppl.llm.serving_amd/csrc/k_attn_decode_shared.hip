// K8, shared-prefix ("cascade") decode attention.  Requests that start with the same system prompt hold the same page ids for their leading
// pages (prefix cache); the ordinary decode kernels stream those pages once per request.  Softmax over cached keys is independent of the
// key's position (RoPE was applied when the key was written), so a decode row's attention splits into
//     shared part  keys [0, P)        -- the same memory for every row of a prefix group (shared_prefix_groups, rt_shared_prefix.cc)
//     own part     keys [P, kv_len)   -- an ordinary decode launch on a page table shifted left by P / page_size columns
// each leaving unnormalised partial rows (O[D], m, l) that ONE log-sum-exp merge combines.  This file holds the shared part and the merge.
//
// attn_decode_shared_kernel: the 16-wide side of mfma_f32_16x16x32_f16 that the grouped-query kernel fills with the query heads of one KV
// head here holds the query rows (request, head of the KV head's group) of up to 16 / grp requests of ONE group: a KV row is read once
// for all of them.  The host lists the tiles (SharedTile, kernels.h); a tile's shared pages are addressed through the page table of its
// lead row.
//   work item = (KV head, shared split, tile); block = SH_WAVES waves; a wave owns whole 16-key sub-tiles wave, wave + SH_WAVES, ... of its
//   split's range of sub-tiles.  P is a multiple of 16 and page_size % 16 == 0: a sub-tile is 16 consecutive slots of one page (one
//   scalar row base per sub-tile), there is no partial sub-tile and no key mask.  K pieces (16 bytes) go from HBM straight into the MFMA A
//   operand (lane = (key, quarter), pieces quarter, quarter + 4, ...; the Q fragments carry the matching channel permutation); V goes
//   through a wave-private LDS image only to be transposed (v_frag_tr).  Two sub-tiles are in flight per wave in two register buffers that
//   rotate statically; the loop has no workgroup barrier, the waves meet once, for the log-sum-exp merge through LDS.
//   A wave steps ONE sub-tile at a time, (P_hi | P_lo) against (V | V) in the 32 k-slots -- not the grouped-query kernel's 32-key pair
//   step: a shared prefix is short (a 512-token prompt over 4 waves and 2 splits is 4 sub-tiles per wave), pairs would run half empty
//   and need a validity mask for the odd one.
// Operand precision (the grouped-query kernel's rule): P an exact hi + lo fp16 pair (p_hi_lo), int8-g8 K and V exact hi + lo pairs of
// q * scale (TwoProduct), fp16 K and V as they are, fp32 accumulation.  What differs from the ordinary path is summation order alone.
//   -DSH_V_ROUNDED: int8 V as q * scale rounded to fp16 once (one LDS image, half the P.V MFMAs); a build switch, not the default.
// Tile reuse: a group that fills several tiles reads the same K / V in each of them.  Built: the GRID ORDER.  The grid is one-dimensional;
// consecutive workgroup ids go round-robin over the 8 XCDs (xcd_head_order, k_attn_dev.h), so workgroup L takes item
// (L % 8) * ceil(items / 8) + L / 8: an XCD walks a contiguous run of the item list, whose fastest index is the tile -- the tiles of one
// (group, KV head, split) run on one XCD back to back and all but the first find the keys in its L2.  The loads are therefore ordinary
// ones, not the non-temporal loads of the streaming kernels.  The other choice -- one block serving several column tiles from one set of
// K / V registers -- costs 32 accumulator registers per extra tile (head_dim 128) and a second Q fragment set, which halves the waves a
// SIMD holds; the grouped-query kernel is issue-bound already (profiles/r06_gqa_experiments.md), so the cheaper choice went in first.
// Formats: KV_FP16 and KV_I8G8, head_dim 128 and 64, grp <= 16, paged cache with page_size % 16 == 0 (attn_shared_supported); KV_FP8 and
// KV_I4G32 are not built.
#include <hip/hip_runtime.h>
#include "k_attn_dev.h"

namespace pplhip {

namespace {

constexpr int SH_WAVES = 4;

__device__ __forceinline__ h8 sh_splat8(_Float16 v) { return h8{v, v, v, v, v, v, v, v}; }
// exact product q * s of 8 small integers (fp16-exact) and an fp16 scale as hi + lo (the error term of a product is representable)
__device__ __forceinline__ void sh_two_product(h8 q, _Float16 s, h8& hi, h8& lo) {
    const h8 sv = sh_splat8(s);
    hi = q * sv;
    lo = __builtin_elementwise_fma(q, sv, -hi);
}

#ifdef SH_V_ROUNDED
constexpr bool SH_V_EXACT = false;
#else
constexpr bool SH_V_EXACT = true;
#endif

template <int QBIT, int D>
constexpr int sh_lds_bytes() {
    constexpr int nimg = (QBIT == KV_I8G8 && SH_V_EXACT) ? 2 : 1;
    constexpr int v_bytes = SH_WAVES * nimg * (D / 16) * ATT_VSUB * 2, merge_bytes = SH_WAVES * 16 * (D + 2) * 4;
    return v_bytes > merge_bytes ? v_bytes : merge_bytes;
}

template <int QBIT, int D>
__global__ __launch_bounds__(SH_WAVES * 64) void attn_decode_shared_kernel(const uint16_t* __restrict__ qkv, KvAddr kv,
                                                                        const int64_t* __restrict__ seq_starts,
                                                                        const int64_t* __restrict__ cache_indices, int64_t max_pages,
                                                                        const SharedTile* __restrict__ tiles, int ntiles, int H, int Hkv,
                                                                        int split, float* __restrict__ workspace) {
    using C = AttnCfg<QBIT, D>;
    constexpr int CH = C::CH, LPT = C::LPT, ELT = C::ELT;
    constexpr int PPL = LPT / 4;        // pieces per lane and sub-tile (K and V alike)
    constexpr int KSTEPS = D / 32;
    constexpr int DT = D / 16;
    constexpr int NIMG = (QBIT == KV_I8G8 && SH_V_EXACT) ? 2 : 1;
    constexpr int VW = DT * ATT_VSUB;   // halfs of one V image of a sub-tile
    static_assert(QBIT == KV_FP16 || QBIT == KV_I8G8, "formats built: fp16 and int8-g8");
    static_assert(LPT % 4 == 0, "a row must hold a multiple of four 16-byte pieces");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // per wave its V image(s); the merge buffer overlays them

    // work item of this workgroup (file header: an XCD walks a contiguous run of items, the tile is the fastest index)
    const int items = Hkv * split * ntiles, per_xcd = (items + 7) >> 3;
    const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (item >= items) return;   // (whole workgroup, before any barrier)
    const int tile_i = item % ntiles, sp_i = (item / ntiles) % split, hk = item / (ntiles * split);
    const SharedTile* const tile = tiles + tile_i;
    const int grp = H / Hkv;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    uint16_t* const vw = reinterpret_cast<uint16_t*>(smem) + wave * NIMG * VW;
    const int64_t rowstride = (int64_t)(H + 2 * Hkv) * D;

    // sub-tiles of this split, and of this wave
    const int nsub = tile->tokens >> 4;
    const int per = (nsub + split - 1) / split;
    const int s_beg = sp_i * per, s_end = s_beg + per < nsub ? s_beg + per : nsub;

    // Q fragments (MFMA B operand): column l15 = (request l15 / grp of the tile, head l15 % grp of the group); padding columns are zero
    const int my_row = tile->row[l15];
    h8 qf[KSTEPS];
    {
        const int64_t qr = my_row >= 0 ? seq_starts[my_row] : 0;
        const uint16_t* qrow = qkv + qr * rowstride + (int64_t)(hk * grp + l15 % grp) * D;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int ch = QBIT != KV_FP16 ? 16 * (kq + 4 * (ks >> 1)) + 8 * (ks & 1) : 8 * (kq + 4 * ks);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (my_row >= 0) v = *reinterpret_cast<const uint4*>(qrow + ch);
            qf[ks] = __builtin_bit_cast(h8, v);
        }
    }
    f4 o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = f4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;
    const float sm_scale = 1.0f / sqrtf((float)D);

    const char* kbase = reinterpret_cast<const char*>(kv.cache) + (int64_t)hk * kv.sH * ELT;
    const char* vbase = kbase + kv.sKV * ELT;
    const uint16_t* ksbase = kv.scale + (int64_t)hk * kv.ssH;
    const uint16_t* vsbase = ksbase + kv.ssKV;
    const int64_t rowb = kv.sN * ELT, srow = kv.ssN;
    const int rowb32 = (int)rowb, srow32 = (int)srow;   // a sub-tile spans 16 rows: the lane part fits 32 bits
    const int64_t* const page_row = cache_indices + (int64_t)tile->lead * max_pages;

    kv_u32x4 kraw[2][PPL], vraw[2][PPL];   // (native vectors: as uint4 structs the fp16 instantiations kept the raw buffers in scratch)
    uint32_t ksc[2][PPL], vsc[2][PPL];
    int vkey_l[PPL], vpc_l[PPL];   // V staging item j of this lane: (key, piece) = divmod(lane + 64 j, LPT)
#pragma unroll
    for (int j = 0; j < PPL; ++j) { vkey_l[j] = (lane + 64 * j) / LPT; vpc_l[j] = (lane + 64 * j) % LPT; }

    // sub-tile si of the shared range into register buffer p.  A prefetch past the wave's last sub-tile re-reads the split's last one
    // (never consumed): the number of loads in flight is static at every wait, and every address lies inside the shared pages
    auto load_sub = [&](auto ptag, int si) {
        constexpr int p = decltype(ptag)::value;   // (a compile-time index: with a run-time one the fp16 instantiations kept a raw buffer in scratch)
        const int64_t kb = (int64_t)(si < s_end ? si : s_end - 1) << 4;
        const int64_t pg = kv.page_shift >= 0 ? (kb >> kv.page_shift) : kb / kv.page_size;
        const int64_t slot_b = page_row[pg] * kv.page_size + (kb - pg * kv.page_size);
        const char* kp = kbase + slot_b * rowb;
        const char* vp = vbase + slot_b * rowb;
        const uint16_t* ksp = ksbase + slot_b * srow;
        const uint16_t* vsp = vsbase + slot_b * srow;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const int pc = kq + 4 * j;
            kraw[p][j] = *reinterpret_cast<const kv_u32x4*>(kp + (uint32_t)(l15 * rowb32 + pc * 16));
            if constexpr (QBIT == KV_I8G8)
                ksc[p][j] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(ksp) + (uint32_t)((l15 * srow32 + pc * 2) * 2));
        }
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            vraw[p][j] = *reinterpret_cast<const kv_u32x4*>(vp + (uint32_t)(vkey_l[j] * rowb32 + vpc_l[j] * 16));
            if constexpr (QBIT == KV_I8G8)
                vsc[p][j] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(vsp) + (uint32_t)((vkey_l[j] * srow32 + vpc_l[j] * 2) * 2));
        }
    };

    // V of buffer P into the wave's LDS image(s), row-major [key][16 channels] sub-tiles (k_attn_dev.h ATT_VSUB)
    auto stage_v = [&](auto ptag) {
        constexpr int P = decltype(ptag)::value;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const int key = vkey_l[j], ch0 = vpc_l[j] * CH;
            if constexpr (QBIT == KV_I8G8) {
                uint16_t* dst = vw + (ch0 >> 4) * ATT_VSUB + key * 16;
                if constexpr (SH_V_EXACT) {
                    h8 q[2], hi0, lo0, hi1, lo1;
                    cvt_i8x16_f16(__builtin_bit_cast(uint4, vraw[P][j]), q);
                    const h2 sc = __builtin_bit_cast(h2, vsc[P][j]);
                    sh_two_product(q[0], sc[0], hi0, lo0);
                    sh_two_product(q[1], sc[1], hi1, lo1);
                    *reinterpret_cast<uint4*>(dst) = __builtin_bit_cast(uint4, hi0);
                    *reinterpret_cast<uint4*>(dst + 8) = __builtin_bit_cast(uint4, hi1);
                    *reinterpret_cast<uint4*>(dst + VW) = __builtin_bit_cast(uint4, lo0);
                    *reinterpret_cast<uint4*>(dst + VW + 8) = __builtin_bit_cast(uint4, lo1);
                } else {
                    h8 v[2];
                    dequant_piece<QBIT>(__builtin_bit_cast(uint4, vraw[P][j]), vsc[P][j], v);
                    *reinterpret_cast<uint4*>(dst) = __builtin_bit_cast(uint4, v[0]);
                    *reinterpret_cast<uint4*>(dst + 8) = __builtin_bit_cast(uint4, v[1]);
                }
            } else {
                *reinterpret_cast<kv_u32x4*>(vw + (ch0 >> 4) * ATT_VSUB + key * 16 + (ch0 & 15)) = vraw[P][j];
            }
        }
    };
    // S^T = K . Q^T of buffer P: this lane gets keys 4 kq + r of column l15
    auto scores = [&](auto ptag) -> f4 {
        constexpr int P = decltype(ptag)::value;
        f4 sacc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            if constexpr (QBIT == KV_I8G8) {
                h8 q[2], hi0, lo0, hi1, lo1;
                cvt_i8x16_f16(__builtin_bit_cast(uint4, kraw[P][j]), q);
                const h2 sc = __builtin_bit_cast(h2, ksc[P][j]);
                sh_two_product(q[0], sc[0], hi0, lo0);
                sh_two_product(q[1], sc[1], hi1, lo1);
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(lo0, qf[2 * j], sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(lo1, qf[2 * j + 1], sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi0, qf[2 * j], sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi1, qf[2 * j + 1], sacc, 0, 0, 0);
            } else {
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, kraw[P][j]), qf[j], sacc, 0, 0, 0);
            }
        }
        return sacc;
    };
    // one 16-key step on buffer P (sub-tile si); the buffer then takes the sub-tile two of the wave's steps ahead
    auto step = [&](auto ptag, int si) {
        using T = decltype(ptag);
        stage_v(T{});
        f4 s = scores(T{});
        load_sub(T{}, si + 2 * SH_WAVES);
        float mx = -1e30f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] *= sm_scale;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(m, mx);
        const float alpha = __expf(m - mnew);
        m = mnew;
        float e[8], rs = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[r] = __expf(s[r] - mnew);
            e[4 + r] = e[r];
            rs += e[r];
        }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        h8 p_hi, p_lo;
        p_hi_lo(e, p_hi, p_lo);
        const h8 pa = __builtin_shufflevector(p_hi, p_lo, 0, 1, 2, 3, 12, 13, 14, 15);   // k-slots: (P_hi | P_lo) of keys 4 kq .. + 3
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
            float ar[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, kq * 4 + r, 64);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= ar[r];
        }
        // O += P . V: V^T fragments through the transposing LDS read (the same wave wrote them: program order, no barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            if constexpr (NIMG == 2) {
                const uint2 al = v_frag_tr(vw + VW + dt * ATT_VSUB, 4 * kq, l15);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, __builtin_bit_cast(h8, make_uint4(al.x, al.y, al.x, al.y)), o[dt], 0, 0, 0);
            }
            const uint2 a = v_frag_tr(vw + dt * ATT_VSUB, 4 * kq, l15);   // keys 4 kq .. + 3 of channel 16 dt + l15
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, __builtin_bit_cast(h8, make_uint4(a.x, a.y, a.x, a.y)), o[dt], 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the reads above precede the next step's writes
        __builtin_amdgcn_wave_barrier();
    };

    int si = s_beg + wave;
    if (si < s_end) {
        load_sub(std::integral_constant<int, 0>{}, si);
        load_sub(std::integral_constant<int, 1>{}, si + SH_WAVES);
        for (;;) {
            step(std::integral_constant<int, 0>{}, si);
            si += SH_WAVES;
            if (si >= s_end) break;
            step(std::integral_constant<int, 1>{}, si);
            si += SH_WAVES;
            if (si >= s_end) break;
        }
    }
    __syncthreads();   // every wave is done with its V image: the merge buffer may overlay them
    // ---- merge the waves: partial (o[column][d], m, l) per wave through LDS; a wave (or a split) without keys leaves m = -1e30, l = 0, O = 0
    float* mg = reinterpret_cast<float*>(smem);   // [wave][16 columns][D + 2]
    {
        float mr[4], lr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mr[r] = __shfl(m, kq * 4 + r, 64);
            lr[r] = __shfl(l, kq * 4 + r, 64);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* row = mg + ((wave * 16) + kq * 4 + r) * (D + 2);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) row[dt * 16 + l15] = o[dt][r];
            if (l15 == 0) { row[D] = mr[r]; row[D + 1] = lr[r]; }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 16 * D; idx += SH_WAVES * 64) {
        const int col = idx / D, d = idx - col * D;
        const int64_t b = tile->row[col];
        if (b < 0) continue;   // padding column: writes nothing
        const LseRow r = lse_merge(mg + col * (D + 2), SH_WAVES, 16 * (D + 2), D, d);
        const int hq = hk * grp + col % grp;
        float* ws = workspace + ((b * H + hq) * (int64_t)split + sp_i) * (D + 2);
        ws[d] = r.o;
        if (d == 0) { ws[D] = r.m; ws[D + 1] = r.l; }
    }
}

// out[row][head] = lse_merge(own partials ++ shared partials) as fp16; one block per (row, head), one thread per channel.  A row with
// row_tokens[row] == 0 is in no group: own partials only (its shared rows were never written)
template <int D>
__global__ void attn_shared_merge_kernel(const float* __restrict__ ws_own, int own_split, const float* __restrict__ ws_shared, int shared_split,
                                         const int32_t* __restrict__ row_tokens, int H, uint16_t* __restrict__ out) {
    const int64_t bh = blockIdx.x;
    const float* wo = ws_own + bh * (int64_t)own_split * (D + 2);
    const float* wsh = ws_shared + bh * (int64_t)shared_split * (D + 2);
    const bool shared = row_tokens[bh / H] > 0;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        LseRow r = lse_merge(wo, own_split, D + 2, D, d);
        if (shared) {
            const LseRow q = lse_merge(wsh, shared_split, D + 2, D, d);
            const float mm = fmaxf(r.m, q.m);
            const float a = __expf(r.m - mm), c = __expf(q.m - mm);
            r.o = fmaf(q.o, c, r.o * a);
            r.l = fmaf(q.l, c, r.l * a);
        }
        out[bh * D + d] = f2h(r.o / r.l);
    }
}

}  // namespace

bool attn_shared_supported(int kv_fmt, int cache_mode, int page_size, int H, int Hkv, int D) {
    if (cache_mode != 1 || page_size <= 0 || page_size % 16) return false;
    if (Hkv <= 0 || H <= 0 || H % Hkv || H / Hkv > 16) return false;
    return (kv_fmt == KV_FP16 || kv_fmt == KV_I8G8) && (D == 128 || D == 64);
}

hipError_t launch_attn_decode_shared(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                     const int64_t* cache_indices, int64_t max_pages, const SharedTile* tiles, int ntiles, int H, int Hkv,
                                     int D, int split, float* workspace) {
    if (ntiles == 0) return hipSuccess;
    if (ntiles < 0 || split < 1 || !attn_shared_supported(kv_fmt, kv.mode, kv.page_size, H, Hkv, D)) return hipErrorInvalidValue;
    const int64_t items = (int64_t)Hkv * split * ntiles;
    if (items > (1 << 28)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((items + 7) / 8 * 8));
    dispatch_int<KV_I8G8, KV_FP16>(kv_fmt, [&](auto QB) {
        dispatch_int<128, 64>(D, [&](auto DD) {
            constexpr int lds = sh_lds_bytes<QB, DD>();
            hipLaunchKernelGGL((attn_decode_shared_kernel<QB, DD>), grid, dim3(SH_WAVES * 64), lds, s, qkv, kv, seq_starts,
                               cache_indices, max_pages, tiles, ntiles, H, Hkv, split, workspace);
        });
    });
    return hipGetLastError();
}

hipError_t launch_attn_shared_merge(hipStream_t s, const float* ws_own, int own_split, const float* ws_shared, int shared_split,
                                    const int32_t* row_tokens, int64_t nb, int H, int D, uint16_t* out) {
    if (nb == 0) return hipSuccess;
    if (D != 128 && D != 64) return hipErrorInvalidValue;
    dispatch_int<128, 64>(D, [&](auto DD) {
        hipLaunchKernelGGL((attn_shared_merge_kernel<DD>), dim3((unsigned)(nb * H)), dim3(DD), 0, s, ws_own, own_split, ws_shared, shared_split,
                           row_tokens, H, out);
    });
    return hipGetLastError();
}

}  // namespace pplhip
