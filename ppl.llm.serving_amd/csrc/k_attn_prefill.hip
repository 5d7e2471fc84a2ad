// K6 / K7 MultiHeadCacheAttention, prefill and cache-prefill (prefix-cache hit) phases, head_dim 64 and 32 (head_dim 128:
// k_attn_prefill32.hip, to which launch_attn_prefill hands such launches): the new tokens of a
// request attend causally to cache positions [0, start_pos + i].  K and V are read back from the KV slab
// (after K5 wrote them), so a cold prefill, a prefix-cache hit (start_pos > 0, ENGINE_CONF_CACHE_PREFILL,
// src/engine/llm_engine.cc:114) and a 1-token request all run this one kernel.  MFMA-bound.
//
// Work decomposition (wave64, gfx950, mfma_f32_16x16x32_f16):
//   grid  = (ceil(max_seq_len / 128), requests, H); block = 8 waves; wave w owns 16 query rows.
//   per KV tile of 128 keys:  K tile -> LDS as fp16 [key][D] (16-B chunks XOR-swizzled against bank conflicts),
//                             V tile -> LDS row-major [16 keys][16 channels] sub-tiles, read TRANSPOSED (ds_read_b64_tr_b16) because the PV
//                             MFMA contracts over keys and needs them contiguous per lane.
//   The tile is staged global -> registers -> LDS; the loads of tile t+1 are issued BEFORE the MFMAs of tile t and
//   converted / written after them (register prefetch, T14 of the CDNA guide), so HBM/L2 latency hides under compute.
//   S^T = K . Q^T  (A = K fragment from LDS, B = Q fragment in registers): the C layout then gives every lane
//   32 scores of ONE query row (col = lane&15), so the online softmax is lane-local plus two xor-shuffles and
//   the probabilities are already in MFMA A-operand order for O += P . V (the k-slot permutation this implies
//   is applied identically to the V^T reads).
//   int8 KV is dequantised to fp16 while staging (one fp16 rounding of q*scale; DESIGN.md "numerics"); fp8 KV likewise, with the
//   row's power-of-two scale inside the conversion -- exact, no rounding; int4 KV (KV_I4G32): a piece is one group of 32 channels, nibble - 8
//   times its 8-bit scale in packed fp16 -- exact as well; the piece fills four K chunks and two 16-channel V sub-tiles.
// Oracle: ref_attention (oracle/llama_ref.c).
#include <stdlib.h>
#include "k_attn_dev.h"

namespace pplhip {

#ifndef PF_NW
#define PF_NW 8   // waves per block, 16 query rows each (4, two blocks per CU: equal at 8192 tokens, 12-18 % slower on shorter prompts -- every staged tile serves half the rows)
#endif
constexpr int PF_BM = 16 * PF_NW;  // query rows per block
constexpr int PF_BN = 128;  // keys per tile
constexpr int PF_THREADS = 64 * PF_NW;

template <int D>
__device__ __forceinline__ int k_swz(int key) {
    constexpr int CPR = D / 8;                         // 16-B chunks per row
    constexpr int RPW = (128 / D) > 0 ? (128 / D) : 1; // rows per 256-B bank window
    return (key / RPW) % CPR;
}
// MODE = cache_mode (0 contiguous slots, 1 paged): a compile-time split keeps the page-table load and its wait out of the
// contiguous kernel's prefetch pipeline.  V tile in LDS and its transposing read: k_attn_dev.h.
template <int QBIT, int D, int MODE>
__global__ __launch_bounds__(PF_THREADS) void attn_prefill_kernel(const uint16_t* __restrict__ qkv, KvAddr kv,
                                                                  const int64_t* __restrict__ seq_starts,
                                                                  const int64_t* __restrict__ start_pos,
                                                                  const int64_t* __restrict__ cache_indices,
                                                                  int64_t max_pages, int64_t b0, int H, int Hkv,
                                                                  int nreq, int nqb, uint16_t* __restrict__ out) {
    using C = AttnCfg<QBIT, D>;
    constexpr int CH = C::CH, LPT = C::LPT;   // channels in one 16-byte piece, pieces per row
    constexpr int KSTEPS = D / 32;
    constexpr int DT = D / 16;
    constexpr int NITEMS = (PF_BN / 2) * LPT;                                // (key pair, piece) staging items per tile
    constexpr int IPT = (NITEMS + PF_THREADS - 1) / PF_THREADS;              // items per thread (1 or 2)
    __shared__ __attribute__((aligned(16))) uint16_t Ks[PF_BN * D];
    __shared__ __attribute__((aligned(16))) uint16_t Vs[(PF_BN / 16) * (D / 16) * ATT_VSUB];

    int hq, qb, r;   // 1-D grid in the XCD-aware order
    xcd_head_order(blockIdx.x, H, nqb, nreq, hq, qb, r);
    const int64_t b = b0 + r;
    const int hk = hq / (H / Hkv);
    const int64_t seqlen = seq_starts[b + 1] - seq_starts[b];
    const int64_t q0 = (int64_t)(nqb - 1 - qb) * PF_BM;
    if (q0 >= seqlen) return;
    const int64_t sp = start_pos[b];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int64_t rowstride = (int64_t)(H + 2 * Hkv) * D;

    // Q fragments: B operand, lane (n = query row l15, kq) holds Q[row][ks*32 + kq*8 .. +8]
    const int64_t wrow0 = q0 + wave * 16;  // first query row of this wave
    int64_t qi = wrow0 + l15;
    if (qi >= seqlen) qi = seqlen - 1;
    const int64_t qpos = sp + qi;
    h8 qf[KSTEPS];
    f4 o[DT];
    const uint16_t* qrow = qkv + (seq_starts[b] + qi) * rowstride + (int64_t)hq * D;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const uint4 v = *reinterpret_cast<const uint4*>(qrow + ks * 32 + kq * 8);
        qf[ks] = __builtin_bit_cast(h8, v);
    }
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = f4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;
    const float sm_scale2 = 1.4426950408889634f / sqrtf((float)D);  // softmax scale x log2(e)

    const int64_t last_q = (q0 + PF_BM - 1 < seqlen - 1) ? q0 + PF_BM - 1 : seqlen - 1;
    const int64_t kv_end = sp + last_q + 1;   // keys needed by this block: [0, kv_end)
    const int ntiles = (int)((kv_end + PF_BN - 1) / PF_BN);
    // waves whose 16 rows lie entirely beyond the sequence still help staging but skip the MFMAs
    const bool wave_active = wrow0 < seqlen;

    const int64_t slot0 = MODE == 0 ? cache_indices[b] : 0;  // contiguous mode: first slot of the request
    const KvHead kh = kv_head<QBIT>(kv, hk);
    const char *const kbase = kh.kbase, *const vbase = kh.vbase;
    const uint16_t *const ksbase = kh.ksbase, *const vsbase = kh.vsbase;

    // ---- register staging of one tile: raw 16-byte pieces of two adjacent keys (+ their int8 group scales) ---------
    uint4 kraw[IPT][2], vraw[IPT][2];
    uint32_t ksc[IPT][2], vsc[IPT][2];  // int8: two fp16 scales (the piece's two groups of 8 channels); fp8: the row's 2^e; fp16: unset
    // Addressing (round 3: the address arithmetic of this lambda was 235 of a tile's ~620 VALU instructions per wave, in a VALU-bound
    // kernel): with contiguous slots the rows of a tile are consecutive slots, so the row base is ONE scalar 64-bit computation
    // per tile and a lane adds a 32-bit offset (key-in-tile x row pitch + piece); with pages, the two keys of an item share a page
    // whenever the page size is even (one table lookup per pair; shift addressing for power-of-two pages).
    const int64_t rowb = kh.rowb, srow = kh.srow;      // row pitch of the cache (bytes) and of the scales (halfs)
    const int rowb32 = (int)rowb, srow32 = (int)srow;  // a tile spans 128 rows: the lane part fits 32 bits
    const bool pair_in_page = MODE == 1 && (kv.page_size % 2 == 0);
    auto load_tile = [&](int tile) {
        const int64_t key0 = (int64_t)tile * PF_BN;
        const int last = (int)(kv_end - 1 - key0);  // >= 0: keys past kv_end re-read the last valid row (masked later: beyond every row's causal horizon)
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
            const int item = threadIdx.x + it * PF_THREADS;
            if (NITEMS % PF_THREADS == 0 || item < NITEMS) {  // compile-time true when the items fill the block (fp16, D = 64): no exec branch around the loads
                const int c = item % LPT, kp = item / LPT;
                if constexpr (MODE == 0) {
                    const char* kt = kbase + (slot0 + key0) * rowb;  // tile-uniform
                    const char* vt = vbase + (slot0 + key0) * rowb;
                    const uint16_t* kst = ksbase + (slot0 + key0) * srow;
                    const uint16_t* vst = vsbase + (slot0 + key0) * srow;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int kk = (2 * kp + e) < last ? (2 * kp + e) : last;
                        kraw[it][e] = *reinterpret_cast<const uint4*>(kt + (kk * rowb32 + c * 16));
                        vraw[it][e] = *reinterpret_cast<const uint4*>(vt + (kk * rowb32 + c * 16));
                        if constexpr (QBIT == 8) {
                            ksc[it][e] = *reinterpret_cast<const uint32_t*>(kst + (kk * srow32 + c * 2));
                            vsc[it][e] = *reinterpret_cast<const uint32_t*>(vst + (kk * srow32 + c * 2));
                        }
                        if constexpr (QBIT == KV_FP8) {   // the row's 2^e
                            ksc[it][e] = kst[kk * srow32];
                            vsc[it][e] = vst[kk * srow32];
                        }
                        if constexpr (QBIT == KV_I4G32) {   // the piece's scale
                            ksc[it][e] = kst[kk * srow32 + c];
                            vsc[it][e] = vst[kk * srow32 + c];
                        }
                    }
                } else {
                    const int k0i = (2 * kp) < last ? (2 * kp) : last, k1i = (2 * kp + 1) < last ? (2 * kp + 1) : last;
                    const int64_t s0 = kv_slot(kv, cache_indices, max_pages, b, key0 + k0i);
                    const int64_t s1 = pair_in_page ? s0 + (k1i - k0i) : kv_slot(kv, cache_indices, max_pages, b, key0 + k1i);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int64_t slot = e ? s1 : s0;
                        kraw[it][e] = *reinterpret_cast<const uint4*>(kbase + slot * rowb + c * 16);
                        vraw[it][e] = *reinterpret_cast<const uint4*>(vbase + slot * rowb + c * 16);
                        if constexpr (QBIT == 8) {
                            ksc[it][e] = *reinterpret_cast<const uint32_t*>(ksbase + slot * srow + c * 2);
                            vsc[it][e] = *reinterpret_cast<const uint32_t*>(vsbase + slot * srow + c * 2);
                        }
                        if constexpr (QBIT == KV_FP8) {
                            ksc[it][e] = ksbase[slot * srow];
                            vsc[it][e] = vsbase[slot * srow];
                        }
                        if constexpr (QBIT == KV_I4G32) {
                            ksc[it][e] = ksbase[slot * srow + c];
                            vsc[it][e] = vsbase[slot * srow + c];
                        }
                    }
                }
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < IPT; ++it) {
            const int item = threadIdx.x + it * PF_THREADS;
            if (NITEMS % PF_THREADS == 0 || item < NITEMS) {  // compile-time true when the items fill the block (fp16, D = 64): no exec branch around the loads
                const int c = item % LPT, kp = item / LPT;
                const int ch0 = c * CH;
                // the piece as CH/8 groups of 8 fp16, per key of the pair
                h8 kf[2][CH / 8], vf[2][CH / 8];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if constexpr (QBIT == 8) {   // dequant_piece's own text: through the function three int8 kernels gained 1-3 s_nop / s_waitcnt
                        const h8 k0 = cvt_i8x8_f16(make_uint2(kraw[it][e].x, kraw[it][e].y)), k1 = cvt_i8x8_f16(make_uint2(kraw[it][e].z, kraw[it][e].w));
                        const h8 v0 = cvt_i8x8_f16(make_uint2(vraw[it][e].x, vraw[it][e].y)), v1 = cvt_i8x8_f16(make_uint2(vraw[it][e].z, vraw[it][e].w));
                        const h2 ksc2 = __builtin_bit_cast(h2, ksc[it][e]), vsc2 = __builtin_bit_cast(h2, vsc[it][e]);
                        kf[e][0] = k0 * ksc2[0]; kf[e][1] = k1 * ksc2[1];
                        vf[e][0] = v0 * vsc2[0]; vf[e][1] = v1 * vsc2[1];
                    } else if constexpr (QBIT == KV_FP8 || QBIT == KV_I4G32) {
                        dequant_piece<QBIT>(kraw[it][e], ksc[it][e], kf[e]);
                        dequant_piece<QBIT>(vraw[it][e], vsc[it][e], vf[e]);
                    } else {   // (no scales: nothing was loaded into ksc / vsc)
                        kf[e][0] = __builtin_bit_cast(h8, kraw[it][e]);
                        vf[e][0] = __builtin_bit_cast(h8, vraw[it][e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int key = 2 * kp + e;
#pragma unroll
                    for (int cc = 0; cc < CH / 8; ++cc) {
                        const int chunk = (ch0 / 8 + cc) ^ k_swz<D>(key);
                        *reinterpret_cast<uint4*>(&Ks[key * D + chunk * 8]) = __builtin_bit_cast(uint4, kf[e][cc]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int key = 2 * kp + e;
#pragma unroll
                    for (int cc = 0; cc < CH / 8; ++cc) {
                        const int ch = ch0 + cc * 8;
                        *reinterpret_cast<uint4*>(&Vs[ATT_V_OFF(D, key, ch)]) = __builtin_bit_cast(uint4, vf[e][cc]);
                    }
                }
            }
        }
    };

    load_tile(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int64_t key0 = (int64_t)tile * PF_BN;
        store_tile();
        __syncthreads();
        if (tile + 1 < ntiles) load_tile(tile + 1);  // in flight during the MFMAs below

        // a wave whose rows all end before this tile starts has nothing to add (causal)
        const int64_t wlast = (wrow0 + 15 < seqlen - 1) ? wrow0 + 15 : seqlen - 1;
        if (wave_active && key0 <= sp + wlast) {
            // ---- S^T = K . Q^T : 8 key tiles of 16 ------------------------------------------------------------
            f4 sacc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) sacc[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int key = j * 16 + l15;
                    const int chunk = (ks * 4 + kq) ^ k_swz<D>(key);
                    const h8 a = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&Ks[key * D + chunk * 8]));
                    sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], sacc[j], 0, 0, 0);
                }
            }
            // ---- online softmax for query row l15; this lane holds keys j*16 + kq*4 + r -----------------------
            // scores are kept in the log2 domain (scale * log2(e) folded into one multiply, v_exp_f32 is 2^x); the causal
            // mask costs two VALU per score and is only applied on tiles that reach the wave's diagonal
            const bool need_mask = key0 + PF_BN - 1 > sp + wrow0;  // wave-uniform: some key of the tile may exceed a row's position
            float mx = -1e30f;
            if (need_mask) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t kpos = key0 + j * 16 + kq * 4 + r;
                        const float sv = (kpos <= qpos) ? sacc[j][r] * sm_scale2 : -1e30f;
                        sacc[j][r] = sv;
                        mx = fmaxf(mx, sv);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sv = sacc[j][r] * sm_scale2;
                        sacc[j][r] = sv;
                        mx = fmaxf(mx, sv);
                    }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mnew = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f(m - mnew);
            m = mnew;
            float rs = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __builtin_amdgcn_exp2f(sacc[j][r] - mnew);  // masked scores: 2^(-1e30 - m) = 0
                    sacc[j][r] = e;
                    rs += e;
                }
            rs += __shfl_xor(rs, 16, 64);
            rs += __shfl_xor(rs, 32, 64);
            l = l * alpha + rs;
            // rescale O only when some row's maximum moved (rare after the first tiles): its C layout has rows
            // (kq*4 + r) -> fetch alpha of those query rows
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
                float ar[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, kq * 4 + r, 64);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[dt][r] *= ar[r];
            }
            // ---- O += P . V : A = P (this lane's 8 keys per k-step: tiles 2s, 2s+1) as an exact hi + lo pair (p_hi_lo: two
            // MFMAs), B = V^T from LDS ---------------------------------------------------------------------------
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                h8 pa, pl;
                {
                    float p[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) p[i] = sacc[2 * s2 + (i >> 2)][i & 3];
                    p_hi_lo(p, pa, pl);
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    // (the lane's key rows 4 kq go into the sub-tile pointer: passed as r0 the fp16 kernels lost a prologue shift)
                    const uint2 lo = v_frag_tr(Vs + (((2 * s2) * DT + dt) * ATT_VSUB + kq * 64), 0, l15);      // keys 16*(2s) + kq*4 .. +4 of channel dt*16 + l15
                    const uint2 hi = v_frag_tr(Vs + (((2 * s2 + 1) * DT + dt) * ATT_VSUB + kq * 64), 0, l15);
                    const h8 bv = __builtin_bit_cast(h8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pl, bv, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, bv, o[dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // ---- epilogue: O / l, fp16, rows kq*4 + r of this wave ---------------------------------------------------------
    float lr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lr[r] = __shfl(l, kq * 4 + r, 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t qrow_i = wrow0 + kq * 4 + r;
        if (qrow_i < seqlen) {
            uint16_t* orow = out + ((seq_starts[b] + qrow_i) * H + hq) * (int64_t)D;
            const float inv = 1.0f / lr[r];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) orow[dt * 16 + l15] = f2h(o[dt][r] * inv);
        }
    }
}

hipError_t launch_attn_prefill(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt,
                               const int64_t* seq_starts, const int64_t* start_pos, const int64_t* cache_indices,
                               int64_t max_pages, int64_t b0, int64_t B, int H, int Hkv, int D, int64_t max_seq_len,
                               uint16_t* out, int64_t max_kv_len, float* ws, size_t ws_bytes, int64_t row0, int64_t nrows) {
    if (B <= b0 || max_seq_len <= 0) return hipSuccess;
    if (kv_fmt != KV_FP16 && kv_fmt != KV_I8G8 && kv_fmt != KV_FP8 && kv_fmt != KV_I4G32) return hipErrorInvalidValue;
    // head_dim 128: the 32-row kernel of k_attn_prefill32.hip
    if (D == 128) return launch_attn_prefill32(s, qkv, kv, kv_fmt, seq_starts, start_pos, cache_indices, max_pages, b0, B, H, Hkv, D, max_seq_len, out, max_kv_len, ws, ws_bytes, row0, nrows);
    if (D != 64 && D != 32) return hipErrorInvalidValue;
    const int nqb = (int)((max_seq_len + PF_BM - 1) / PF_BM), nreq = (int)(B - b0);
    dim3 grid((unsigned)((int64_t)nqb * nreq * H));
    dispatch_int<KV_I8G8, KV_FP16, KV_FP8, KV_I4G32>(kv_fmt, [&](auto QB) {
        dispatch_int<64, 32>(D, [&](auto DD) {
            dispatch_int<0, 1>(kv.mode, [&](auto MD) {
                hipLaunchKernelGGL((attn_prefill_kernel<QB, DD, MD>), grid, dim3(PF_THREADS), 0, s, qkv, kv, seq_starts, start_pos, cache_indices,
                                   max_pages, b0, H, Hkv, nreq, nqb, out);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace pplhip
