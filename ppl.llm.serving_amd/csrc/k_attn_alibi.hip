// ALiBi attention (Press et al., "Attention with Linear Biases"; Baichuan-13B, Bloom, MPT): q and k are not rotated, and the score of the
// query at absolute position p against the key at absolute position j <= p is dot(q, k_j) / sqrt(D) + slope[h] * (j - p), softmax as ever.
// Multi-head (H == Hkv), head_dim 128, KV fp16 / int8-g8, contiguous and paged cache.  Two parts:
//
// 1. attn_alibi_prefill_kernel -- prefill and cache-prefill rows.  The wave tile of k_attn_prefill32.hip, unchanged in everything but the
//    scores: a wave owns 32 query rows on mfma_f32_32x32x16_f16, S^T = K . Q^T so that lane (query l31, half hi) holds 16 scores of ITS query per
//    32-key block, keys key0 + 32 kb + crow(i, hi); 64-key K / V tiles double-buffered in LDS with one barrier per tile, the next tile's
//    global loads in flight during the MFMAs; P an exact hi + lo pair; int8 x scale rounded to fp16 once; xcd_head_order; the causal
//    upper-edge mask on the tiles that need it.
//    The bias.  With one query per lane, j - p = crow(i, 0) + (key0 + 32 kb + 4 hi - p): a part that depends on the value index alone -- the
//    same for every lane, every tile and every query -- and a part that is one number per lane and 32-key block.  The kernel works in RAW
//    score units like its parent (the softmax scale is folded into the exponent's fma), so the slope is taken into them once,
//    r = slope * sqrt(D), and
//      bvec[i]  = r * crow(i, 0)                  16 numbers built once in front of the key loop and made wave-uniform for the compiler
//                                                 (readfirstlane): it may hold them in scalar registers wherever the vector file is full.
//                                                 As 16 lane registers r * crow(i, hi) they put the 4-wave fp16 forms 20 and 52 bytes per
//                                                 lane into scratch; in this form no instantiation spills (DESIGN.md has the report)
//      tb[kb]   = r * (key0 + 32 kb + 4 hi - p)   two numbers per lane and tile; the integer is an exact float
//      u[kb][i] = S[kb][i] + bvec[i]              ONE add per score -- as built, v_pk_add_f32 on pairs of scores, 16 instructions for the 32
//                                                 scores a lane holds per tile -- and all that a score pays
//    and tb never touches a score: it enters the block's maximum (max_i u[kb][i] + tb[kb], one add per block) and the offset of the
//    exponent's fma, p = 2^(u c + (tb[kb] - m) c) with m the running maximum of the biased scores -- the fma the parent already has, with a
//    per-block offset in place of -m c.  j - p is never formed per score, and no integer work is added per score.
//    Rounding.  Not the single fma of the decode form: r is rounded (sqrt(128) is no fp32 number), bvec[i] is rounded, the add is rounded,
//    and tb is rounded where it meets m -- each to half an ulp of a magnitude no larger than the bias itself, so the exponent is off by a few
//    2^-24 |bias| where one fma would be off by one: 1e-4 nats at a bias of 400 nats, on a key whose weight is e^-400.  Keys that carry
//    weight have a small bias and a small error.  (m is the rounded u + tb, so the leading key's p may be 2^(+-1e-6) rather than 1; l carries
//    the same factor and O / l does not see it.)  A head with slope == 0 has bvec = tb = 0: every added operation is x + 0 or 0 - x, exact, and
//    the kernel gives the parent's bits (a zero's sign can differ on the way; no output depends on it).
//    No split-KV form: launch_attn_prefill_alibi never splits the keys, whatever the suffix and prefix lengths are -- a short suffix behind a
//    long prefix runs as H x requests blocks that walk the prefix.
//
// 2. attn_decode_alibi_kernel -- decode rows: the ALIBI = 1 form of attn_decode_body (k_attn_decode_dev.h).  A block reads its head's slope
//    once; each key's scaled score gets fmaf(slope, (float)(j - p), score), j the key's absolute position in every split, so the partial rows
//    of a K-split merge through launch_attn_reduce as they are.  One rounding; slope == 0 gives launch_attn_decode's bits.
// Oracle: none in oracle/ (the reference project has no ALiBi); tests/test_gpu_attn_alibi.py carries float64 attention with the bias.
#include "k_attn_decode_dev.h"

namespace pplhip {

namespace {

constexpr int AB_BN = 64, AB_D = 128;
constexpr int AB_KS_HALFS = AB_BN * AB_D, AB_VS_HALFS = (AB_BN / 16) * (AB_D / 16) * ATT_VSUB;
typedef float f16v __attribute__((ext_vector_type(16)));

// key (within a 32-key block) of score value i of lane half hi: the C layout of mfma_f32_32x32x16
__device__ __forceinline__ int crow(int i, int hi) { return (i & 3) + 8 * (i >> 2) + 4 * hi; }

template <int QBIT, int MODE, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_alibi_prefill_kernel(
    const uint16_t* __restrict__ qkv, KvAddr kv, const int64_t* __restrict__ seq_starts, const int64_t* __restrict__ start_pos,
    const int64_t* __restrict__ cache_indices, int64_t max_pages, int64_t b0, int H, int Hkv, int nreq, int nqb,
    const float* __restrict__ slopes, uint16_t* __restrict__ out) {
    static_assert(QBIT == KV_I8G8 || QBIT == KV_FP16, "the ALiBi prefill kernel is built for int8-g8 and fp16 KV");
    constexpr int D = AB_D;
    constexpr int BM = NW * 32, THREADS = NW * 64;   // NW waves x 32 query rows share the staged K / V tiles
    using C = AttnCfg<QBIT, D>;
    constexpr int CH = C::CH, LPT = C::LPT;          // channels of a 16-byte piece, pieces per row: 16 x 8 (int8), 8 x 16 (fp16)
    constexpr int IPT = AB_BN * LPT / THREADS;       // (key, piece) items per thread and matrix: 2 / 4 (4 waves), 1 / 2 (8 waves)
    constexpr int KSTEPS = D / 16;
    constexpr int STAGE_HALFS = AB_KS_HALFS + AB_VS_HALFS;
    __shared__ __attribute__((aligned(16))) uint16_t smem[2 * STAGE_HALFS];

    int hq, qb, r;
    xcd_head_order(blockIdx.x, H, nqb, nreq, hq, qb, r);
    const int64_t b = b0 + r;
    const int hk = hq / (H / Hkv);
    const int64_t seqlen = seq_starts[b + 1] - seq_starts[b];
    const int64_t q0 = (int64_t)(nqb - 1 - qb) * BM;
    if (q0 >= seqlen) return;
    const int64_t sp = start_pos[b];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, hi = lane >> 5, l15 = lane & 15, chblk = (lane >> 4) & 1;
    const int64_t rowstride = (int64_t)(H + 2 * Hkv) * D;

    const int64_t wrow0 = q0 + wave * 32;
    int64_t qi = wrow0 + l31;
    if (qi >= seqlen) qi = seqlen - 1;
    const int64_t qpos = sp + qi;   // ABSOLUTE position of this lane's query: a cache-prefill row's bias counts from the cache's first key
    h8 qf[KSTEPS];  // B operand: lane (query l31, hi) holds channels 16 ks + 8 hi .. + 8
    {
        const uint16_t* qrow = qkv + (seq_starts[b] + qi) * rowstride + (int64_t)hq * D;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(qrow + ks * 16 + hi * 8));
    }
    f16v o[4];  // O^T blocks: lane = channel c32 * 32 + l31, values i = queries crow(i, hi)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[c][i] = 0.f;
    float m = -1e30f, l = 0.f;   // m: running maximum of the BIASED scores, raw units
    const float sm_scale2 = 1.4426950408889634f / sqrtf((float)D);  // softmax scale x log2(e)
    // the head's slope in raw score units, and the lane's part of the bias (header)
    const float slope_raw = slopes[hq] * sqrtf((float)D);
    float bvec[16];   // wave-uniform, pinned to scalar registers: the per-score add takes its bias as the instruction's scalar operand
#pragma unroll
    for (int i = 0; i < 16; ++i) bvec[i] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(slope_raw * (float)crow(i, 0))));

    const int64_t last_q = (q0 + BM - 1 < seqlen - 1) ? q0 + BM - 1 : seqlen - 1;
    const int64_t kv_end = sp + last_q + 1;
    const int ntiles = (int)((kv_end + AB_BN - 1) / AB_BN);
    const bool wave_active = wrow0 < seqlen;
    const int64_t wlast = (wrow0 + 31 < seqlen - 1) ? wrow0 + 31 : seqlen - 1;

    const int64_t slot0 = MODE == 0 ? cache_indices[b] : 0;
    const KvHead kh = kv_head<QBIT>(kv, hk);
    const char *const kbase = kh.kbase, *const vbase = kh.vbase;
    const uint16_t *const ksbase = kh.ksbase, *const vsbase = kh.vsbase;
    const int64_t rowb = kh.rowb, srow = kh.srow;
    const int rowb32 = (int)rowb, srow32 = (int)srow;

    // ---- staging registers of one 64-key tile: item (key, piece) = divmod(tid + THREADS it, LPT).  (Macros and named scalars, as in
    // k_attn_prefill32.hip: register arrays captured by reference or indexed in a loop end up in scratch memory.)
    uint4 kr0, kr1, kr2, kr3, vr0, vr1, vr2, vr3;
    uint32_t kc0 = 0, kc1 = 0, kc2 = 0, kc3 = 0, vc0 = 0, vc1 = 0, vc2 = 0, vc3 = 0;
    kr1 = kr2 = kr3 = vr1 = vr2 = vr3 = make_uint4(0, 0, 0, 0);
#define AB_ITEM_KEY(it) ((int)(threadIdx.x + (it) * THREADS) / LPT)
#define AB_ITEM_PC(it) ((int)(threadIdx.x + (it) * THREADS) % LPT)
    // rows past kv_end re-read the last valid row (beyond every row's causal horizon); contiguous slots: one scalar tile base plus
    // 32-bit lane offsets
#define AB_LOAD_ITEM(it, KR, VR, KC, VC)                                                                                        \
    do {                                                                                                                       \
        const int kk_ = AB_ITEM_KEY(it) < last_ ? AB_ITEM_KEY(it) : last_, pc_ = AB_ITEM_PC(it);                               \
        const char *kp_, *vp_;                                                                                                 \
        const uint16_t *ksp_, *vsp_;                                                                                           \
        if constexpr (MODE == 0) {                                                                                             \
            const int64_t sb_ = slot0 + key0_;                                                                                 \
            kp_ = kbase + sb_ * rowb + (kk_ * rowb32 + pc_ * 16);                                                              \
            vp_ = vbase + sb_ * rowb + (kk_ * rowb32 + pc_ * 16);                                                              \
            ksp_ = ksbase + sb_ * srow + (kk_ * srow32 + pc_ * 2);                                                             \
            vsp_ = vsbase + sb_ * srow + (kk_ * srow32 + pc_ * 2);                                                             \
        } else {                                                                                                               \
            const int64_t slot_ = kv_slot(kv, cache_indices, max_pages, b, key0_ + kk_);                                       \
            kp_ = kbase + slot_ * rowb + pc_ * 16;                                                                             \
            vp_ = vbase + slot_ * rowb + pc_ * 16;                                                                             \
            ksp_ = ksbase + slot_ * srow + pc_ * 2;                                                                            \
            vsp_ = vsbase + slot_ * srow + pc_ * 2;                                                                            \
        }                                                                                                                      \
        KR = *reinterpret_cast<const uint4*>(kp_);                                                                             \
        VR = *reinterpret_cast<const uint4*>(vp_);                                                                             \
        if constexpr (QBIT == KV_I8G8) {                                                                                       \
            KC = *reinterpret_cast<const uint32_t*>(ksp_);                                                                     \
            VC = *reinterpret_cast<const uint32_t*>(vsp_);                                                                     \
        }                                                                                                                      \
    } while (0)
#define AB_LOAD_TILE(TILE)                                                                                                     \
    do {                                                                                                                       \
        const int64_t key0_ = (int64_t)(TILE) * AB_BN;                                                                         \
        const int last_ = (int)(kv_end - 1 - key0_);                                                                           \
        AB_LOAD_ITEM(0, kr0, vr0, kc0, vc0);                                                                                   \
        if constexpr (IPT >= 2) AB_LOAD_ITEM(1, kr1, vr1, kc1, vc1);                                                           \
        if constexpr (IPT == 4) {                                                                                              \
            AB_LOAD_ITEM(2, kr2, vr2, kc2, vc2);                                                                               \
            AB_LOAD_ITEM(3, kr3, vr3, kc3, vc3);                                                                               \
        }                                                                                                                      \
    } while (0)
    // dequantise one item -> stage.  K: fp16 [64 keys][128 channels], 16-byte chunks XOR-swizzled with (key & 15) (conflict-free b128
    // fragment reads); V: row-major [16 keys][16 channels] sub-tiles.  int8: q x scale rounded to fp16 once, the causal kernel's form
#define AB_STORE_ITEM(it, KR, VR, KC, VC)                                                                                       \
    do {                                                                                                                       \
        const int key = AB_ITEM_KEY(it), ch0 = AB_ITEM_PC(it) * CH;                                                            \
        if constexpr (QBIT == KV_I8G8) {                                                                                       \
            const h8 k0 = cvt_i8x8_f16(make_uint2(KR.x, KR.y)), k1 = cvt_i8x8_f16(make_uint2(KR.z, KR.w));                     \
            const h8 v0 = cvt_i8x8_f16(make_uint2(VR.x, VR.y)), v1 = cvt_i8x8_f16(make_uint2(VR.z, VR.w));                     \
            const h2 ks2 = __builtin_bit_cast(h2, KC), vs2 = __builtin_bit_cast(h2, VC);                                       \
            const h8 kh0 = k0 * ks2[0], kh1 = k1 * ks2[1], vh0 = v0 * vs2[0], vh1 = v1 * vs2[1];                               \
            *reinterpret_cast<uint4*>(&Kw[key * D + ((ch0 >> 3) ^ (key & 15)) * 8]) = __builtin_bit_cast(uint4, kh0);          \
            *reinterpret_cast<uint4*>(&Kw[key * D + (((ch0 >> 3) + 1) ^ (key & 15)) * 8]) = __builtin_bit_cast(uint4, kh1);    \
            uint16_t* vd = &Vw[((key >> 4) * (D / 16) + (ch0 >> 4)) * ATT_VSUB + (key & 15) * 16];                              \
            *reinterpret_cast<uint4*>(vd) = __builtin_bit_cast(uint4, vh0);                                                    \
            *reinterpret_cast<uint4*>(vd + 8) = __builtin_bit_cast(uint4, vh1);                                                \
        } else {                                                                                                               \
            *reinterpret_cast<uint4*>(&Kw[key * D + ((ch0 >> 3) ^ (key & 15)) * 8]) = KR;                                      \
            *reinterpret_cast<uint4*>(&Vw[((key >> 4) * (D / 16) + (ch0 >> 4)) * ATT_VSUB + (key & 15) * 16 + (ch0 & 15)]) = VR; \
        }                                                                                                                      \
    } while (0)

    AB_LOAD_TILE(0);   // (ntiles >= 1: the block holds a row, and a row sees its own key)
    for (int tile = 0; tile < ntiles; ++tile) {
        const int64_t key0 = (int64_t)tile * AB_BN;
        {   // dequantise the tile loaded during the previous iteration -> stage tile & 1
            uint16_t* Kw = smem + (tile & 1) * STAGE_HALFS;
            uint16_t* Vw = Kw + AB_KS_HALFS;
            AB_STORE_ITEM(0, kr0, vr0, kc0, vc0);
            if constexpr (IPT >= 2) AB_STORE_ITEM(1, kr1, vr1, kc1, vc1);
            if constexpr (IPT == 4) {
                AB_STORE_ITEM(2, kr2, vr2, kc2, vc2);
                AB_STORE_ITEM(3, kr3, vr3, kc3, vc3);
            }
        }
        __syncthreads();  // the tile is visible in its stage; every wave is past its reads of the other stage (tile - 1)
        // the next tile's loads are in flight during the MFMAs below; unconditional (the last iteration re-reads its own tile and drops it)
        AB_LOAD_TILE(tile + 1 < ntiles ? tile + 1 : tile);
        const uint16_t* Ks = smem + (tile & 1) * STAGE_HALFS;
        const uint16_t* Vs = Ks + AB_KS_HALFS;
        if (wave_active && key0 <= sp + wlast) {  // causal: a wave whose rows all end before this tile has nothing to add
            // ---- S^T = K . Q^T: two 32-key blocks, K fragments two k-steps ahead of their MFMAs in named registers ------------------
            f16v sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#define AB_KFRAG(ks, kb) __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&Ks[((kb) * 32 + l31) * D + ((2 * (ks) + hi) ^ (l31 & 15)) * 8]))
            h8 ka0 = AB_KFRAG(0, 0), kb0 = AB_KFRAG(0, 1), ka1 = AB_KFRAG(1, 0), kb1 = AB_KFRAG(1, 1);
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks += 2) {
                sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka0, qf[ks], sacc[0], 0, 0, 0);
                sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kb0, qf[ks], sacc[1], 0, 0, 0);
                if (ks + 2 < KSTEPS) { ka0 = AB_KFRAG(ks + 2, 0); kb0 = AB_KFRAG(ks + 2, 1); }
                sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka1, qf[ks + 1], sacc[0], 0, 0, 0);
                sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kb1, qf[ks + 1], sacc[1], 0, 0, 0);
                if (ks + 3 < KSTEPS) { ka1 = AB_KFRAG(ks + 3, 0); kb1 = AB_KFRAG(ks + 3, 1); }
            }
#undef AB_KFRAG
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // pin that order: 4 reads | (2 MFMAs, 2 reads) x 6 | 4 MFMAs
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                if (ks + 2 < KSTEPS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            // ---- the bias: the value's part onto every score (one add each); the lane's and the blocks' part tb is two numbers per tile.
            // key0 + 4 hi - qpos fits an int, and a float exactly (positions stay far below 2^24) --------------------------------------------
            const int64_t d = qpos - key0;
            const float rel = (float)(4 * hi - (int)d);
            const float tb0 = slope_raw * rel, tb1 = slope_raw * (rel + 32.0f);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = sacc[kb][i] + bvec[i];
            // ---- online softmax of query l31.  Masked scores are -inf (and stay so under the bias) while m starts FINITE (-1e30): a row
            // whose tile is wholly masked keeps m, gets alpha = 2^0 and p = 2^(-inf) = 0 exactly --------------------------------------------
            if (key0 + AB_BN - 1 > sp + wrow0) {  // wave-uniform: some key of the tile may exceed a row's position
                const int qrel = d < 0 ? -1 : (d > 2 * AB_BN ? 2 * AB_BN : (int)d);  // keys of the tile with index <= qrel are visible
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        sacc[kb][i] = (32 * kb + crow(i, hi) <= qrel) ? sacc[kb][i] : -INFINITY;
            }
            float mx0 = sacc[0][0], mx1 = sacc[1][0];
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                mx0 = fmaxf(mx0, sacc[0][i]);
                mx1 = fmaxf(mx1, sacc[1][i]);
            }
            float mx = fmaxf(mx0 + tb0, mx1 + tb1);   // the blocks' maxima in common units
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])), mx);  // own value and lane ^ 32's
            }
            const float mnew = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f((m - mnew) * sm_scale2);
            m = mnew;
            const float nmc[2] = {(tb0 - mnew) * sm_scale2, (tb1 - mnew) * sm_scale2};   // the block's bias enters here, not per score
            float rs4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][i], sm_scale2, nmc[kb]));  // masked scores: 2^(-inf) = 0
                    sacc[kb][i] = e;
                    rs4[i & 3] += e;
                }
            float rs = (rs4[0] + rs4[1]) + (rs4[2] + rs4[3]);
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
                rs = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);  // one of the two is this lane's own sum, the other lane ^ 32's
            }
            l = l * alpha + rs;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {   // rescale O only when some row's maximum moved
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float ar = __shfl(alpha, crow(i, hi), 64);
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c][i] *= ar;
                }
            }
            // ---- O += P . V over four 16-key k-steps; P as an exact hi + lo pair ---------------------------------------------------------
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                h8 pa, pl;
                {
                    float p[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) p[i] = sacc[s >> 1][8 * (s & 1) + i];
                    p_hi_lo(p, pa, pl);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint16_t* sub = Vs + (s * (D / 16) + 2 * c + chblk) * ATT_VSUB;  // keys 16 s .. + 16, channels 32 c + 16 chblk .. + 16
                    const uint2 v0 = v_frag_tr(sub, 4 * hi, l15), v1 = v_frag_tr(sub, 8 + 4 * hi, l15);
                    const h8 bv = __builtin_bit_cast(h8, make_uint4(v0.x, v0.y, v1.x, v1.y));
                    o[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl, bv, o[c], 0, 0, 0);
                    o[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa, bv, o[c], 0, 0, 0);
                }
            }
        }
    }
    // ---- epilogue: O / l, fp16; value i of channel block c = query wrow0 + crow(i, hi), channel 32 c + l31 (l > 0: a row sees its own key)
    if (!wave_active) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int rr = crow(i, hi);
        const float lr = __shfl(l, rr, 64);
        const int64_t qrow_i = wrow0 + rr;
        if (qrow_i < seqlen) {
            uint16_t* orow = out + ((seq_starts[b] + qrow_i) * H + hq) * (int64_t)D;
            const float inv = 1.0f / lr;
#pragma unroll
            for (int c = 0; c < 4; ++c) orow[c * 32 + l31] = f2h(o[c][i] * inv);
        }
    }
}

#undef AB_LOAD_TILE
#undef AB_LOAD_ITEM
#undef AB_STORE_ITEM
#undef AB_ITEM_KEY
#undef AB_ITEM_PC

// the multi-head decode kernel's ALIBI form (k_attn_decode.hip attn_decode_kernel plus the slopes)
template <int QBIT>
__global__ void attn_decode_alibi_kernel(const uint16_t* __restrict__ qkv, KvAddr kv, const int64_t* __restrict__ seq_starts,
                                         const int64_t* __restrict__ start_pos, const int64_t* __restrict__ cache_indices, int64_t max_pages,
                                         int H, int Hkv, int split, float* __restrict__ workspace, uint16_t* __restrict__ out,
                                         const float* __restrict__ slopes) {
    extern __shared__ __attribute__((aligned(16))) float dsmem[];  // [NW][D + 2]
    attn_decode_body<QBIT, AB_D, 0, 1>(qkv, kv, seq_starts, start_pos, cache_indices, max_pages, H, Hkv, split, workspace, out, (int)blockIdx.x,
                                       (int64_t)blockIdx.y, (int)blockIdx.z, (int)(blockDim.x >> 6), dsmem, nullptr, slopes);
}

}  // namespace

bool attn_alibi_supported(int kv_fmt, int H, int Hkv, int D) { return D == AB_D && H > 0 && H == Hkv && (kv_fmt == KV_FP16 || kv_fmt == KV_I8G8); }

hipError_t launch_attn_prefill_alibi(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                     const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t b0, int64_t B, int H,
                                     int Hkv, int D, int64_t max_seq_len, const float* slopes, uint16_t* out) {
    if (!attn_alibi_supported(kv_fmt, H, Hkv, D) || !slopes) return hipErrorInvalidValue;
    if (B <= b0 || max_seq_len <= 0) return hipSuccess;
    const int nreq = (int)(B - b0);
    // launch_attn_prefill32's rule for the unsplit form: 8 waves (256 query rows share a staged tile) once the sequences are long
    const int nw = max_seq_len >= 1024 ? 8 : 4;
    const int nqb = (int)((max_seq_len + nw * 32 - 1) / (nw * 32));
    const dim3 grid((unsigned)((int64_t)nqb * nreq * H));
    dispatch_int<KV_I8G8, KV_FP16>(kv_fmt, [&](auto QB) {
        dispatch_int<0, 1>(kv.mode, [&](auto MD) {
            dispatch_int<8, 4>(nw, [&](auto NW) {
                hipLaunchKernelGGL((attn_alibi_prefill_kernel<QB, MD, NW>), grid, dim3(NW * 64), 0, s, qkv, kv, seq_starts, start_pos, cache_indices,
                                   max_pages, b0, H, Hkv, nreq, nqb, slopes, out);
            });
        });
    });
    return hipGetLastError();
}

hipError_t launch_attn_decode_alibi(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                    const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t nb, int H, int Hkv, int D,
                                    int split, int threads, float* workspace, const float* slopes, uint16_t* out) {
    if (nb == 0) return hipSuccess;
    if (!attn_alibi_supported(kv_fmt, H, Hkv, D) || !slopes) return hipErrorInvalidValue;
    if (threads < 64 || threads > 64 * DEC_MAX_WAVES || threads % 64) return hipErrorInvalidValue;
    if (threads < D) threads = D;  // the final merge uses one thread per channel
    if (split < 1) split = 1;
    if (split > 1 && !workspace) return hipErrorInvalidValue;
    const size_t lds = (size_t)(threads / 64) * (AB_D + 2) * sizeof(float);
    dispatch_int<KV_I8G8, KV_FP16>(kv_fmt, [&](auto QB) {
        hipLaunchKernelGGL((attn_decode_alibi_kernel<QB>), dim3(H, (unsigned)nb, split), dim3(threads), lds, s, qkv, kv, seq_starts, start_pos,
                           cache_indices, max_pages, H, Hkv, split, workspace, out, slopes);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || split == 1) return e;
    return launch_attn_reduce(s, workspace, split, nb * H, D, out);
}

}  // namespace pplhip
