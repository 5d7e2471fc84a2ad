// Sliding-window attention (window W >= 1: the query at absolute position p attends keys max(0, p - W + 1) .. p, HF Mistral's mask), head_dim
// 128, KV fp16 / int8-g8, contiguous and paged cache.  Two parts:
//
// 1. attn_band_prefill_kernel -- prefill and cache-prefill rows.  The wave tile of k_attn_prefill32.hip (a wave owns 32 query rows on
//    mfma_f32_32x32x16_f16, S^T = K . Q^T so that the softmax is lane-local plus one exchange with lane ^ 32, 64-key K / V tiles
//    double-buffered in LDS with ONE barrier per tile, exact hi + lo P, V through the transposing LDS read, xcd_head_order), with a key loop
//    of its own: the block of query rows [q0, q0 + BM) of a request at start_pos sp walks only the 64-key tiles that meet its BAND, keys
//    max(0, sp + q0 - W + 1) .. sp + min(q0 + BM, seqlen) - 1 -- about (W + BM) / 64 tiles however long the prompt is, where the causal kernel
//    walks (sp + q0 + BM) / 64.  Tiles are 64-aligned in absolute key positions; a load never goes below the band's first key (rows of the
//    first tile in front of it re-read that key and are masked), so the paged form touches no page below the band's first.
//    Per wave a tile is one of (wave-uniform, decided from scalars):
//      outside     every key above every row's position, or below every row's window: skipped, no MFMA
//      interior    every key inside every one of the wave's 32 rows' windows: NO mask instructions
//      upper edge  some key may exceed a row's position: causal mask j <= p
//      lower edge  some key may lie below a row's window: mask j >= p - W + 1
//    (W < 64 + 32: one tile can be both edges; the edge path applies both bounds, each of which is a no-op where it does not bind).
//    A ROW may meet a tile in which all its keys are masked -- the first tiles of a block for its later rows, the last for its earlier rows,
//    always when W < BM.  Masked scores are -inf while the running maximum starts FINITE (-1e30): such a tile gives the row mx = -inf,
//    mnew = m, alpha = 2^0 = 1 and p = 2^(-inf) = 0 exactly, so (m, l, O) stay as they are and no exp(-inf - -inf) is ever formed; a row
//    whose m is still -1e30 when its first visible key arrives gets alpha = 2^(-huge) = 0 on l = 0, O = 0.
//    No split-KV form: a short suffix behind a long prefix walks at most W + BM keys.  Work per block is roughly uniform for long
//    prompts (the band's width), so the heaviest-first query-block order of xcd_head_order is kept but no longer matters much: only the
//    first W / BM blocks of a request are lighter.
//
// 2. Windowed decode rows.  The host (rt_window.cc) shifts a row's position and its first slot / its page table to the window's first
//    key f = max(0, pos - W + 1); on a contiguous cache the ordinary decode kernels then run unchanged.  On a paged cache the table can
//    only start at a page, so the row carries skip = f % page_size keys in front of its window: the WIN = 1 forms of attn_decode_body
//    (k_attn_decode_dev.h) and of the grouped-query body (k_attn_decode_gqa_dev.h), instantiated here, leave them out.
// Numerics: P an exact hi + lo pair; fp16 K / V as they are; int8 K / V as exact hi + lo pairs (Q . K_lo + Q . K_hi, P . V_hi + P_hi . V_lo)
// in a second LDS image of each -- unlike the causal 32-row kernel, which rounds int8 x scale to fp16 once; the decode forms: those of
// the kernels they are (DESIGN.md numerics).  Oracle: ref_attention (oracle/llama_ref.c) under the band mask.
#include "k_attn_decode_dev.h"
#include "k_attn_decode_gqa_dev.h"

namespace pplhip {

namespace {

constexpr int BW_BN = 64, BW_D = 128;
constexpr int BW_KS_HALFS = BW_BN * BW_D, BW_VS_HALFS = (BW_BN / 16) * (BW_D / 16) * ATT_VSUB;
typedef float f16v __attribute__((ext_vector_type(16)));

// key (within a 32-key block) of score value i of lane half hi: the C layout of mfma_f32_32x32x16
__device__ __forceinline__ int crow(int i, int hi) { return (i & 3) + 8 * (i >> 2) + 4 * hi; }

template <int QBIT, int MODE, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_band_prefill_kernel(
    const uint16_t* __restrict__ qkv, KvAddr kv, const int64_t* __restrict__ seq_starts, const int64_t* __restrict__ start_pos,
    const int64_t* __restrict__ cache_indices, int64_t max_pages, int64_t b0, int H, int Hkv, int nreq, int nqb, int window,
    uint16_t* __restrict__ out) {
    static_assert(QBIT == KV_I8G8 || QBIT == KV_FP16, "the band kernel is built for int8-g8 and fp16 KV");
    constexpr int D = BW_D;
    constexpr int BM = NW * 32, THREADS = NW * 64;   // NW waves x 32 query rows share the staged K / V tiles
    using C = AttnCfg<QBIT, D>;
    constexpr int CH = C::CH, LPT = C::LPT;          // channels of a 16-byte piece, pieces per row: 16 x 8 (int8), 8 x 16 (fp16)
    constexpr int IPT = BW_BN * LPT / THREADS;       // (key, piece) items per thread and matrix: 2 / 4 (4 waves), 1 / 2 (8 waves)
    constexpr int KSTEPS = D / 16;
    // int8: K and V are staged as EXACT hi + lo pairs of fp16 numbers, hi = fp16(q x scale), lo = fma(q, scale, -hi) (two_product, as the
    // grouped-query decode kernel): a second image of each, LO_OFF halfs behind the first.  Rounded once (the causal 32-row kernel's form)
    // the output sat up to 2.6e-3 from attention over the exactly dequantised cache
    constexpr int NIMG = QBIT == KV_I8G8 ? 2 : 1;
    constexpr int LO_OFF = BW_KS_HALFS + BW_VS_HALFS, STAGE_HALFS = NIMG * LO_OFF;
    __shared__ __attribute__((aligned(16))) uint16_t smem[2 * STAGE_HALFS];

    int hq, qb, r;
    xcd_head_order(blockIdx.x, H, nqb, nreq, hq, qb, r);
    const int64_t b = b0 + r;
    const int hk = hq / (H / Hkv);
    const int64_t seqlen = seq_starts[b + 1] - seq_starts[b];
    const int64_t q0 = (int64_t)(nqb - 1 - qb) * BM;
    if (q0 >= seqlen) return;
    const int64_t sp = start_pos[b];
    const int64_t W = window;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, hi = lane >> 5, l15 = lane & 15, chblk = (lane >> 4) & 1;
    const int64_t rowstride = (int64_t)(H + 2 * Hkv) * D;

    const int64_t wrow0 = q0 + wave * 32;
    int64_t qi = wrow0 + l31;
    if (qi >= seqlen) qi = seqlen - 1;
    const int64_t qpos = sp + qi;
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
    float m = -1e30f, l = 0.f;
    const float sm_scale2 = 1.4426950408889634f / sqrtf((float)D);  // softmax scale x log2(e)

    // the block's band [key_lo, kv_end) and its tiles [t_lo, t_hi)
    const int64_t last_q = (q0 + BM - 1 < seqlen - 1) ? q0 + BM - 1 : seqlen - 1;
    const int64_t kv_end = sp + last_q + 1;
    const int64_t key_lo = sp + q0 - W + 1 > 0 ? sp + q0 - W + 1 : 0;
    const int t_lo = (int)(key_lo / BW_BN), t_hi = (int)((kv_end + BW_BN - 1) / BW_BN);
    // the wave's rows: positions sp + wrow0 .. sp + wlast, window bounds wlow0 (first row's, the lowest) .. wlow1 (last row's)
    const bool wave_active = wrow0 < seqlen;
    const int64_t wlast = (wrow0 + 31 < seqlen - 1) ? wrow0 + 31 : seqlen - 1;
    const int64_t wpos0 = sp + wrow0, wpos1 = sp + wlast;
    const int64_t wlow0 = wpos0 - W + 1, wlow1 = wpos1 - W + 1;

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
#define BW_ITEM_KEY(it) ((int)(threadIdx.x + (it) * THREADS) / LPT)
#define BW_ITEM_PC(it) ((int)(threadIdx.x + (it) * THREADS) % LPT)
    // rows of the tile outside [key_lo, kv_end) re-read the band's first / last key (masked for every row)
#define BW_LOAD_ITEM(it, KR, VR, KC, VC)                                                                                        \
    do {                                                                                                                       \
        const int k0_ = BW_ITEM_KEY(it) > first_ ? BW_ITEM_KEY(it) : first_;                                                   \
        const int kk_ = k0_ < last_ ? k0_ : last_, pc_ = BW_ITEM_PC(it);                                                       \
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
#define BW_LOAD_TILE(TILE)                                                                                                     \
    do {                                                                                                                       \
        const int64_t key0_ = (int64_t)(TILE) * BW_BN;                                                                         \
        const int first_ = key_lo > key0_ ? (int)(key_lo - key0_) : 0;                                                         \
        const int last_ = (int)(kv_end - 1 - key0_);                                                                           \
        BW_LOAD_ITEM(0, kr0, vr0, kc0, vc0);                                                                                   \
        if constexpr (IPT >= 2) BW_LOAD_ITEM(1, kr1, vr1, kc1, vc1);                                                           \
        if constexpr (IPT == 4) {                                                                                              \
            BW_LOAD_ITEM(2, kr2, vr2, kc2, vc2);                                                                               \
            BW_LOAD_ITEM(3, kr3, vr3, kc3, vc3);                                                                               \
        }                                                                                                                      \
    } while (0)
    // dequantise one item -> stage.  K: fp16 [64 keys][128 channels], 16-byte chunks XOR-swizzled with (key & 15) (conflict-free b128
    // fragment reads); V: row-major [16 keys][16 channels] sub-tiles.  int8: the exact hi + lo pair of q x scale, the lo image LO_OFF halfs
    // behind the hi image (DESIGN.md numerics, sliding-window row)
#define BW_STORE_ITEM(it, KR, VR, KC, VC)                                                                                       \
    do {                                                                                                                       \
        const int key = BW_ITEM_KEY(it), ch0 = BW_ITEM_PC(it) * CH;                                                            \
        if constexpr (QBIT == KV_I8G8) {                                                                                       \
            const h8 k0 = cvt_i8x8_f16(make_uint2(KR.x, KR.y)), k1 = cvt_i8x8_f16(make_uint2(KR.z, KR.w));                     \
            const h8 v0 = cvt_i8x8_f16(make_uint2(VR.x, VR.y)), v1 = cvt_i8x8_f16(make_uint2(VR.z, VR.w));                     \
            const h2 ks2 = __builtin_bit_cast(h2, KC), vs2 = __builtin_bit_cast(h2, VC);                                       \
            h8 kh0, kl0, kh1, kl1, vh0, vl0, vh1, vl1;                                                                         \
            two_product(k0, ks2[0], kh0, kl0);                                                                                 \
            two_product(k1, ks2[1], kh1, kl1);                                                                                 \
            two_product(v0, vs2[0], vh0, vl0);                                                                                 \
            two_product(v1, vs2[1], vh1, vl1);                                                                                 \
            uint16_t* kd0 = &Kw[key * D + ((ch0 >> 3) ^ (key & 15)) * 8];                                                      \
            uint16_t* kd1 = &Kw[key * D + (((ch0 >> 3) + 1) ^ (key & 15)) * 8];                                                \
            *reinterpret_cast<uint4*>(kd0) = __builtin_bit_cast(uint4, kh0);                                                   \
            *reinterpret_cast<uint4*>(kd1) = __builtin_bit_cast(uint4, kh1);                                                   \
            *reinterpret_cast<uint4*>(kd0 + LO_OFF) = __builtin_bit_cast(uint4, kl0);                                          \
            *reinterpret_cast<uint4*>(kd1 + LO_OFF) = __builtin_bit_cast(uint4, kl1);                                          \
            uint16_t* vd = &Vw[((key >> 4) * (D / 16) + (ch0 >> 4)) * ATT_VSUB + (key & 15) * 16];                              \
            *reinterpret_cast<uint4*>(vd) = __builtin_bit_cast(uint4, vh0);                                                    \
            *reinterpret_cast<uint4*>(vd + 8) = __builtin_bit_cast(uint4, vh1);                                                \
            *reinterpret_cast<uint4*>(vd + LO_OFF) = __builtin_bit_cast(uint4, vl0);                                           \
            *reinterpret_cast<uint4*>(vd + LO_OFF + 8) = __builtin_bit_cast(uint4, vl1);                                       \
        } else {                                                                                                               \
            *reinterpret_cast<uint4*>(&Kw[key * D + ((ch0 >> 3) ^ (key & 15)) * 8]) = KR;                                      \
            *reinterpret_cast<uint4*>(&Vw[((key >> 4) * (D / 16) + (ch0 >> 4)) * ATT_VSUB + (key & 15) * 16 + (ch0 & 15)]) = VR; \
        }                                                                                                                      \
    } while (0)

    BW_LOAD_TILE(t_lo);   // (t_lo < t_hi: the band holds the block's own keys)
    for (int tile = t_lo; tile < t_hi; ++tile) {
        const int64_t key0 = (int64_t)tile * BW_BN;
        {   // dequantise the tile loaded during the previous iteration -> stage (tile - t_lo) & 1
            uint16_t* Kw = smem + ((tile - t_lo) & 1) * STAGE_HALFS;
            uint16_t* Vw = Kw + BW_KS_HALFS;
            BW_STORE_ITEM(0, kr0, vr0, kc0, vc0);
            if constexpr (IPT >= 2) BW_STORE_ITEM(1, kr1, vr1, kc1, vc1);
            if constexpr (IPT == 4) {
                BW_STORE_ITEM(2, kr2, vr2, kc2, vc2);
                BW_STORE_ITEM(3, kr3, vr3, kc3, vc3);
            }
        }
        __syncthreads();  // the tile is visible in its stage; every wave is past its reads of the other stage (tile - 1)
        // the next tile's loads are in flight during the MFMAs below; unconditional (the last iteration re-reads its own tile and drops it)
        BW_LOAD_TILE(tile + 1 < t_hi ? tile + 1 : tile);
        const uint16_t* Ks = smem + ((tile - t_lo) & 1) * STAGE_HALFS;
        const uint16_t* Vs = Ks + BW_KS_HALFS;
        // outside: all keys above the wave's last position, or all below its first row's window
        if (wave_active && key0 <= wpos1 && key0 + BW_BN - 1 >= wlow0) {
            // ---- S^T = K . Q^T: two 32-key blocks, K fragments two k-steps ahead of their MFMAs in named registers ------------------
            f16v sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#define BW_KFRAG(KP, ks, kb) __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&(KP)[((kb) * 32 + l31) * D + ((2 * (ks) + hi) ^ (l31 & 15)) * 8]))
            // one pass over a K image; the order is pinned: 4 reads | (2 MFMAs, 2 reads) x 6 | 4 MFMAs
#define BW_S_PASS(KP)                                                                                                          \
    do {                                                                                                                       \
        h8 ka0 = BW_KFRAG(KP, 0, 0), kb0 = BW_KFRAG(KP, 0, 1), ka1 = BW_KFRAG(KP, 1, 0), kb1 = BW_KFRAG(KP, 1, 1);             \
        _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ks += 2) {                                                             \
            sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka0, qf[ks], sacc[0], 0, 0, 0);                                   \
            sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kb0, qf[ks], sacc[1], 0, 0, 0);                                   \
            if (ks + 2 < KSTEPS) { ka0 = BW_KFRAG(KP, ks + 2, 0); kb0 = BW_KFRAG(KP, ks + 2, 1); }                             \
            sacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka1, qf[ks + 1], sacc[0], 0, 0, 0);                               \
            sacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kb1, qf[ks + 1], sacc[1], 0, 0, 0);                               \
            if (ks + 3 < KSTEPS) { ka1 = BW_KFRAG(KP, ks + 3, 0); kb1 = BW_KFRAG(KP, ks + 3, 1); }                             \
        }                                                                                                                      \
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                                                     \
        _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ++ks) {                                                                \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                                                 \
            if (ks + 2 < KSTEPS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                            \
        }                                                                                                                      \
    } while (0)
            if constexpr (NIMG == 2) BW_S_PASS(Ks + LO_OFF);   // int8: Q . K_lo first (the small terms), then Q . K_hi
            BW_S_PASS(Ks);
#undef BW_S_PASS
#undef BW_KFRAG
            // ---- the tile's class (wave-uniform scalars).  Edge: key index idx of the tile is visible to this lane's query iff
            // lo_rel <= idx <= hi_rel; the bound that does not bind for the wave is still right for the lane.  Interior: nothing ----------
            const bool upper_edge = key0 + BW_BN - 1 > wpos0, lower_edge = key0 < wlow1;
            if (upper_edge || lower_edge) {
                const int64_t dh = qpos - key0, dl = dh - W + 1;
                const int hi_rel = dh < 0 ? -1 : (dh > 2 * BW_BN ? 2 * BW_BN : (int)dh);
                const int lo_rel = dl < 0 ? 0 : (dl > 2 * BW_BN ? 2 * BW_BN : (int)dl);
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int idx = 32 * kb + crow(i, hi);
                        sacc[kb][i] = (idx <= hi_rel && idx >= lo_rel) ? sacc[kb][i] : -INFINITY;
                    }
            }
            // ---- online softmax of query l31 (header: a wholly masked tile leaves the row's m, l, O untouched) ---------------------------
            float mx0 = sacc[0][0], mx1 = sacc[1][0];
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                mx0 = fmaxf(mx0, sacc[0][i]);
                mx1 = fmaxf(mx1, sacc[1][i]);
            }
            float mx = fmaxf(mx0, mx1);
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])), mx);  // own value and lane ^ 32's
            }
            const float mnew = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f((m - mnew) * sm_scale2);
            m = mnew;
            const float nmc = -mnew * sm_scale2;
            float rs4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][i], sm_scale2, nmc));  // masked scores: 2^(-inf) = 0
                    sacc[kb][i] = e;
                    rs4[i & 3] += e;
                }
            float rs = (rs4[0] + rs4[1]) + (rs4[2] + rs4[3]);
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
                rs = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
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
                    if constexpr (NIMG == 2) {   // int8: P_hi . V_lo (P_lo . V_lo is 2^-22 of the product: left out)
                        const uint2 w0 = v_frag_tr(sub + LO_OFF, 4 * hi, l15), w1 = v_frag_tr(sub + LO_OFF, 8 + 4 * hi, l15);
                        o[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa, __builtin_bit_cast(h8, make_uint4(w0.x, w0.y, w1.x, w1.y)), o[c], 0, 0, 0);
                    }
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

#undef BW_LOAD_TILE
#undef BW_LOAD_ITEM
#undef BW_STORE_ITEM
#undef BW_ITEM_KEY
#undef BW_ITEM_PC

// the multi-head decode kernel's WIN form (k_attn_decode.hip attn_decode_kernel plus skip)
template <int QBIT>
__global__ void attn_decode_win_kernel(const uint16_t* __restrict__ qkv, KvAddr kv, const int64_t* __restrict__ seq_starts,
                                       const int64_t* __restrict__ start_pos, const int64_t* __restrict__ cache_indices, int64_t max_pages,
                                       int H, int Hkv, int split, float* __restrict__ workspace, uint16_t* __restrict__ out,
                                       const int32_t* __restrict__ skip) {
    extern __shared__ __attribute__((aligned(16))) float dsmem[];  // [NW][D + 2]
    attn_decode_body<QBIT, BW_D, 1>(qkv, kv, seq_starts, start_pos, cache_indices, max_pages, H, Hkv, split, workspace, out, (int)blockIdx.x,
                                    (int64_t)blockIdx.y, (int)blockIdx.z, (int)(blockDim.x >> 6), dsmem, skip);
}

}  // namespace

bool attn_window_supported(int kv_fmt, int D) { return D == BW_D && (kv_fmt == KV_FP16 || kv_fmt == KV_I8G8); }

hipError_t launch_attn_prefill_window(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                      const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t b0, int64_t B, int H,
                                      int Hkv, int D, int64_t max_seq_len, int window, uint16_t* out) {
    if (!attn_window_supported(kv_fmt, D) || window < 1 || Hkv <= 0 || H % Hkv) return hipErrorInvalidValue;
    if (B <= b0 || max_seq_len <= 0) return hipSuccess;
    const int nreq = (int)(B - b0);
    // 8 waves (256 query rows share a staged tile) once the sequences are long, as the causal kernel; a block then walks (W + 256) / 64 tiles
    // int8: always 8 waves -- the exact hi + lo stages fill 132 KiB of LDS, one block per CU either way, and 8 waves keep 2 per SIMD
    const int nw = (max_seq_len >= 1024 || kv_fmt == KV_I8G8) ? 8 : 4;
    const int nqb = (int)((max_seq_len + nw * 32 - 1) / (nw * 32));
    const dim3 grid((unsigned)((int64_t)nqb * nreq * H));
    dispatch_int<KV_I8G8, KV_FP16>(kv_fmt, [&](auto QB) {
        dispatch_int<0, 1>(kv.mode, [&](auto MD) {
            dispatch_int<8, 4>(nw, [&](auto NW) {
                if constexpr (QB != KV_I8G8 || NW == 8)
                    hipLaunchKernelGGL((attn_band_prefill_kernel<QB, MD, NW>), grid, dim3(NW * 64), 0, s, qkv, kv, seq_starts, start_pos,
                                       cache_indices, max_pages, b0, H, Hkv, nreq, nqb, window, out);
            });
        });
    });
    return hipGetLastError();
}

hipError_t launch_attn_decode_window(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                     const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, const int32_t* skip, int64_t nb,
                                     int H, int Hkv, int D, int split, int threads, float* workspace, uint16_t* out) {
    if (nb == 0) return hipSuccess;
    if (!attn_window_supported(kv_fmt, D) || kv.mode != 1 || !skip || Hkv <= 0 || H % Hkv) return hipErrorInvalidValue;
    if (threads < 64 || threads > 64 * DEC_MAX_WAVES || threads % 64) return hipErrorInvalidValue;
    if (threads < D) threads = D;  // the final merge uses one thread per channel
    if (split < 1) split = 1;
    if (attn_decode_gqa_supported(kv_fmt, H, Hkv, D)) {   // the launch rule of launch_attn_decode_gqa
        const bool small = (int64_t)Hkv * nb * split >= GQ_SMALL_BLOCK_MIN;
        dispatch_int<KV_I8G8, KV_FP16>(kv_fmt, [&](auto QB) {
            dispatch_int<GQ_WAVES_SMALL, GQ_WAVES_BIG>(small ? GQ_WAVES_SMALL : GQ_WAVES_BIG, [&](auto NW) {
                const auto kernel = attn_decode_gqa_kernel<QB, BW_D, 1, NW, const int32_t*>;
                constexpr int lds = gq_lds_bytes<QB, BW_D, NW>();
                if constexpr (lds > 65536) {
                    static std::mutex mu;
                    static LdsOptIn once;
                    std::lock_guard<std::mutex> g(mu);
                    if (once.first()) set_max_lds(lds, kernel);
                }
                hipLaunchKernelGGL(kernel, dim3((unsigned)Hkv, (unsigned)nb, (unsigned)split), dim3(NW * 64), lds, s, qkv, kv, seq_starts, start_pos,
                                   cache_indices, max_pages, H, Hkv, split, workspace, out, skip);
            });
        });
    } else {
        const size_t lds = (size_t)(threads / 64) * (BW_D + 2) * sizeof(float);
        dispatch_int<KV_I8G8, KV_FP16>(kv_fmt, [&](auto QB) {
            hipLaunchKernelGGL((attn_decode_win_kernel<QB>), dim3(H, (unsigned)nb, split), dim3(threads), lds, s, qkv, kv, seq_starts, start_pos,
                               cache_indices, max_pages, H, Hkv, split, workspace, out, skip);
        });
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || split == 1) return e;
    return launch_attn_reduce(s, workspace, split, nb * H, D, out);
}

}  // namespace pplhip
