// Device layer shared by the four attention kernels (k_attn_decode_dev.h / k_attn_decode.hip, k_attn_decode_gqa.hip, k_attn_prefill.hip,
// k_attn_prefill32.hip): the KV format's constants, one head's cache pointers, the XCD-aware block order, the V sub-tile and its
// transposing read, a 16-byte piece -> fp16, the exact P split and the log-sum-exp merge.
// Not every kernel takes every piece from here: where a helper changed a kernel's instruction count the kernel kept its own text, and
// a new KV format or a change of the KV addressing is an edit there as well as here:
//   kv_head        used by the multi-head decode and both prefill kernels; the grouped-query kernel spells its own four pointers
//   ATT_V_OFF      used by the 16-row prefill; the 32-row prefill (P3_STORE_ITEM) and the grouped-query kernel (stage_v) spell theirs
//   dequant_piece  used by the 16-row prefill's store_tile (fp8; int8 there and P3_STORE_ITEM keep their own conversion) and by the
//                  grouped-query stage_v's rounded int8 form (GQ_V_EXACT = 0); that kernel's fp8 V and fp8 scores keep their own;
//                  the int4 form (KV_I4G32) is used by the 16-row prefill and the grouped-query kernel (V and scores)
#pragma once
#include "kernels.h"
#include "k_launch.h"

namespace pplhip {

// a KV row of D channels in format QBIT (KV_FP16 / KV_I8G8 / KV_FP8 / KV_I4G32) as 16-byte pieces
template <int QBIT, int D>
struct AttnCfg {
    static constexpr int ELT = QBIT != KV_FP16 ? 1 : 2;   // bytes per slab element (int8 and fp8: a channel; int4: two channels)
    static constexpr int CH = QBIT == KV_I4G32 ? 32 : 16 / ELT;   // channels per piece (int4: a piece is one quant group)
    static constexpr int LPT = D / CH;        // pieces per row (multi-head decode: lanes per token row)
    static constexpr int TPW = 64 / LPT;      // multi-head decode: token rows per wave-load
    static constexpr int NG = CH / 8;         // int8: quant groups per piece (group = 8 channels); fp8: one scale per row; int4: unused
};

// K / V rows and scales of KV head hk from channel ch0 on; row (slot) r is at kbase + r * rowb bytes, its scales at ksbase + r * srow halfs
struct KvHead {
    const char *kbase, *vbase;
    const uint16_t *ksbase, *vsbase;
    int64_t rowb, srow;   // row pitch of the cache (bytes) and of the scales (halfs)
};
template <int QBIT>
__device__ __forceinline__ KvHead kv_head(const KvAddr& kv, int hk, int ch0 = 0) {
    constexpr int ELT = QBIT != KV_FP16 ? 1 : 2;
    KvHead h;
    h.kbase = reinterpret_cast<const char*>(kv.cache) + ((int64_t)hk * kv.sH + (QBIT == KV_I4G32 ? ch0 / 2 : ch0)) * ELT;
    h.vbase = h.kbase + kv.sKV * ELT;
    h.ksbase = kv.scale + (int64_t)hk * kv.ssH + (QBIT == KV_I8G8 ? ch0 / 8 : (QBIT == KV_I4G32 ? ch0 / 32 : 0));
    h.vsbase = h.ksbase + kv.ssKV;
    h.rowb = kv.sN * ELT;
    h.srow = kv.ssN;
    return h;
}

// Prefill grids are 1-D in an XCD-aware order: consecutive workgroup ids go round-robin over the 8 XCDs (each with its own 4 MiB L2), so
// XCD x takes the H / 8 consecutive query heads x H/8 .. (same KV head under grouped-query attention) and walks them one after the
// other, each head's query blocks heaviest (last) first: what an XCD runs at any moment reads ONE head's K / V, which then lives in
// its L2, and the launch ends with light blocks.  L = workgroup id -> query head hq, query block qb, request r.
__device__ __forceinline__ void xcd_head_order(int L, int H, int nqb, int nreq, int& hq, int& qb, int& r) {
    const int per = nqb * nreq;
    int rem;
    if ((H & 7) == 0) {
        const int j = L >> 3;
        hq = (L & 7) * (H >> 3) + j / per;
        rem = j % per;
    } else {
        hq = L / per;
        rem = L % per;
    }
    qb = rem / nreq;
    r = rem % nreq;
}

// V tile in LDS: row-major [16 keys][16 channels] fp16 sub-tiles of ATT_VSUB halfs (256 + 16 of skew: bank spread of the writes),
// sub-tile (key / 16, channel / 16) at (key / 16 * D/16 + channel / 16) * ATT_VSUB.  The P.V MFMA contracts over keys, so its B operand wants
// 4 keys of ONE channel per lane: gfx950's transposing LDS read delivers exactly that from the row-major image (lane l of a 16-lane
// group supplies the address of row l/4, columns (l%4)*4.. and receives column l of the [4][16] block --
// profiles/probes/lds_tr_read_probe.hip), so the staging writes V like K (16-byte stores, no shuffling).
constexpr int ATT_VSUB = 272;
// offset in halfs of (key, channel ch) in a V tile of head_dim D.  (A macro: as an inline function the same expression cost the staging
// loops of three kernels one to four address instructions; the 32-row prefill and the grouped-query kernel keep their own text.)
#define ATT_V_OFF(D, key, ch) ((((key) >> 4) * ((D) / 16) + ((ch) >> 4)) * ATT_VSUB + ((key) & 15) * 16 + ((ch) & 15))
// lane l15 of a 16-lane group receives keys r0 .. r0 + 3 of channel l15 of the sub-tile
typedef short att_s4 __attribute__((__vector_size__(4 * sizeof(short))));
__device__ __forceinline__ uint2 v_frag_tr(const uint16_t* sub, int r0, int l15) {
    const uint16_t* p = sub + (r0 + (l15 >> 2)) * 16 + (l15 & 3) * 4;
    const att_s4 w = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) att_s4*)p);
    return __builtin_bit_cast(uint2, w);
}

// the 16 int8 of a piece -> fp16, exact
__device__ __forceinline__ void cvt_i8x16_f16(uint4 raw, h8* q) {
    q[0] = cvt_i8x8_f16(make_uint2(raw.x, raw.y));
    q[1] = cvt_i8x8_f16(make_uint2(raw.z, raw.w));
}
// A 16-byte piece and its scale word -> CH / 8 groups of 8 fp16.  int8: times the group's fp16 scale in packed fp16 (sc = the piece's two
// scales; one rounding of q * scale, as the oracle's dequantisation); fp8: the row's power-of-two scale inside the conversion -- exact,
// no rounding; fp16: the piece itself; int4: the piece is one group of 32 channels -> four groups of 8 fp16 times its scale, exact.
template <int QBIT>
__device__ __forceinline__ void dequant_piece(uint4 raw, uint32_t sc, h8* out) {
    if constexpr (QBIT == KV_I8G8) {
        const h2 s2 = __builtin_bit_cast(h2, sc);
        cvt_i8x16_f16(raw, out);
        out[0] = out[0] * s2[0];
        out[1] = out[1] * s2[1];
    } else if constexpr (QBIT == KV_FP8) {
        const float s = h2f((uint16_t)sc);
        out[0] = cvt_fp8x8_f16(make_uint2(raw.x, raw.y), s);
        out[1] = cvt_fp8x8_f16(make_uint2(raw.z, raw.w), s);
    } else if constexpr (QBIT == KV_I4G32) {
        const _Float16 s = __builtin_bit_cast(_Float16, (uint16_t)sc);
        out[0] = cvt_i4x8_f16(raw.x, s);
        out[1] = cvt_i4x8_f16(raw.y, s);
        out[2] = cvt_i4x8_f16(raw.z, s);
        out[3] = cvt_i4x8_f16(raw.w, s);
    } else {
        out[0] = __builtin_bit_cast(h8, raw);
    }
}

// P enters the P.V MFMAs of the prefill kernels as an exact pair of fp16 numbers: hi = p truncated to 11 significant bits (a mask:
// exactly an fp16 number for p >= 2^-14), lo = p - hi (exact in fp32); both packed to fp16 by v_cvt_pkrtz (hi converts exactly, lo
// keeps 11 more bits): 3 VALU ops per probability, 22 significant bits.  With P rounded to fp16 alone the output differed from the
// oracle's by one fp16 ulp on a third of its elements (twice the oracle's own summation-order noise on the HF fixtures,
// tests/test_gpu_model.py).
__device__ __forceinline__ void p_hi_lo(const float (&p)[8], h8& hi, h8& lo) {
    typedef __fp16 pk_h2 __attribute__((ext_vector_type(2)));
    uint32_t hw[4], lw[4];
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) {
        const float p0 = p[2 * q2], p1 = p[2 * q2 + 1];
        const float h0 = __uint_as_float(__float_as_uint(p0) & 0xffffe000u), h1 = __uint_as_float(__float_as_uint(p1) & 0xffffe000u);
        hw[q2] = __builtin_bit_cast(uint32_t, (pk_h2)__builtin_amdgcn_cvt_pkrtz(h0, h1));
        lw[q2] = __builtin_bit_cast(uint32_t, (pk_h2)__builtin_amdgcn_cvt_pkrtz(p0 - h0, p1 - h1));
    }
    hi = __builtin_bit_cast(h8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
    lo = __builtin_bit_cast(h8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
}

// Log-sum-exp merge of n partial softmax rows of D + 2 floats each (unnormalised O[D], maximum m, sum l; natural-log units), `stride`
// floats apart, for channel d: the waves of a decode block, the splits of a split-K / split-KV launch.  The output is o / l.
struct LseRow {
    float o, l, m;
};
__device__ __forceinline__ LseRow lse_merge(const float* rows, int n, int stride, int D, int d) {
    float mm = -1e30f;
    for (int i = 0; i < n; ++i) mm = fmaxf(mm, rows[i * stride + D]);
    float ll = 0.f, o = 0.f;
    for (int i = 0; i < n; ++i) {
        const float a = __expf(rows[i * stride + D] - mm);
        ll = fmaf(rows[i * stride + D + 1], a, ll);
        o = fmaf(rows[i * stride + d], a, o);
    }
    return LseRow{o, ll, mm};
}

}  // namespace pplhip
