// What the RoPE + KV-write kernels (k_rope_kv.hip, k_rope_prologue.hip) share: the stores of 8 channels into the KV slab in each cache
// format, and the cross-lane maximum their item groups meet in.
#pragma once
#include "kernels.h"

namespace pplhip {

template <int QBIT>
__device__ __forceinline__ void store_group8(const KvAddr& kv, int kvsel, int head, int64_t slot, int ch0,
                                             const float* x /*8*/) {
    const int64_t base = (int64_t)kvsel * kv.sKV + (int64_t)head * kv.sH + slot * kv.sN + ch0;
    if constexpr (QBIT == 0) {
        *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(kv.cache) + base) = pack8(x);
    } else {
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(x[i]));
        const _Float16 sh = to_h(mx / 127.0f);
        const float sf = (float)sh;
        const float inv = sf > 0.f ? __fdiv_rn(1.0f, sf) : 0.f;  // one correctly rounded reciprocal per group
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float q = rintf(__fmul_rn(x[i], inv));
            q = fminf(fmaxf(q, -127.f), 127.f);
            const uint32_t b = (uint32_t)(int)q & 0xffu;
            if (i < 4) lo |= b << (8 * i); else hi |= b << (8 * (i - 4));
        }
        *reinterpret_cast<uint2*>(reinterpret_cast<int8_t*>(kv.cache) + base) = make_uint2(lo, hi);
        const int64_t sbase = (int64_t)kvsel * kv.ssKV + (int64_t)head * kv.ssH + slot * kv.ssN + ch0 / 8;
        kv.scale[sbase] = __builtin_bit_cast(uint16_t, sh);
    }
}

// KV_FP8: 8 channels of a head row whose scale exponent is e (fp8_row_exp of the row's max|x|): codes e4m3fn(x 2^-e), saturated to
// +-240 at e = 8 so that q 2^e stays finite in fp16; the item of channel 0 stores the row's scale fp16(2^e)
__device__ __forceinline__ void store_fp8_row8(const KvAddr& kv, int kvsel, int head, int64_t slot, int ch0, const float* x /*8*/,
                                               int e) {
    const int64_t base = (int64_t)kvsel * kv.sKV + (int64_t)head * kv.sH + slot * kv.sN + ch0;
    const float inv = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);   // 2^-e, exact
    const float lim = e == 8 ? 240.0f : 448.0f;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float y = __fmul_rn(x[i], inv);
        const uint32_t b = fp8_e4m3_rne(fminf(fmaxf(y, -lim), lim));
        if (i < 4) lo |= b << (8 * i); else hi |= b << (8 * (i - 4));
    }
    *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(kv.cache) + base) = make_uint2(lo, hi);
    if (ch0 == 0) kv.scale[(int64_t)kvsel * kv.ssKV + (int64_t)head * kv.ssH + slot * kv.ssN] = f2h(__builtin_bit_cast(float, (uint32_t)(127 + e) << 23));
}
// KV_I4G32: 8 channels of a group whose max|x| is amax: nibbles q + 8, q = clamp(rint(x / s), +-7), s = kv_i4_scale(amax); the item of the
// group's first channel stores s
__device__ __forceinline__ void store_i4_group8(const KvAddr& kv, int kvsel, int head, int64_t slot, int ch0, const float* x /*8*/, float amax) {
    const float sf = kv_i4_scale(amax);
    const float inv = __fdiv_rn(1.0f, sf);   // one correctly rounded reciprocal per group
    const int64_t base = (int64_t)kvsel * kv.sKV + (int64_t)head * kv.sH + slot * kv.sN + ch0 / 2;   // a row of D / 2 one-byte elements
    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(kv.cache) + base) = kv_i4_pack8(x, inv);
    if ((ch0 & 31) == 0) kv.scale[(int64_t)kvsel * kv.ssKV + (int64_t)head * kv.ssH + slot * kv.ssN + ch0 / 32] = f2h(sf);
}
// max over the n lanes (a power of two, aligned) of an item group
__device__ __forceinline__ float group_max(float v, int n) {
    for (int o = 1; o < n; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

}  // namespace pplhip
