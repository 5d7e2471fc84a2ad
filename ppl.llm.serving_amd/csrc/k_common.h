// Device-side helpers shared by the gfx950 kernels (wave64, CDNA4).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "k_tune.h"

namespace pplhip {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int WAVE = 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float h2f(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
// fp32 -> fp16 of a COMPUTED value: the empty asm pins the fp32 value in a register first.  Without it hipcc folds a preceding
// fp32 multiply and the conversion into v_fma_mixlo_f16, which rounds the exact product once to fp16 -- not the same result as
// v_mul_f32 + v_cvt_f16_f32 (fp32 rounding, then fp16 rounding: the oracle's arithmetic) when the fp32 rounding lands on an fp16
// tie -- and it picks either form PER ELEMENT: in the GEMM epilogue 7 of the 8 row groups of a tile got the fused form for two of
// their four columns and the 8th did not, so an output row depended on where its input row sat in the batch
// (profiles/probes/gemm_position_probe*.py; caught by the permutation test of tests/test_gpu_properties.py).
__device__ __forceinline__ _Float16 to_h(float f) {
    asm("" : "+v"(f));
    return (_Float16)f;
}
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, to_h(f)); }
__device__ __forceinline__ float round_h(float f) { return (float)to_h(f); }

// 16-byte vector of 8 halfs <-> floats
// 8 int8 -> 8 fp16, exact: x ^ 0x80 is the biased byte u = x + 128; v_perm puts it under the fp16 exponent 0x64
// (= 1024 + u), minus 1152 gives x.  Two VALU ops per pair.
__device__ __forceinline__ h8 cvt_i8x8_f16(uint2 v) {
    const uint32_t w0 = v.x ^ 0x80808080u, w1 = v.y ^ 0x80808080u;
    const h2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
    const h2 a = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w0, 0x04010400u)) - bias;
    const h2 b = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w0, 0x04030402u)) - bias;
    const h2 c = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w1, 0x04010400u)) - bias;
    const h2 d = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w1, 0x04030402u)) - bias;
    return h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    const h8 h = __builtin_bit_cast(h8, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    h8 h;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = to_h(f[i]);
    return __builtin_bit_cast(uint4, h);
}

// KV cache formats.  The host derives one from (cache_quant_bit, cache_quant_group) once (pplhip.cc kv_format) and the launchers
// take it in place of the quant bit; the two older formats keep their quant bits as values, so their kernel instantiations are unchanged.
//   KV_FP16: fp16 rows, no scales.
//   KV_I8G8: int8 rows, one fp16 scale per 8 channels.
//   KV_FP8 : OCP e4m3fn rows, ONE fp16 scale per head row, a power of two 2^e with e in [-15, 8] (DESIGN.md "numerics"): every
//            dequantised element q * 2^e is exactly an fp16 number, so the fp8 cache is the fp16 cache with every row replaced by Q(row).
//   KV_I4G32: int4 rows, one fp16 scale per 32 channels (a group is one 16-byte piece), D = 32, 64, 128.  Channel 2j of a group is the low
//            nibble of byte j, channel 2j + 1 the high one; a nibble is q + 8 with q in [-7, 7] (the W4A16 convention of k_gemm_dev.h), so
//            0 is never written.  The scale has 8 significant bits (kv_i4_scale): q * s is exactly an fp16 number, and the int4 cache is the
//            fp16 cache with every written group replaced by Q(group) = q * s (DESIGN.md "numerics").
constexpr int KV_FP16 = 0, KV_I8G8 = 8, KV_FP8 = 1, KV_I4G32 = 4;

// fp8 write: exponent e of a row's scale -- the smallest integer with 448 * 2^e >= amax, clamped to [-15, 8] (amax = 0: -15).
// amax = m 2^k (m in [0.5, 1)): 448 = 0.875 2^9, so e = k - 9 when m <= 0.875, else k - 8.  amax is an fp16 value: an fp32 normal or 0.
__device__ __forceinline__ int fp8_row_exp(float amax) {
    const uint32_t u = __builtin_bit_cast(uint32_t, amax);
    const int k = (int)(u >> 23) - 126;
    const int e = k - 9 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
    return u == 0 ? -15 : (e < -15 ? -15 : (e > 8 ? 8 : e));
}
// e4m3fn code of y (|y| <= 448), round to nearest even, fp8 subnormals included (integer rounding: no dependence on the
// conversion instruction's rounding or clamp modes).  Normal range (|y| >= 2^-6): round the fp32 mantissa to 3 bits; below it the
// value is m 2^-9 with m = rne(|y| 2^9) in 0 .. 8 -- and code 8 is 2^-6, the smallest normal, so m is the code as it stands.
__device__ __forceinline__ uint32_t fp8_e4m3_rne(float y) {
    const uint32_t u = __builtin_bit_cast(uint32_t, y);
    const uint32_t sign = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu;
    uint32_t code;
    if (a >= 0x3c800000u) {                      // 2^-6
        a += 0x7ffffu + ((a >> 20) & 1u);
        code = (((a >> 23) - 120u) << 3) | ((a >> 20) & 7u);
    } else {
        code = (uint32_t)rintf(__builtin_bit_cast(float, a) * 512.0f);
    }
    return sign | code;
}
// 2^e as an fp32 (e in [-126, 127]), exact
__device__ __forceinline__ float pow2f(int e) { return __builtin_bit_cast(float, (uint32_t)(127 + e) << 23); }
// e4m3fn code of x in a row of scale exponent e: rne(x 2^-e), saturated to +-448, or +-240 at e = 8 so that q 2^e stays finite in fp16
__device__ __forceinline__ uint32_t fp8_quant(float x, int e) {
    const float lim = e == 8 ? 240.0f : 448.0f;
    return fp8_e4m3_rne(fminf(fmaxf(__fmul_rn(x, pow2f(-e)), -lim), lim));
}
// 16 e4m3fn codes (a 16-byte piece) -> 16 fp32, exact (v_cvt_pk_f32_fp8)
__device__ __forceinline__ void cvt_fp8x16_f32(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
    }
}
// 4 e4m3fn codes (bytes of w) -> 4 fp16 times the power-of-two scale sc, by the hardware conversion with the scale inside (exact:
// every q * 2^e of the format is an fp16 number)
__device__ __forceinline__ h4 cvt_fp8x4_f16(uint32_t w, float sc) {
    const h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, sc, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, sc, true);
    return h4{a[0], a[1], b[0], b[1]};
}
__device__ __forceinline__ h8 cvt_fp8x8_f16(uint2 v, float sc) {
    const h4 a = cvt_fp8x4_f16(v.x, sc), b = cvt_fp8x4_f16(v.y, sc);
    return h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// int4 write: scale of a group whose max|x| is amax (an fp16 value) -- amax / 7 (one correctly rounded division) rounded UP to 8
// significant bits, clamped to [2^-14, 9344]: exactly an fp16 number whose low three mantissa bits are zero, 7 s <= 65408 is finite and
// every q s (|q| <= 7) is a normal fp16 number or 0
__device__ __forceinline__ float kv_i4_scale(float amax) {
    uint32_t u = __builtin_bit_cast(uint32_t, __fdiv_rn(amax, 7.0f));
    u = (u + 0xffffu) & ~0xffffu;
    return fminf(fmaxf(__builtin_bit_cast(float, u), 6.103515625e-05f), 9344.0f);
}
// nibble (q + 8, in 1..15) of x under the reciprocal inv = 1 / s (one correctly rounded division per group: the int8 writer's rule)
__device__ __forceinline__ uint32_t kv_i4_quant(float x, float inv) {
    const float q = fminf(fmaxf(rintf(__fmul_rn(x, inv)), -7.f), 7.f);
    return (uint32_t)((int)q + 8);
}
// 8 channels' nibbles -> one 32-bit word, channel i at bits 4 i
__device__ __forceinline__ uint32_t kv_i4_pack8(const float* x, float inv) {
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) w |= kv_i4_quant(x[i], inv) << (4 * i);
    return w;
}
// the 8 nibbles of a word -> 8 fp16 q = nibble - 8 in channel order, exact: the nibbles become the bytes n0 .. n3 | n4 .. n7 (v_perm),
// each goes under the fp16 exponent 0x64 (= 1024 + n), minus 1032
__device__ __forceinline__ h8 cvt_i4x8_f16(uint32_t w) {
    const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;   // even / odd channels
    const uint32_t b0 = __builtin_amdgcn_perm(hi, lo, 0x05010400u), b1 = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
    const h2 bias = {(_Float16)1032.0f, (_Float16)1032.0f};
    const h2 a = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, b0, 0x04010400u)) - bias;
    const h2 b = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, b0, 0x04030402u)) - bias;
    const h2 c = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, b1, 0x04010400u)) - bias;
    const h2 d = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, b1, 0x04030402u)) - bias;
    return h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// ... times the group's scale in packed fp16: exact (a 3-bit by 8-bit product), no rounding
__device__ __forceinline__ h8 cvt_i4x8_f16(uint32_t w, _Float16 s) { return cvt_i4x8_f16(w) * s; }

// Decode attention reads every K/V row exactly once per step: non-temporal loads (compile-time switch PPLHIP_KV_NT) stream them
// past the caches instead of through them -- measured +5..9 % (batch 1024 kv 512: 5.92 -> 6.23 TB/s, kv 1024: 6.24 -> 6.70 TB/s,
// profiles/attn_microbench.py; MI355X_MICROARCH.md quotes 6.4 TB/s default policy vs 6.5-6.8 nt for a streaming read)
#ifndef PPLHIP_KV_NT
#define PPLHIP_KV_NT 1
#endif
typedef uint32_t kv_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 kv_stream_load(const uint4* p) {
#if PPLHIP_KV_NT
    return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const kv_u32x4*>(p)));
#else
    return *p;
#endif
}
__device__ __forceinline__ uint32_t kv_stream_load(const uint32_t* p) {
#if PPLHIP_KV_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// KV slab addressing (src/engine/llm_engine.cc:118-169): element strides of (layer, k/v, head, token)
// for the four cache layouts; `d` is the innermost extent (head_dim, or head_dim/group for scales).
struct KvStrides {
    int64_t sL, sKV, sH, sN;
};
__host__ __device__ inline KvStrides kv_strides(int layout, int64_t N, int64_t L, int64_t h, int64_t d) {
    KvStrides s;
    switch (layout) {
        case 0: s.sN = L * 2 * h * d; s.sL = 2 * h * d; s.sKV = h * d; s.sH = d; break;
        case 1: s.sL = N * 2 * h * d; s.sN = 2 * h * d; s.sKV = h * d; s.sH = d; break;
        case 2: s.sL = 2 * N * h * d; s.sKV = N * h * d; s.sN = h * d; s.sH = d; break;
        default: s.sL = 2 * h * N * d; s.sKV = h * N * d; s.sH = N * d; s.sN = d; break;
    }
    return s;
}

// everything an attention / cache-write kernel needs to find K/V rows of one layer
struct KvAddr {
    void* cache;        // fp16 or int8 base of this LAYER's K plane (kv = 0); V plane = + sKV
    uint16_t* scale;    // fp16 scales, same convention
    int64_t sKV, sH, sN;       // element strides in the cache
    int64_t ssKV, ssH, ssN;    // element strides in the scale slab
    int32_t mode, page_size;   // cache_mode (0 contiguous / 1 paged)
    int32_t page_shift;        // log2(page_size) when it is a power of two (the usual 16), else -1: a 64-bit division per KV row is ~50 VALU ops
};

// KV slot of (request b, position pos): mode 0 cache_indices[b] + pos; mode 1 paged
// (src/generator/llm_generator.cc:487,553-554; llm_engine.cc:64-71)
__device__ __forceinline__ int64_t kv_slot(const KvAddr& a, const int64_t* __restrict__ cache_indices, int64_t max_pages,
                                           int64_t b, int64_t pos) {
    if (a.mode == 0) return cache_indices[b] + pos;
    if (a.page_shift >= 0) {
        const int64_t pg = pos >> a.page_shift;
        return (cache_indices[b * max_pages + pg] << a.page_shift) + (pos & (int64_t)(a.page_size - 1));
    }
    const int64_t pg = pos / a.page_size;
    return cache_indices[b * max_pages + pg] * a.page_size + (pos - pg * a.page_size);
}

}  // namespace pplhip
