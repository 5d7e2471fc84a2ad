// online_i8i8 (W8A8) linear layers: the quant method src/backends/cuda/resource_manager.cc:51-52 hands to ppl.nn.
//   activations  per token row:   sx = max|x| / 127 (fp32), q = clamp(rint(x * (127 / max|x|)))           quant_act_kernel
//   weights      per output row:  scale = fp16(max|w| / 127), q = clamp(rint(w / scale))   (once, at load) quant_weight_kernel
//   y[m,n] = fp16( (float)(sum_k qx * qw) * sx[m] * scale[n] ),  the sum exact in int32 on the matrix cores
// Oracle: linear_fwd_a8 / ref_quant_act_rows / ref_quant_weight_rows (oracle/llama_ref.c) -- integer accumulation makes
// the GEMM itself bit-exact against it; only the fp16 rounding of the two fp32 multiplies is left, done in the same order.
//
// Tile kernel (M > 32, K % 128 == 0): block tile 128 (n) x 128 (m) x 128 (k) int8, 4 multiplying waves as 2 x 2, each 64 x 64 =
// 4 x 4 tiles of v_mfma_i32_16x16x64_i8 (weights = A operand, so a lane owns 4 consecutive n of one activation row), and 4 producer
// waves that only move the tiles (gemm_i8_pc_kernel).  Both operands go global -> LDS by DMA into [row][128 B] tiles whose 16-byte
// chunk index is XOR-swizzled with (row >> 1) & 7 on the source address and on the fragment reads (same scheme as the fp16 activation
// tile of k_gemm_dev.h).  A ring of 2 LDS stages (64 KiB -> two blocks per CU) or, for launches of <= 256 tiles, 4; one barrier per
// K tile.  The 128 x 384 blocks (gemm_i8_wide_kernel) share its consumer step (mma_tile), block order (xcd_tile) and DMA source layout
// (dma_src128); they and the 256 x 256 blocks (gemm_i8_256_kernel; int8, M >= 4096) share its epilogue (store_wave_tile).
// Skinny / generic kernel (any M, K % 16 == 0): one block per 16 weight rows, waves split K, weights straight from HBM
// into the MFMA A operand, activations (L2 resident) into B; grid.y walks 32-row activation groups.
//
// online_f8f8 (fp8 e4m3fn W8A8) runs on the same kernels (template flag F8): per row, the fp8 KV row rule (k_common.h) gives
// q = e4m3fn_rne(x 2^-e) with one power-of-two scale 2^e per token (sx, fp32) and per output row (scale, fp16)   quant_*_f8_kernel
//   y[m,n] = fp16( (sum_k qx * qw) * 2^ex[m] * 2^ew[n] ),  fp32 sums of exact products on v_mfma_scale_f32_16x16x128_f8f6f4
// A 128-deep K tile of 128-byte LDS rows feeds ONE fp8 MFMA per 16 x 16 tile where it feeds two int8 ones; ring, swizzle, tile
// shapes and epilogues are shared.  No 256 x 256 form: fp8 steps of M >= 4096 run the 128 x 128 producer / consumer form.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "k_gemm_dev.h"

namespace pplhip {

typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));
// accumulator of a 16 x 16 tile: exact int32 sums (int8) or fp32 (fp8 -- exact as well for operands whose sums stay below 2^24)
template <bool F8> using qacc_t = std::conditional_t<F8, f4v, i4v>;

// (the tile sizes I_BN / I_BM / I_BK and IW_* are in k_gemm_tiles.h: the launch plan sizes its grids from them)

__device__ __forceinline__ float block_max_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ int q8(float v) {
    v = rintf(v);
    v = fminf(fmaxf(v, -127.f), 127.f);
    return (int)v;
}

// The quantisers: one block per row.  int8 (F8 false): activations q = clamp(rint(x * (127 / max|x|))), sx = max|x| / 127; weights
// scale = fp16(max|w| / 127), q = clamp(rint(w / scale)).  online_f8f8 (F8 true): the fp8 KV row rule (k_common.h fp8_row_exp /
// fp8_quant) -- e = the smallest integer with 448 2^e >= max|x| (clamped to [-15, 8]), q = e4m3fn_rne(x 2^-e), sx = 2^e (fp32),
// scale = fp16(2^e).  Only the per-element rule and the scale write differ between the two.
// x [M, ldx] fp16 (K valid) -> q [M, ldq] codes (columns K..ldq-1 zero) + sx [M]
template <bool F8>
__device__ __forceinline__ void quant_act_row(const uint16_t* __restrict__ x, int K, int64_t ldx, uint8_t* __restrict__ q, int64_t ldq,
                                              float* __restrict__ sx) {
    __shared__ float red[4];
    const int64_t m = blockIdx.x;
    const uint16_t* xr = x + m * ldx;
    uint8_t* qr = q + m * ldq;
    const int K8 = K >> 3;
    float amax = 0.f;
    for (int i = threadIdx.x; i < K8; i += 256) {
        const h8 v = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(xr + i * 8));
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)v[j]));
    }
    for (int k = K8 * 8 + threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(h2f(xr[k])));
    amax = block_max_256(amax, red);
    const int e = F8 ? fp8_row_exp(amax) : 0;
    const float inv = amax > 0.f ? 127.0f / amax : 0.f;
    if (threadIdx.x == 0) sx[m] = F8 ? pow2f(e) : amax / 127.0f;
    auto code = [&](float v) -> uint32_t { return F8 ? fp8_quant(v, e) : (uint32_t)(q8(v * inv) & 0xff); };
    for (int i = threadIdx.x; i < K8; i += 256) {
        const h8 v = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(xr + i * 8));
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) lo |= code((float)v[j]) << (8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) hi |= code((float)v[4 + j]) << (8 * j);
        *reinterpret_cast<uint2*>(qr + i * 8) = make_uint2(lo, hi);
    }
    for (int k = K8 * 8 + threadIdx.x; k < K; k += 256) qr[k] = (uint8_t)code(h2f(xr[k]));
    for (int64_t k = K + threadIdx.x; k < ldq; k += 256) qr[k] = 0;
}
// w [N, K] fp16 -> q [N, ldq] codes (pad columns zero) + scale [N] fp16
template <bool F8>
__device__ __forceinline__ void quant_weight_row(const uint16_t* __restrict__ w, int K, uint8_t* __restrict__ q, int64_t ldq,
                                                 uint16_t* __restrict__ scale) {
    __shared__ float red[4];
    const int64_t n = blockIdx.x;
    const uint16_t* wr = w + n * K;
    uint8_t* qr = q + n * ldq;
    float amax = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(h2f(wr[k])));
    amax = block_max_256(amax, red);
    const int e = F8 ? fp8_row_exp(amax) : 0;
    const uint16_t sh = F8 ? f2h(pow2f(e)) : f2h(amax / 127.0f);
    if (threadIdx.x == 0) scale[n] = sh;
    const float s = h2f(sh) > 0.f ? h2f(sh) : 1.0f;
    for (int k = threadIdx.x; k < K; k += 256)  // int8: IEEE division (hipcc default: correctly rounded)
        qr[k] = F8 ? (uint8_t)fp8_quant(h2f(wr[k]), e) : (uint8_t)q8(h2f(wr[k]) / s);
    for (int64_t k = K + threadIdx.x; k < ldq; k += 256) qr[k] = 0;
}
__global__ __launch_bounds__(256) void quant_act_kernel(const uint16_t* __restrict__ x, int K, int64_t ldx, int8_t* __restrict__ q,
                                                        int64_t ldq, float* __restrict__ sx) {
    quant_act_row<false>(x, K, ldx, reinterpret_cast<uint8_t*>(q), ldq, sx);
}
__global__ __launch_bounds__(256) void quant_act_f8_kernel(const uint16_t* __restrict__ x, int K, int64_t ldx, uint8_t* __restrict__ q,
                                                           int64_t ldq, float* __restrict__ sx) {
    quant_act_row<true>(x, K, ldx, q, ldq, sx);
}
__global__ __launch_bounds__(256) void quant_weight_kernel(const uint16_t* __restrict__ w, int K, int8_t* __restrict__ q, int64_t ldq,
                                                           uint16_t* __restrict__ scale) {
    quant_weight_row<false>(w, K, reinterpret_cast<uint8_t*>(q), ldq, scale);
}
__global__ __launch_bounds__(256) void quant_weight_f8_kernel(const uint16_t* __restrict__ w, int K, uint8_t* __restrict__ q, int64_t ldq,
                                                              uint16_t* __restrict__ scale) {
    quant_weight_row<true>(w, K, q, ldq, scale);
}

template <int EPI>
__device__ __forceinline__ void store4_i8(void* yv, int64_t ldy, int64_t m, int n, i4v acc, float sxm, h4 sh) {
    store4<EPI>(yv, ldy, m, n, ((float)acc[0] * sxm) * (float)sh[0], ((float)acc[1] * sxm) * (float)sh[1],
                ((float)acc[2] * sxm) * (float)sh[2], ((float)acc[3] * sxm) * (float)sh[3]);
}
// fp8: sxm = 2^ex and sh = 2^ew, so both products are exact -- y = fp16(2^(ex + ew) * acc)
template <int EPI>
__device__ __forceinline__ void store4_i8(void* yv, int64_t ldy, int64_t m, int n, f4v acc, float sxm, h4 sh) {
    store4<EPI>(yv, ldy, m, n, (acc[0] * sxm) * (float)sh[0], (acc[1] * sxm) * (float)sh[1], (acc[2] * sxm) * (float)sh[2],
                (acc[3] * sxm) * (float)sh[3]);
}

// one 16 x 16 x 128 fp8 product on the scaled MFMA with unit E8M0 scales (127 = 2^0; the power-of-two scales go on in the epilogue).
// lo / hi: the 16-byte k chunks the int8 form feeds its two 16x16x64 MFMAs with (chunks kq and 4 + kq of the 128-deep tile).  Both
// operands carry the same k permutation, so the sum is the sum over the tile's 128 k.
__device__ __forceinline__ f4v mma_f8(i4v alo, i4v ahi, i4v blo, i4v bhi, f4v c) {
    const i8v a = __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7), b = __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}
// Consumer step of a 128-deep LDS tile pair ([row][128 B], g_swz chunks) for a 64 x 64 wave tile, weight rows wr0.., activation rows
// xr0..: the fragments of 16-byte chunk c = ks * 4 + kq (k-step ks), then int8 two rounds of 16 MFMAs, fp8 one round on both k-steps
__device__ __forceinline__ void tile_frags(const char* ws, const char* xs, int wr0, int xr0, int l15, int c, i4v (&a)[4], i4v (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wr0 + i * 16 + l15;
        a[i] = *reinterpret_cast<const i4v*>(ws + row * I_BK + g_swz(row, c) * 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = xr0 + j * 16 + l15;
        b[j] = *reinterpret_cast<const i4v*>(xs + row * I_BK + g_swz(row, c) * 16);
    }
}
__device__ __forceinline__ void mma_tile(const char* ws, const char* xs, int wr0, int xr0, int l15, int kq, i4v (&acc)[4][4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        i4v a[4], b[4];
        tile_frags(ws, xs, wr0, xr0, l15, ks * 4 + kq, a, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}
__device__ __forceinline__ void mma_tile(const char* ws, const char* xs, int wr0, int xr0, int l15, int kq, f4v (&acc)[4][4]) {
    i4v a[2][4], b[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) tile_frags(ws, xs, wr0, xr0, l15, ks * 4 + kq, a[ks], b[ks]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mma_f8(a[0][i], a[1][i], b[0][j], b[1][j], acc[i][j]);
}

// epilogue of a wave tile of 4 (n) x NJ (m) 16 x 16 tiles whose first output is y[m0][n0]
template <int EPI, class ACC, int NJ>
__device__ __forceinline__ void store_wave_tile(void* yv, int64_t ldy, const float* __restrict__ sx, const uint16_t* __restrict__ scale,
                                                int64_t M, int N, int64_t m0, int n0, int l15, int kq, const ACC (&acc)[4][NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t m = m0 + j * 16 + l15;
        if (m >= M) continue;
        const float sxm = sx[m];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + i * 16 + kq * 4;
            if (n >= N) continue;
            const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + n));
            store4_i8<EPI>(yv, ldy, m, n, acc[i][j], sxm, sh);
        }
    }
}

// LDS-DMA source of lane position p (16-byte chunk p & 7 of tile row p >> 3) of a [rows][128 B] tile that starts at row row0 of the
// matrix base [nrows][K]: rows past the matrix repeat its last row (never stored), the chunk is XOR-swizzled on the source side (the
// DMA writes LDS linearly)
template <class I>
__device__ __forceinline__ const int8_t* dma_src128(const int8_t* base, I row0, I nrows, int K, int p) {
    const int row = p >> 3, c = (p & 7) ^ ((row >> 1) & 7);
    I r = row0 + row;
    if (r >= nrows) r = nrows - 1;
    return base + (int64_t)r * K + c * 16;
}

// The tile kernel, a producer / consumer block of 8 waves: waves 0..3 multiply (2 x 2, each 64 x 64), waves 4..7 do nothing but wait
// for their LDS-DMA pieces and refill the ring (the ~100-cycle issue cost of a piece then runs beside the MFMA stream instead of in
// front of it: int8 moves 8 pieces per 32 MFMAs and wave, more than the fp16 kernel).  ST stages of 32 KiB, one barrier per tile.
template <int EPI, int ST, bool F8>
__global__ __launch_bounds__(512) void gemm_i8_pc_kernel(const int8_t* __restrict__ xq, const float* __restrict__ sx,
                                                         const int8_t* __restrict__ w, const uint16_t* __restrict__ scale, int64_t M,
                                                         int N, int K, void* __restrict__ yv, int64_t ldy, int n_tiles, int m_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem_i8[];  // ST x (X 16 KiB) then ST x (W 16 KiB)
    constexpr int TILE = I_BM * I_BK;
    int nt, mt;
    xcd_tile((int)blockIdx.x, m_tiles, nt, mt);
    if (nt >= n_tiles) return;
    const int n0 = nt * I_BN;
    const int64_t m0 = (int64_t)mt * I_BM;
    const bool producer = threadIdx.x >= 256;
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int ktiles = K / I_BK;
    constexpr int D = ST - 1, PT = 8;  // pieces per producer wave and tile

    if (producer) {
        const int8_t* xsrc[4];
        const int8_t* wsrc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xsrc[j] = dma_src128(xq, m0, M, K, j * 256 + tid);
            wsrc[j] = dma_src128(w, n0, N, K, j * 256 + tid);
        }
        const uint32_t xdst = __builtin_amdgcn_readfirstlane(lds_addr(smem_i8) + wave * 1024);
        const uint32_t wdst = xdst + ST * TILE;
        auto issue = [&](int stage, int k0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) glds16(xsrc[j] + k0, xdst + stage * TILE + j * 4096);
#pragma unroll
            for (int j = 0; j < 4; ++j) glds16(wsrc[j] + k0, wdst + stage * TILE + j * 4096);
        };
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d < ktiles) issue(d, d * I_BK);
        int stn = D % ST;
        for (int t = 0; t < ktiles; ++t) {
            ring_wait<PT>((ktiles - 1 - t) < (D - 1) ? (ktiles - 1 - t) : (D - 1));
            __syncthreads();
            if (t + D < ktiles) issue(stn, (t + D) * I_BK);
            stn = stn == ST - 1 ? 0 : stn + 1;
        }
        return;
    }

    const int wn = wave & 1, wm = wave >> 1;
    qacc_t<F8> acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = qacc_t<F8>{0, 0, 0, 0};
    int st = 0;
    for (int t = 0; t < ktiles; ++t) {
        __syncthreads();
        const char* xs = smem_i8 + st * TILE;
        const char* ws = smem_i8 + ST * TILE + st * TILE;
        st = st == ST - 1 ? 0 : st + 1;
        mma_tile(ws, xs, wn * 64, wm * 64, l15, kq, acc);
    }
    store_wave_tile<EPI>(yv, ldy, sx, scale, M, N, m0 + wm * 64, n0 + wn * 64, l15, kq, acc);
}

// 128 (m) x 384 (n) x 128 (k) block: the int8 form of gemm_w8_wide_kernel (k_gemm_wide.hip).  Twelve consumer waves as 6 (n) x 2 (m), wave
// tile 64 x 64 like the waves of the kernel above, share ONE activation tile; four producer waves keep a two-stage ring of 64 KiB filled.
// Two co-resident 128 x 128 blocks move 64 KiB per 1024 MFMA cycles and CU -- the whole 64 B / clk of the CU's vector-memory path --, this
// block moves 64 KiB per 3072 (profiles/r03_gemm_experiments.md #16-17).  Taken when its tiles fill rounds of 256 one-per-CU blocks.
constexpr int IW_PP = (IW_XB + IW_WB) / 1024 / IW_NP;           // 16 one-KiB pieces per producer wave and tile (4 activation + 12 weight)
template <int EPI, bool F8>
__global__ __launch_bounds__((IW_NC + IW_NP) * 64) void gemm_i8_wide_kernel(const int8_t* __restrict__ xq, const float* __restrict__ sx,
                                                                             const int8_t* __restrict__ w, const uint16_t* __restrict__ scale,
                                                                             int64_t M, int N, int K, void* __restrict__ yv, int64_t ldy,
                                                                             int n_tiles, int m_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem_i8[];  // IW_ST x (X 16 KiB) then IW_ST x (W 48 KiB)
    int nt, mt;
    xcd_tile((int)blockIdx.x, m_tiles, nt, mt);
    if (nt >= n_tiles) return;
    const int n0 = nt * IW_BN;
    const int64_t m0 = (int64_t)mt * I_BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ktiles = K / I_BK;

    if (wave >= IW_NC) {
        // producer pw: pieces P = pw + 4 j; j < 4: activation piece P (rows 8 P .. + 8), else weight piece P - 16 (rows 8 (P - 16) .. + 8);
        // 128-byte rows, 16-byte chunks XOR-swizzled with (row >> 1) & 7 on the SOURCE side (the DMA writes LDS linearly)
        const int pw = wave - IW_NC;
        const int8_t* psrc[IW_PP];
        uint32_t pdst[IW_PP];
        const uint32_t xbase = lds_addr(smem_i8), wbase = xbase + IW_ST * IW_XB;
#pragma unroll
        for (int j = 0; j < IW_PP; ++j) {
            const int P = pw + IW_NP * j;
            const bool isx = j < IW_XB / 1024 / IW_NP;
            const int Pl = isx ? P : P - IW_XB / 1024;
            psrc[j] = isx ? dma_src128(xq, m0, M, K, Pl * 64 + lane) : dma_src128(w, n0, N, K, Pl * 64 + lane);
            pdst[j] = __builtin_amdgcn_readfirstlane((isx ? xbase : wbase) + Pl * 1024);
        }
        auto produce = [&](int kt, int stage) {
#pragma unroll
            for (int j = 0; j < IW_PP; ++j) glds16(psrc[j] + (int64_t)kt * I_BK, pdst[j] + stage * (j < IW_XB / 1024 / IW_NP ? IW_XB : IW_WB));
        };
        produce(0, 0);
        for (int t = 0; t < ktiles; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // tile t is published; the other stage (read during iteration t - 1) is free
            if (t + 1 < ktiles) produce(t + 1, (t + 1) & 1);
        }
        return;
    }

    const int l15 = lane & 15, kq = lane >> 4;
    const int wn = wave % 6, wm = wave / 6;
    qacc_t<F8> acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = qacc_t<F8>{0, 0, 0, 0};
    for (int t = 0; t < ktiles; ++t) {
        __syncthreads();
        const char* xs = smem_i8 + (t & 1) * IW_XB;
        const char* ws = smem_i8 + IW_ST * IW_XB + (t & 1) * IW_WB;
        mma_tile(ws, xs, wn * 64, wm * 64, l15, kq, acc);
    }
    store_wave_tile<EPI>(yv, ldy, sx, scale, M, N, m0 + wm * 64, n0 + wn * 64, l15, kq, acc);
}

// Large M (steps that carry prefill): 256(n) x 256(m) x 64(k) tiles, 8 waves as 4 (n) x 2 (m), wave tile 64 x 128 = 4 x 8 MFMA tiles
// (12 fragment reads and 4 LDS-DMA pieces per 32 MFMAs and wave, against 16 and 8 in the 128 x 128 kernels), 64-byte rows with the
// w_swz chunk swizzle for both operands, ST-stage ring of 32 KiB, one barrier per tile, one block per CU.
template <int EPI, int ST>
__global__ __launch_bounds__(512) void gemm_i8_256_kernel(const int8_t* __restrict__ xq, const float* __restrict__ sx,
                                                          const int8_t* __restrict__ w, const uint16_t* __restrict__ scale, int64_t M,
                                                          int N, int K, void* __restrict__ yv, int64_t ldy, int n_tiles, int m_tiles,
                                                          int gn, int gm) {
    extern __shared__ __attribute__((aligned(16))) char smem_i8[];  // ST x (X 16 KiB) then ST x (W 16 KiB)
    constexpr int TILE = 256 * 64;
    // XCD id % 8 walks its weight tiles in super-tiles of gn (n) x gm (m) tiles (xcd_super_tile): the blocks it runs at a time share gn
    // weight and gm activation tiles per K step
    int nt, mt;
    xcd_super_tile((int)blockIdx.x, m_tiles, gn, gm, nt, mt);
    if (nt >= n_tiles) return;
    const int n0 = nt * 256;
    const int64_t m0 = (int64_t)mt * 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int wn = wave & 3, wm = wave >> 2;

    const int8_t* xsrc[2];
    const int8_t* wsrc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = j * 512 + tid, row = p >> 2, c = (p & 3) ^ w_swz(row);
        int64_t m = m0 + row;
        if (m >= M) m = M - 1;
        int n = n0 + row;
        if (n >= N) n = N - 1;
        xsrc[j] = xq + m * K + c * 16;
        wsrc[j] = w + (int64_t)n * K + c * 16;
    }
    const uint32_t xdst = __builtin_amdgcn_readfirstlane(lds_addr(smem_i8) + wave * 1024);
    const uint32_t wdst = xdst + ST * TILE;
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(xsrc[j] + k0, xdst + stage * TILE + j * 8192);
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(wsrc[j] + k0, wdst + stage * TILE + j * 8192);
    };
    int woff[4], xoff[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wn * 64 + i * 16 + l15;
        woff[i] = ST * TILE + row * 64 + (kq ^ w_swz(row)) * 16;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = wm * 128 + j * 16 + l15;
        xoff[j] = row * 64 + (kq ^ w_swz(row)) * 16;
    }
    i4v acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = i4v{0, 0, 0, 0};

    constexpr int D = ST - 1, PT = 4;
    const int ktiles = K / 64;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < ktiles) issue(d, d * 64);
    int st = 0, stn = D % ST;
    for (int t = 0; t < ktiles; ++t) {
        ring_wait<PT>((ktiles - 1 - t) < (D - 1) ? (ktiles - 1 - t) : (D - 1));
        __syncthreads();
        if (t + D < ktiles) issue(stn, (t + D) * 64);
        const char* sb = smem_i8 + st * TILE;
        st = st == ST - 1 ? 0 : st + 1;
        stn = stn == ST - 1 ? 0 : stn + 1;
        i4v a[4], b[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const i4v*>(sb + woff[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = *reinterpret_cast<const i4v*>(sb + xoff[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    store_wave_tile<EPI>(yv, ldy, sx, scale, M, N, m0 + wm * 128, n0 + wn * 64, l15, kq, acc);
}

// skinny / generic: block = NW waves = NW K slices of 16 weight rows; MT = 16-row activation tiles per block (grid.y walks M)
// fp8 (F8): one scaled 16x16x128 MFMA per two wave-loads (their 16-byte pieces as the lo / hi halves of both operands, mma_f8)
template <int MT, int EPI, int NW, bool F8>
__global__ __launch_bounds__(NW * 64) void gemv_i8_kernel(const int8_t* __restrict__ xq, const float* __restrict__ sx,
                                                          const int8_t* __restrict__ w, const uint16_t* __restrict__ scale, int64_t M, int N,
                                                          int K, void* __restrict__ yv, int64_t ldy) {
    __shared__ __attribute__((aligned(16))) int red[NW - 1][MT][64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int64_t mbase = (int64_t)blockIdx.y * (MT * 16);
    int n = n0 + l15;
    if (n >= N) n = N - 1;
    const int steps = (K + 63) / 64;  // one wave-load = 16 rows x 64 bytes
    const int per = (steps + NW - 1) / NW;
    const int s_begin = wave * per, s_end = (s_begin + per < steps) ? s_begin + per : steps;
    const int8_t* wrow = w + (int64_t)n * K;
    const int8_t* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int64_t m = mbase + mt * 16 + l15;
        if (m >= M) m = M - 1;
        xrow[mt] = xq + m * K;
    }
    qacc_t<F8> acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = qacc_t<F8>{0, 0, 0, 0};
    constexpr int U = 8;  // wave-loads of weights in flight (the block streams its rows once: bytes in flight = bandwidth)
    for (int st0 = s_begin; st0 < s_end; st0 += U) {
        i4v wr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = (st0 + u) * 64 + kq * 16;
            const bool ok = st0 + u < s_end && k < K;  // K % 16 == 0 (launcher)
            wr[u] = ok ? *reinterpret_cast<const i4v*>(wrow + k) : i4v{0, 0, 0, 0};
        }
        if constexpr (F8) {
#pragma unroll
            for (int u = 0; u < U; u += 2) {
                const int k = (st0 + u) * 64 + kq * 16;
                const bool ok0 = st0 + u < s_end && k < K, ok1 = st0 + u + 1 < s_end && k + 64 < K;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const i4v x0 = ok0 ? *reinterpret_cast<const i4v*>(xrow[mt] + k) : i4v{0, 0, 0, 0};
                    const i4v x1 = ok1 ? *reinterpret_cast<const i4v*>(xrow[mt] + k + 64) : i4v{0, 0, 0, 0};
                    acc[mt] = mma_f8(wr[u], wr[u + 1], x0, x1, acc[mt]);
                }
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = (st0 + u) * 64 + kq * 16;
            const bool ok = st0 + u < s_end && k < K;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const i4v xr = ok ? *reinterpret_cast<const i4v*>(xrow[mt] + k) : i4v{0, 0, 0, 0};
                acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wr[u], xr, acc[mt], 0, 0, 0);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<qacc_t<F8>*>(red[wave - 1][mt][lane]) = acc[mt];
    }
    __syncthreads();
    if (wave == 0) {
        const int nn = n0 + kq * 4;
        if (nn < N) {
            const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + nn));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                qacc_t<F8> v = acc[mt];
#pragma unroll
                for (int ww = 0; ww < NW - 1; ++ww) v += *reinterpret_cast<const qacc_t<F8>*>(red[ww][mt][lane]);
                const int64_t m = mbase + mt * 16 + l15;
                if (m >= M) continue;
                store4_i8<EPI>(yv, ldy, m, nn, v, sx[m], sh);
            }
        }
    }
}

hipError_t launch_quant_act(hipStream_t s, const uint16_t* x, int64_t M, int K, int64_t ldx, int8_t* q, int64_t ldq, float* sx) {
    if (M == 0) return hipSuccess;
    if (K % 8 || ldx % 8 || ldq % 8 || ldq < K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quant_act_kernel, dim3((unsigned)M), dim3(256), 0, s, x, K, ldx, q, ldq, sx);
    return hipGetLastError();
}

hipError_t launch_quant_weight(hipStream_t s, const uint16_t* w, int N, int K, int8_t* q, int64_t ldq, uint16_t* scale) {
    if (N == 0) return hipSuccess;
    if (ldq < K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quant_weight_kernel, dim3((unsigned)N), dim3(256), 0, s, w, K, q, ldq, scale);
    return hipGetLastError();
}

hipError_t launch_quant_act_f8(hipStream_t s, const uint16_t* x, int64_t M, int K, int64_t ldx, uint8_t* q, int64_t ldq, float* sx) {
    if (M == 0) return hipSuccess;
    if (K % 8 || ldx % 8 || ldq % 8 || ldq < K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quant_act_f8_kernel, dim3((unsigned)M), dim3(256), 0, s, x, K, ldx, q, ldq, sx);
    return hipGetLastError();
}

hipError_t launch_quant_weight_f8(hipStream_t s, const uint16_t* w, int N, int K, uint8_t* q, int64_t ldq, uint16_t* scale) {
    if (N == 0) return hipSuccess;
    if (ldq < K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quant_weight_f8_kernel, dim3((unsigned)N), dim3(256), 0, s, w, K, q, ldq, scale);
    return hipGetLastError();
}

// launch_linear_q8: validate -> plan_linear_q8 (linear_plan.cc: which kernel, which grid, which template arguments; int8 and fp8 share the
// dispatch table, except that fp8 has no 256 x 256 form) -> route text -> one switch on the family.  The LDS opt-in stays a launch-time
// action (once per device and format), so a dry run makes no HIP call.
template <bool F8>
static hipError_t launch_linear_q8(hipStream_t s, const int8_t* xq, const float* sx, const int8_t* w, const uint16_t* scale, int64_t M,
                                   int N, int K, void* y, int64_t ldy, bool out_fp32, bool swiglu, LinearRoute* route) {
    if (M == 0) return hipSuccess;
    if (swiglu && out_fp32) return hipErrorInvalidValue;
    const int epi = swiglu ? EPI_SWIGLU : (out_fp32 ? EPI_F32 : EPI_F16);
    if (!linear_q8_valid(M, N, K, ldy, epi)) return hipErrorInvalidValue;
    static const Q8Tuning tuning = Q8Tuning::from_env();
    const Q8Plan p = plan_linear_q8(F8, M, N, K, ldy, epi, tuning);
    if (!p.ok) return hipErrorInvalidValue;
    if (route) {
        char text[256];
        format_route(p, text, (int)sizeof text);
        route->add("%s", text);
        if (route->dry) return hipSuccess;
    }
    const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
    switch (p.family) {
        case QF_256:
            if constexpr (!F8) {
                static LdsOptIn once;  // (per device: see k_launch.h)
                if (once.first())
                    for_each_epi([](auto E) {
                        set_max_lds(i8_256_lds_bytes(3), gemm_i8_256_kernel<E, 3>);
                        set_max_lds(i8_256_lds_bytes(4), gemm_i8_256_kernel<E, 4>);
                    });
                dispatch_epi(epi, [&](auto E) {
                    dispatch_int<3, 4>(p.stages, [&](auto ST) {
                        hipLaunchKernelGGL((gemm_i8_256_kernel<E, ST>), grid, block, p.lds, s, xq, sx, w, scale, M, N, K, y, ldy, p.n_tiles, p.m_tiles,
                                           p.gn, p.gm);
                    });
                });
                break;
            }
            return hipErrorInvalidValue;   // (the plan gives fp8 no 256 x 256 form)
        case QF_WIDE: {
            static LdsOptIn once;
            if (once.first())
                set_max_lds(i8_wide_lds_bytes(), gemm_i8_wide_kernel<EPI_F16, F8>, gemm_i8_wide_kernel<EPI_F32, F8>, gemm_i8_wide_kernel<EPI_SWIGLU, F8>);
            dispatch_epi(epi, [&](auto E) {
                hipLaunchKernelGGL((gemm_i8_wide_kernel<E, F8>), grid, block, p.lds, s, xq, sx, w, scale, M, N, K, y, ldy, p.n_tiles, p.m_tiles);
            });
            break;
        }
        case QF_PC: {
            static LdsOptIn once;
            if (once.first())
                for_each_epi([](auto E) {
                    set_max_lds(i8_pc_lds_bytes(3), gemm_i8_pc_kernel<E, 3, F8>);
                    set_max_lds(i8_pc_lds_bytes(4), gemm_i8_pc_kernel<E, 4, F8>);
                    set_max_lds(i8_pc_lds_bytes(2), gemm_i8_pc_kernel<E, 2, F8>);
                });
            dispatch_epi(epi, [&](auto E) {
                dispatch_int<2, 3, 4>(p.stages, [&](auto ST) {
                    hipLaunchKernelGGL((gemm_i8_pc_kernel<E, ST, F8>), grid, block, p.lds, s, xq, sx, w, scale, M, N, K, y, ldy, p.n_tiles, p.m_tiles);
                });
            });
            break;
        }
        case QF_GEMV:
            dispatch_epi(epi, [&](auto E) {
                auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, xq, sx, w, scale, M, N, K, y, ldy); };
                if (p.mt == 2) go(gemv_i8_kernel<2, E, 4, F8>);
                else if (p.nw == 8) go(gemv_i8_kernel<1, E, 8, F8>);
                else go(gemv_i8_kernel<1, E, 4, F8>);
            });
            break;
    }
    return hipGetLastError();
}

hipError_t launch_linear_i8(hipStream_t s, const int8_t* xq, const float* sx, const int8_t* w, const uint16_t* scale, int64_t M, int N,
                            int K, void* y, int64_t ldy, bool out_fp32, bool swiglu, LinearRoute* route) {
    return launch_linear_q8<false>(s, xq, sx, w, scale, M, N, K, y, ldy, out_fp32, swiglu, route);
}

hipError_t launch_linear_f8(hipStream_t s, const uint8_t* xq, const float* sx, const uint8_t* w, const uint16_t* scale, int64_t M, int N,
                            int K, void* y, int64_t ldy, bool out_fp32, bool swiglu, LinearRoute* route) {
    return launch_linear_q8<true>(s, (const int8_t*)xq, sx, (const int8_t*)w, scale, M, N, K, y, ldy, out_fp32, swiglu, route);
}

}  // namespace pplhip
