// K3 / K9 / K11 linear layers: y[M,N] = x[M,K] . W[N,K]^T with weight-only quantisation (W8A16 per output
// channel, W4A16 per K-group, or plain fp16 weights).  MFMA-bound at the batch sizes of the headline
// configuration (M = 1024 rows: ~2*M flop per weight byte >> machine balance), so the kernel is an LDS-tiled
// mfma_f32_16x16x32_f16 GEMM with the int8 / int4 weights dequantised to fp16 on their way into LDS.
//
//   block tile 128 (weight rows n) x 128 (activation rows m) x 64 (k); 4 waves as 2 x 2, each 64 x 64 =
//   4 x 4 MFMA tiles; the WEIGHT fragment is the MFMA A operand and the activation fragment the B operand, so
//   the accumulator layout gives each lane 4 consecutive n of one activation row -> 8-byte (fp16) stores and
//   an 8-byte load of the 4 per-channel scales in the epilogue.
//   LDS tiles are [row][64] fp16 with the 16-byte chunk index XOR-swizzled by (row>>1)&7 (128-byte rows: two
//   rows per 256-byte bank window) so ds_read_b128 fragment reads are conflict-free.
//   global -> register -> LDS staging with the next tile's loads in flight during the MFMAs of the current.
//   1-D grid remapped so that the M-tiles of one weight tile run on the same XCD (its L2 then serves the tile
//   to all of them; MI355X_MICROARCH: block b -> XCD b % 8).
// Numerics: fp32 accumulate; W8: y = scale[n] * sum (exact int8 -> fp16); W4: fp16(q * scale) per element
// (one rounding).  Oracle: ref_linear_fwd (oracle/llama_ref.c).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include <type_traits>
#include "k_gemm_dev.h"

namespace pplhip {

void LinearRoute::add(const char* fmt, ...) {
    if (!buf || cap <= 0 || len >= cap - 1) return;
    if (len > 0) buf[len++] = ' ';
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf + len, (size_t)(cap - len), fmt, ap);
    va_end(ap);
    len = n < 0 ? len : (len + n < cap - 1 ? len + n : cap - 1);
    buf[len] = 0;
}

template <int WQ, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(const uint16_t* __restrict__ x, const void* __restrict__ wv,
                                                   const uint16_t* __restrict__ scale, int64_t M, int N, int K, int group,
                                                   void* __restrict__ yv, int64_t ldy, int n_tiles, int m_tiles) {
    __shared__ __attribute__((aligned(16))) uint16_t Ws[G_BN * G_BK];
    __shared__ __attribute__((aligned(16))) uint16_t Xs[G_BM * G_BK];

    int nt, mt;
    xcd_tile((int)blockIdx.x, m_tiles, nt, mt);
    if (nt >= n_tiles) return;
    const int n0 = nt * G_BN;
    const int64_t m0 = (int64_t)mt * G_BM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int wn = wave >> 1, wm = wave & 1;

    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    // staging registers
    uint4 xr[4];
    uint4 wr[WQ == 0 ? 4 : (WQ == 8 ? 2 : 1)];
    float wsc = 1.f;  // W4: group scale of this thread's chunk

    auto load_tile = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i, row = q >> 3, cc = q & 7;
            const int64_t m = m0 + row;
            const int k = k0 + cc * 8;
            xr[i] = (m < M && k < K) ? *reinterpret_cast<const uint4*>(x + m * K + k) : make_uint4(0, 0, 0, 0);
        }
        if constexpr (WQ == 0) {
            const uint16_t* w = reinterpret_cast<const uint16_t*>(wv);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = tid + 256 * i, row = q >> 3, cc = q & 7;
                const int n = n0 + row, k = k0 + cc * 8;
                wr[i] = (n < N && k < K) ? *reinterpret_cast<const uint4*>(w + (int64_t)n * K + k) : make_uint4(0, 0, 0, 0);
            }
        } else if constexpr (WQ == 8) {
            const int8_t* w = reinterpret_cast<const int8_t*>(wv);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q = tid + 256 * i, row = q >> 2, c16 = q & 3;
                const int n = n0 + row, k = k0 + c16 * 16;
                wr[i] = (n < N && k < K) ? *reinterpret_cast<const uint4*>(w + (int64_t)n * K + k) : make_uint4(0, 0, 0, 0);
            }
        } else {
            const uint8_t* w = reinterpret_cast<const uint8_t*>(wv);
            const int row = tid >> 1, c32 = tid & 1;
            const int n = n0 + row, k = k0 + c32 * 32;
            const bool ok = n < N && k < K;
            wr[0] = ok ? *reinterpret_cast<const uint4*>(w + ((int64_t)n * K + k) / 2) : make_uint4(0, 0, 0, 0);
            wsc = ok ? h2f(scale[(int64_t)n * (K / group) + k / group]) : 0.f;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i, row = q >> 3, cc = q & 7;
            *reinterpret_cast<uint4*>(&Xs[row * G_BK + g_swz(row, cc) * 8]) = xr[i];
        }
        if constexpr (WQ == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = tid + 256 * i, row = q >> 3, cc = q & 7;
                *reinterpret_cast<uint4*>(&Ws[row * G_BK + g_swz(row, cc) * 8]) = wr[i];
            }
        } else if constexpr (WQ == 8) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q = tid + 256 * i, row = q >> 2, c16 = q & 3;
                const uint32_t w4[4] = {wr[i].x, wr[i].y, wr[i].z, wr[i].w};
#pragma unroll
                for (int hc = 0; hc < 2; ++hc) {
                    h8 v;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int idx = hc * 8 + e;
                        v[e] = (_Float16)(int)(int8_t)(w4[idx >> 2] >> (8 * (idx & 3)));
                    }
                    *reinterpret_cast<uint4*>(&Ws[row * G_BK + g_swz(row, c16 * 2 + hc) * 8]) = __builtin_bit_cast(uint4, v);
                }
            }
        } else {
            const int row = tid >> 1, c32 = tid & 1;
            const uint32_t w4[4] = {wr[0].x, wr[0].y, wr[0].z, wr[0].w};
#pragma unroll
            for (int hc = 0; hc < 4; ++hc) {
                h8 v;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int idx = hc * 8 + e;  // element 0..31; byte idx>>1, low nibble = even element
                    const uint32_t byte = (w4[idx >> 3] >> (8 * ((idx >> 1) & 3))) & 0xffu;
                    const int nib = (idx & 1) ? (int)(byte >> 4) : (int)(byte & 15u);
                    v[e] = (_Float16)((float)(nib - 8) * wsc);
                }
                *reinterpret_cast<uint4*>(&Ws[row * G_BK + g_swz(row, c32 * 4 + hc) * 8]) = __builtin_bit_cast(uint4, v);
            }
        }
    };

    const int ktiles = (K + G_BK - 1) / G_BK;
    load_tile(0);
    store_tile();
    __syncthreads();
    for (int t = 0; t < ktiles; ++t) {
        if (t + 1 < ktiles) load_tile((t + 1) * G_BK);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            h8 a[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wn * 64 + i * 16 + l15;
                a[i] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&Ws[row * G_BK + g_swz(row, ks * 4 + kq) * 8]));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wm * 64 + j * 16 + l15;
                bfr[j] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&Xs[row * G_BK + g_swz(row, ks * 4 + kq) * 8]));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (t + 1 < ktiles) {
            store_tile();
            __syncthreads();
        }
    }

    // epilogue: lane holds, for activation row m = .. + l15, weight rows n = .. + kq*4 + r (r = 0..3)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + kq * 4;
        if (n >= N) continue;  // N is a multiple of 4 (checked by the launcher)
        float sc[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (WQ == 8) {
            const uint2 s2 = *reinterpret_cast<const uint2*>(scale + n);
            const h4 sh = __builtin_bit_cast(h4, s2);
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[r] = (float)sh[r];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = m0 + wm * 64 + j * 16 + l15;
            if (m >= M) continue;
            store4<EPI>(yv, ldy, m, n, acc[i][j][0] * sc[0], acc[i][j][1] * sc[1], acc[i][j][2] * sc[2], acc[i][j][3] * sc[3]);
        }
    }
}

// stand-alone launch of the tile body (k_gemm_dev.h)
template <int WQ, int EPI, int G_ST, int WL, int BM = G_BM, int MAXG = W4_MAXG>
__global__ __launch_bounds__(WL == 6 ? 768 : (WL == 5 ? 512 : 256)) void gemm_dma_kernel(const uint16_t* __restrict__ x, const void* __restrict__ wv,
                                                             const uint16_t* __restrict__ scale, int64_t M, int N, int K,
                                                             void* __restrict__ yv, int64_t ldy, int n_tiles, int m_tiles,
                                                             int map_mode, int kt_per_split, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) char smem[gemm_dma_lds_bytes(WQ, G_ST, BM, MAXG)];
    gemm_dma_body<WQ, EPI, G_ST, WL, BM>(x, wv, scale, M, N, K, yv, ldy, n_tiles, m_tiles, map_mode, kt_per_split, ws, (int)blockIdx.x,
                                     (int)blockIdx.y, (int)gridDim.y, smem);
}

// ---------------------------------------------------------------------------------------------------------------
// W8A16, 4 < M <= 64 (decode steps of a few dozen requests): the half-height tile with a 128-deep K tile (round 4).
// These steps are bound by the weight stream (2 M flop per weight byte), and the 64-deep tile of gemm_dma_body fetches HALF a 128-byte
// line of every weight row per LDS-DMA piece (16 rows x 64 B) -- the access pattern that held the MFMA skinny kernel at 2.75 TB/s
// (k_gemv.hip: whole lines 4.3 TB/s); the 7B layer at M = 64 ran at 2.4 TB/s.  Here a piece is 8 weight rows x 128 B: the weight stage
// is [128 rows][128 B] (two 64-deep sub-tiles side by side, chunk-swizzled like an activation tile), the activation stage two
// [64 rows][64 fp16] sub-tiles; 4 waves of 32 (n) x 64 (m), 32 MFMAs per wave and stage, split-K slabs + the common reduce kernel.
// ---------------------------------------------------------------------------------------------------------------
// Round 4, second step: the activation sub-tile is as tall as the batch needs (BM = 16 / 32 / 64 rows), so that the LDS a block does not
// spend on padding rows holds more stages of the weight stream: what bounds these steps is weight bytes in flight per CU (32 KiB with two
// 64-row blocks of two stages; 64 KiB with three stages of a 16- or 32-row block, two blocks per CU).
// (S_KS = 2 64-deep sub-tiles per stage, S_WB weight and s_xb(BM) activation bytes per stage: k_gemm_tiles.h)
template <int EPI, int ST, int BM>
__global__ __launch_bounds__(256) void gemm_w8_half128_kernel(const uint16_t* __restrict__ x, const int8_t* __restrict__ w,
                                                              const uint16_t* __restrict__ scale, int64_t M, int N, int K,
                                                              void* __restrict__ yv, int64_t ldy, int n_tiles, int kt_per_split,
                                                              float* __restrict__ ws) {
    constexpr int XB = s_xb(BM), NJ = BM / 16;
    constexpr int XP = XB / 1024, WP = S_WB / 1024, PP = (XP + WP) / 4;   // 1-KiB DMA pieces per stage: X, W, per wave (5 / 6 / 8)
    static_assert((XP + WP) % 4 == 0, "every wave issues the same number of pieces");
    extern __shared__ __attribute__((aligned(16))) char smem_h[];  // ST x X, then ST x W
    char* const Xs0 = smem_h;
    char* const Wq0 = smem_h + ST * XB;
    const int nt = blockIdx.x;               // (one activation tile; XCD id % 8 streams the weight tiles n == id (mod 8))
    if (nt >= n_tiles) return;
    const int n0 = nt * G_BN;
    const int split_id = blockIdx.y, n_splits = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    const int nb = wave * 32;

    // piece P = wave + 4 j of a stage.  P < XP: activation sub-tile u = P / (BM / 8), rows 8 (P % (BM / 8)) .. + 8, chunk permutation of
    // gemm_dma_body (ONE 16-byte read of an int8 row then serves both k-steps of a lane); else weight rows 8 (P - XP) .. + 8, 128 B each
    const char* psrc[PP];
    uint32_t pdst[PP];
    const uint32_t xbase = lds_addr(Xs0), wbase = lds_addr(Wq0);
#pragma unroll
    for (int j = 0; j < PP; ++j) {
        const int P = wave + 4 * j;
        if (P < XP) {
            const int u = P / (BM / 8), q = P % (BM / 8);
            const int row = q * 8 + (lane >> 3), pos = (lane & 7) ^ ((row >> 1) & 7);
            const int c = ((pos & 3) << 1) | (pos >> 2);
            int64_t m = row;
            if (m >= M) m = M - 1;
            psrc[j] = reinterpret_cast<const char*>(x + m * K + u * G_BK + c * 8);
            pdst[j] = __builtin_amdgcn_readfirstlane(xbase + P * 1024);
        } else {
            const int row = (P - XP) * 8 + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
            int n = n0 + row;
            if (n >= N) n = N - 1;
            psrc[j] = reinterpret_cast<const char*>(w) + (int64_t)n * K + c * 16;
            pdst[j] = __builtin_amdgcn_readfirstlane(wbase + (P - XP) * 1024);
        }
    }
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            const bool isx = wave + 4 * j < XP;   // (wave-uniform)
            glds16(psrc[j] + (isx ? (int64_t)k0 * 2 : (int64_t)k0), pdst[j] + stage * (isx ? XB : S_WB));
        }
    };
    constexpr int D = ST - 1;

    f4 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    const int kt_all = K / (G_BK * S_KS);
    const int kt0 = split_id * kt_per_split;
    const int ktiles = (kt0 + kt_per_split < kt_all) ? kt_per_split : kt_all - kt0;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < ktiles) issue(d, (kt0 + d) * (G_BK * S_KS));
    int st = 0, stn = D % ST;
    for (int t = 0; t < ktiles; ++t) {
        ring_wait<PP>((ktiles - 1 - t) < (D - 1) ? (ktiles - 1 - t) : (D - 1));
        __syncthreads();
        if (t + D < ktiles) issue(stn, (kt0 + t + D) * (G_BK * S_KS));
        const char* xs0 = Xs0 + st * XB;
        const char* wq = Wq0 + st * S_WB;
        st = st == ST - 1 ? 0 : st + 1;
        stn = stn == ST - 1 ? 0 : stn + 1;
#pragma unroll
        for (int u = 0; u < S_KS; ++u) {
            const uint16_t* xs = reinterpret_cast<const uint16_t*>(xs0 + u * (BM * G_BK * 2));
            uint4 wraw[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = nb + i * 16 + l15;
                wraw[i] = *reinterpret_cast<const uint4*>(&wq[row * 128 + g_swz(row, u * 4 + kq) * 16]);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                h8 a[2], bfr[NJ];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = cvt_i8x8_f16(ks == 0 ? make_uint2(wraw[i].x, wraw[i].y) : make_uint2(wraw[i].z, wraw[i].w));
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int row = j * 16 + l15;
                    bfr[j] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&xs[row * G_BK + g_swz(row, ks * 4 + kq) * 8]));
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    if (n_splits > 1) {  // fp32 partial slab [split][M][N]
        float* slab = ws + (int64_t)split_id * M * N;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = n0 + nb + i * 16 + kq * 4;
            if (n >= N) continue;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int64_t m = j * 16 + l15;
                if (m < M) *reinterpret_cast<float4*>(slab + m * N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + nb + i * 16 + kq * 4;
        if (n >= N) continue;
        const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + n));
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t m = j * 16 + l15;
            if (m >= M) continue;
            store4<EPI>(yv, ldy, m, n, acc[i][j][0] * (float)sh[0], acc[i][j][1] * (float)sh[1], acc[i][j][2] * (float)sh[2],
                        acc[i][j][3] * (float)sh[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// W8A16, large M (prefill steps, M >= 4096): 256 x 256 x 64 block tile, 8 waves as 8 (n) x 1 (m), wave tile
// 32 (n) x 256 (m) = 2 x 16 MFMA tiles (each weight fragment is converted once and feeds 16 MFMAs; +2.5 % over 4 x 2).  Same DMA / int8-in-LDS / swizzle scheme as the 128 x 128 kernel, but per MFMA it
// reads ~40 % fewer LDS bytes and converts half as many weight fragments, and each activation / weight byte fetched
// from L2 feeds twice the flops.  One block per CU (3-stage ring = 144 KiB LDS), prefetch distance 2.
// ---------------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void gemm_w8_dma256_kernel(const uint16_t* __restrict__ x, const int8_t* __restrict__ w,
                                                             const uint16_t* __restrict__ scale, int64_t M, int N, int K,
                                                             void* __restrict__ yv, int64_t ldy, int n_tiles, int m_tiles, int gn, int gm, int staged) {
    extern __shared__ __attribute__((aligned(16))) char smem256[];  // H_ST x (X 32 KiB + W 16 KiB)
    uint16_t* const Xs0 = reinterpret_cast<uint16_t*>(smem256);
    int8_t* const Wq0 = reinterpret_cast<int8_t*>(smem256 + H_ST * H_BM * G_BK * 2);

    // block -> tile in super-tiles (xcd_super_tile): the ~32 blocks an XCD runs at a time touch gn weight tiles and gm activation tiles
    // per K step instead of 1 and 32, i.e. a third of the bytes through its L2
    int nt, mt;
    xcd_super_tile((int)blockIdx.x, m_tiles, gn, gm, nt, mt);
    if (nt >= n_tiles) return;
    const int n0 = nt * H_BN;
    const int64_t m0 = (int64_t)mt * H_BM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int wn = wave, wm = 0;  // 8 (n) x 1 (m): wave tile 32 (n) x 256 (m); every weight fragment is converted by one wave only

    const uint16_t* xsrc[4];
    const int8_t* wsrc[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = j * 512 + tid, row = p >> 3, pos = (p & 7) ^ ((row >> 1) & 7);
        const int c = ((pos & 3) << 1) | (pos >> 2);
        int64_t m = m0 + row;
        if (m >= M) m = M - 1;
        xsrc[j] = x + m * K + c * 8;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = j * 512 + tid, row = p >> 2, c = (p & 3) ^ w_swz(row);
        int n = n0 + row;
        if (n >= N) n = N - 1;
        wsrc[j] = w + (int64_t)n * K + c * 16;
    }
    const uint32_t xdst = __builtin_amdgcn_readfirstlane(lds_addr(Xs0) + wave * 1024);
    const uint32_t wdst = __builtin_amdgcn_readfirstlane(lds_addr(Wq0) + wave * 1024);
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(xsrc[j] + k0, xdst + stage * (H_BM * G_BK * 2) + j * 8192);
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(wsrc[j] + k0, wdst + stage * (H_BN * G_BK) + j * 8192);
    };

    f4 acc[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int ktiles = K / G_BK;
    issue(0, 0);
    if (ktiles > 1) issue(1, G_BK);
    int st = 0, stn = 2;
    for (int t = 0; t < ktiles; ++t) {
        if (t + 1 < ktiles) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 2 < ktiles) issue(stn, (t + 2) * G_BK);
        const uint16_t* xs = Xs0 + st * (H_BM * G_BK);
        const int8_t* wq = Wq0 + st * (H_BN * G_BK);
        st = st == H_ST - 1 ? 0 : st + 1;
        stn = stn == H_ST - 1 ? 0 : stn + 1;
        uint4 wraw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wn * 32 + i * 16 + l15;
            wraw[i] = *reinterpret_cast<const uint4*>(&wq[row * G_BK + (kq ^ w_swz(row)) * 16]);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            h8 a[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = cvt_i8x8_f16(ks == 0 ? make_uint2(wraw[i].x, wraw[i].y) : make_uint2(wraw[i].z, wraw[i].w));
#pragma unroll
            for (int jh = 0; jh < 4; ++jh) {
                h8 bfr[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = wm * 128 + (jh * 4 + j) * 16 + l15;
                    bfr[j] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&xs[row * G_BK + g_swz(row, ks * 4 + kq) * 8]));
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][jh * 4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bfr[j], acc[i][jh * 4 + j], 0, 0, 0);
            }
        }
    }

    if (staged && EPI != EPI_F32) {
        // Output through LDS (the ring is idle; round 4): the MFMA layout gives a store instruction 32 bytes of 16 different rows; staged,
        // a wave stores 512 contiguous bytes of two rows (16 bytes per lane).  On multi-round prefill GEMMs the partial-line stores of
        // finishing blocks otherwise sit in the memory pipeline beside the running blocks' tile fetches (measured on the asm-loop
        // kernel: w13 at M = 8192 1593 -> 1382 us, profiles/r04_gemm_asm_experiments.md).  Rows padded by 16 bytes against bank conflicts.
        constexpr int OUTW = EPI == EPI_SWIGLU ? H_BN / 2 : H_BN, ROWB = OUTW * 2 + 16, CPR = OUTW / 8;
        static_assert(H_BM * ROWB <= H_ST * (H_BM * G_BK * 2 + H_BN * G_BK), "the staging image fits the ring");
        char* const stg = smem256;
        __syncthreads();  // every wave is past its last fragment read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nl = wn * 32 + i * 16 + kq * 4;
            const int nc = n0 + nl < N ? n0 + nl : 0;
            const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + nc));
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float v0 = acc[i][j][0] * (float)sh[0], v1 = acc[i][j][1] * (float)sh[1], v2 = acc[i][j][2] * (float)sh[2],
                            v3 = acc[i][j][3] * (float)sh[3];
                char* dst = stg + (j * 16 + l15) * ROWB;
                if constexpr (EPI == EPI_F16) {
                    const h4 o = {to_h(v0), to_h(v1), to_h(v2), to_h(v3)};
                    *reinterpret_cast<uint2*>(dst + nl * 2) = __builtin_bit_cast(uint2, o);
                } else {
                    const float g0 = round_h(v0), u0 = round_h(v1), g1 = round_h(v2), u1 = round_h(v3);
                    const h2 o = {to_h(g0 / (1.0f + __expf(-g0)) * u0), to_h(g1 / (1.0f + __expf(-g1)) * u1)};
                    *reinterpret_cast<uint32_t*>(dst + nl) = __builtin_bit_cast(uint32_t, o);
                }
            }
        }
        __syncthreads();
        uint16_t* const y = reinterpret_cast<uint16_t*>(yv);
        const int nout = EPI == EPI_SWIGLU ? N / 2 : N, c0 = EPI == EPI_SWIGLU ? n0 / 2 : n0;
#pragma unroll 4
        for (int c = tid; c < H_BM * CPR; c += 512) {
            const int row = c / CPR, ch = c - row * CPR;
            const uint4 v = *reinterpret_cast<const uint4*>(stg + row * ROWB + ch * 16);
            const int64_t m = m0 + row;
            const int col = c0 + ch * 8;
            if (m < M) {
                if (col + 8 <= nout) {
                    *reinterpret_cast<uint4*>(y + m * ldy + col) = v;
                } else {
                    const uint16_t* e = reinterpret_cast<const uint16_t*>(&v);
                    for (int k = 0; k < 8; ++k)
                        if (col + k < nout) y[m * ldy + col + k] = e[k];
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + wn * 32 + i * 16 + kq * 4;
        if (n >= N) continue;
        const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + n));
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t m = m0 + wm * 128 + j * 16 + l15;
            if (m >= M) continue;
            store4<EPI>(yv, ldy, m, n, acc[i][j][0] * (float)sh[0], acc[i][j][1] * (float)sh[1], acc[i][j][2] * (float)sh[2],
                        acc[i][j][3] * (float)sh[3]);
        }
    }
}

// MFMA skinny kernel, M <= 16: one 16-row activation tile (MT = 1 is the only form compiled)
template <int WQ, int MT, int EPI, int NW>
__global__ __launch_bounds__(NW * 64) void gemv_kernel(const uint16_t* __restrict__ x, const void* __restrict__ wv,
                                                   const uint16_t* __restrict__ scale, int64_t M, int N, int K, int group,
                                                   void* __restrict__ yv, int64_t ldy) {
    static_assert(MT == 1, "launch_linear takes this kernel up to 16 rows only");
    constexpr int KL = WQ == 8 ? 16 : (WQ == 4 ? 32 : 8);  // k elements in one lane's 16 bytes
    constexpr int KSTEP = KL * 4;                          // k elements per wave-load
    constexpr int NKS = KL / 8;                            // MFMA k-steps per load
    __shared__ __attribute__((aligned(16))) float red[NW - 1][MT][64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    int n = n0 + l15;
    if (n >= N) n = N - 1;
    const int steps = (K + KSTEP - 1) / KSTEP;
    const int per = (steps + NW - 1) / NW;
    const int s_begin = wave * per, s_end = (s_begin + per < steps) ? s_begin + per : steps;
    const char* wrow = reinterpret_cast<const char*>(wv) + ((int64_t)n * K * (WQ == 0 ? 16 : WQ)) / 8;
    const uint16_t* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int64_t m = mt * 16 + l15;
        if (m >= M) m = M - 1;
        xrow[mt] = x + m * K;
    }
    f4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f4{0.f, 0.f, 0.f, 0.f};

    // U wave-loads of weights are issued before the first is consumed: a block streams 16 rows once, so the bytes it keeps
    // in flight (U KiB per wave) set its share of the HBM bandwidth (measured: 2.6 TB/s with one load in flight)
    constexpr int U = 8;
    for (int st0 = s_begin; st0 < s_end; st0 += U) {
        uint4 wr[U];
        float wsc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = (st0 + u) * KSTEP + kq * KL;
            const bool ok = st0 + u < s_end && k < K;  // K is a multiple of KL (checked by the launcher)
            wr[u] = ok ? *reinterpret_cast<const uint4*>(wrow + ((int64_t)k * (WQ == 0 ? 16 : WQ)) / 8) : make_uint4(0, 0, 0, 0);
            wsc[u] = 1.f;
            if constexpr (WQ == 4) wsc[u] = ok ? h2f(scale[(int64_t)n * (K / group) + k / group]) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = (st0 + u) * KSTEP + kq * KL;
            const bool ok = st0 + u < s_end && k < K;
            const uint32_t w4[4] = {wr[u].x, wr[u].y, wr[u].z, wr[u].w};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                h8 a;
                if constexpr (WQ == 0) {
                    a = __builtin_bit_cast(h8, wr[u]);
                } else if constexpr (WQ == 8) {
                    a = cvt_i8x8_f16(make_uint2(w4[ks * 2], w4[ks * 2 + 1]));
                } else {
                    const _Float16 sh = (_Float16)wsc[u];  // exact: wsc came from an fp16
                    a = cvt_i4x8_f16(w4[ks], h2{sh, sh});  // 8 nibbles, low nibble = even k
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const uint4 xr = ok ? *reinterpret_cast<const uint4*>(xrow[mt] + k + ks * 8) : make_uint4(0, 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, xr), acc[mt], 0, 0, 0);
                }
            }
        }
    }
    // sum the NW K slices
    if (wave > 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f4*>(red[wave - 1][mt][lane]) = acc[mt];
    }
    __syncthreads();
    if (wave == 0) {
        const int nn = n0 + kq * 4;
        if (nn < N) {
            float sc[4] = {1.f, 1.f, 1.f, 1.f};
            if constexpr (WQ == 8) {
                const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + nn));
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[r] = (float)sh[r];
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f4 v = acc[mt];
#pragma unroll
                for (int w = 0; w < NW - 1; ++w) {
                    const f4 o = *reinterpret_cast<const f4*>(red[w][mt][lane]);
                    v += o;
                }
                const int64_t m = mt * 16 + l15;
                if (m >= M) continue;
                store4<EPI>(yv, ldy, m, nn, v[0] * sc[0], v[1] * sc[1], v[2] * sc[2], v[3] * sc[3]);
            }
        }
    }
}

// split-K reduce: y[m][n] = (sum_z slab[z][m][n]) * scale[n]  (scale == NULL: 1)
template <int EPI>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, int splits, int64_t M, int N,
                                                            const uint16_t* __restrict__ scale, void* __restrict__ yv, int64_t ldy) {
    const int64_t total = M * (N / 4);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / (N / 4);
        const int n = (int)(i - m * (N / 4)) * 4;
        float4 v = *reinterpret_cast<const float4*>(ws + m * N + n);
        for (int z = 1; z < splits; ++z) {
            const float4 o = *reinterpret_cast<const float4*>(ws + ((int64_t)z * M + m) * N + n);
            v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (scale) {
            const h4 sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(scale + n));
            v.x *= (float)sh[0]; v.y *= (float)sh[1]; v.z *= (float)sh[2]; v.w *= (float)sh[3];
        }
        store4<EPI>(yv, ldy, m, n, v.x, v.y, v.z, v.w);
    }
}

hipError_t launch_splitk_reduce(hipStream_t s, const float* ws, int splits, int64_t M, int N, const uint16_t* scale, void* y, int64_t ldy, int epi) {
    const int64_t total = M * (N / 4);
    if (total == 0) return hipSuccess;
    const unsigned rb = (unsigned)std::min<int64_t>((total + 255) / 256, 2048);
    dispatch_epi(epi, [&](auto E) { hipLaunchKernelGGL(splitk_reduce_kernel<E>, dim3(rb), dim3(256), 0, s, ws, splits, M, N, scale, y, ldy); });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// launch_linear: validate -> plan_linear (linear_plan.cc: which kernel, which grid, which template arguments) -> route text -> launch.
// The launchers below instantiate a family's kernels from its part of the plan; a family with dynamic LDS names its instantiations in
// ONE list that both the opt-in and the dispatch walk.
// ---------------------------------------------------------------------------------------------------------------
namespace {

struct LinearArgs {   // the operands of one part
    hipStream_t s;
    const uint16_t* x;
    const void* w;
    const uint16_t* scale;
    int group, N, K;
    void* y;
    int64_t ldy;
    float* ws;
};

void run_gemv(const LinearPart& p, const LinearArgs& a) {
    dispatch_int<0, 8, 4>(p.wq, [&](auto WQ) {
        dispatch_epi(p.epi, [&](auto E) {
            dispatch_int<8, 4>(p.nw, [&](auto NW) {
                hipLaunchKernelGGL((gemv_kernel<WQ, 1, E, NW>), dim3(p.grid_x), dim3(p.threads), 0, a.s, a.x, a.w, a.scale, p.M, a.N, a.K, a.group, a.y, a.ldy);
            });
        });
    });
}

void run_w8_256(const LinearPart& p, const LinearArgs& a) {
    static LdsOptIn once;
    if (once.first()) for_each_epi([](auto E) { set_max_lds(H_LDS, gemm_w8_dma256_kernel<E>); });
    dispatch_epi(p.epi, [&](auto E) {
        hipLaunchKernelGGL((gemm_w8_dma256_kernel<E>), dim3(p.grid_x), dim3(p.threads), p.lds, a.s, a.x, (const int8_t*)a.w, a.scale, p.M, a.N, a.K, a.y,
                           a.ldy, p.n_tiles, p.m_tiles, (int)p.map.gn, (int)p.map.gm, p.staged);
    });
}

// the (stages, activation rows) instantiations of gemm_w8_half128_kernel; two stages: 64-row sub-tiles only
template <class F>
void for_each_half128(F&& f) {
    f(int_c<3>{}, int_c<16>{}); f(int_c<3>{}, int_c<32>{}); f(int_c<2>{}, int_c<64>{}); f(int_c<3>{}, int_c<64>{});
    f(int_c<3>{}, int_c<80>{}); f(int_c<3>{}, int_c<96>{}); f(int_c<3>{}, int_c<112>{}); f(int_c<3>{}, int_c<128>{});
}
void run_w8_half128(const LinearPart& p, const LinearArgs& a) {
    static LdsOptIn once;
    if (once.first())
        for_each_epi([](auto E) {
            for_each_half128([&](auto ST, auto BM) { set_max_lds(half128_lds_bytes(ST, BM), gemm_w8_half128_kernel<E, ST, BM>); });
        });
    dispatch_epi(p.epi, [&](auto E) {
        for_each_half128([&](auto ST, auto BM) {
            if (ST == p.stages && BM == p.bm)
                hipLaunchKernelGGL((gemm_w8_half128_kernel<E, ST, BM>), dim3(p.grid_x, p.grid_y), dim3(p.threads), p.lds, a.s, a.x, (const int8_t*)a.w,
                                   a.scale, p.M, a.N, a.K, a.y, a.ldy, p.n_tiles, p.kt_per, a.ws);
        });
    });
}

void run_ring(const LinearPart& p, const LinearArgs& a) {
    dispatch_int<8, 4, 0>(p.wq, [&](auto WQ) {
        dispatch_epi(p.epi, [&](auto E) {
            dispatch_int<2, 3, 4>(p.stages, [&](auto ST) {
                auto go = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(p.threads), 0, a.s, a.x, a.w, a.scale, p.M, a.N, a.K, a.y, a.ldy, p.n_tiles,
                                       p.m_tiles, map_pack(p.map), p.kt_per, a.ws);
                };
                if constexpr (WQ == 8 && ST >= 3) {
                    if (p.wl == 6) return go(gemm_dma_kernel<WQ, E, ST, 6>);
                }
                if (p.wl == 5) go(gemm_dma_kernel<WQ, E, ST, 5>);
                else if (p.bm == 64) go(gemm_dma_kernel<WQ, E, ST, 1, 64>);
                else if (p.maxg == 16) go(gemm_dma_kernel<WQ, E, ST, 1, G_BM, 16>);
                else go(gemm_dma_kernel<WQ, E, ST, 1>);
            });
        });
    });
}

void run_generic(const LinearPart& p, const LinearArgs& a) {
    dispatch_int<0, 8, 4>(p.wq, [&](auto WQ) {
        dispatch_epi(p.epi, [&](auto E) {
            hipLaunchKernelGGL((gemm_kernel<WQ, E>), dim3(p.grid_x), dim3(p.threads), 0, a.s, a.x, a.w, a.scale, p.M, a.N, a.K, a.group, a.y, a.ldy,
                               p.n_tiles, p.m_tiles);
        });
    });
}

}  // namespace

hipError_t launch_linear(hipStream_t s, const uint16_t* x, const void* w, const uint16_t* scale, int wq_bit, int group,
                         int64_t M, int N, int K, void* y, int64_t ldy, bool out_fp32, float* ws, size_t ws_bytes, bool swiglu, SplitSlabs* defer,
                         LinearRoute* route) {
    if (defer) *defer = SplitSlabs{};
    if (M == 0) return hipSuccess;
    if (swiglu && out_fp32) return hipErrorInvalidValue;
    LinearProblem pr;
    pr.wq_bit = wq_bit, pr.group = group, pr.M = M, pr.N = N, pr.K = K, pr.ldy = ldy;
    pr.epi = swiglu ? EPI_SWIGLU : (out_fp32 ? EPI_F32 : EPI_F16);
    pr.ws_bytes = ws ? ws_bytes : 0;
    pr.accept_defer = defer != nullptr;
    pr.x = (uintptr_t)x, pr.w = (uintptr_t)w, pr.scale = (uintptr_t)scale, pr.y = (uintptr_t)y;
    if (!linear_problem_valid(pr)) return hipErrorInvalidValue;
    static const LinearTuning tuning = LinearTuning::from_env();
    const LinearPlan plan = plan_linear(pr, tuning);
    if (!plan.ok) return hipErrorInvalidValue;
    if (route) {
        char text[512];
        format_route(plan, text, (int)sizeof text);
        route->add("%s", text);
        if (route->dry) return hipSuccess;
    }
    const uint16_t* rscale = wq_bit == 8 ? scale : nullptr;   // the channel scales a reduce applies
    for (int i = 0; i < plan.n_parts; ++i) {
        const LinearPart& p = plan.part[i];
        const LinearArgs a{s, x + p.m0 * K, w, scale, group, N, K, (char*)y + (size_t)p.m0 * ldy * (out_fp32 ? 4 : 2), ldy, ws};
        hipError_t e = hipSuccess;
        bool sub = false;   // a sub-launcher checked its own launch
        switch (p.family) {
            case LF_GEMV_STREAM: sub = true, e = launch_gemv_stream(s, a.x, w, scale, wq_bit, group, p.M, N, K, a.y, ldy, p.epi); break;
            case LF_W4_PC: sub = true, e = launch_linear_w4_pc(s, a.x, w, scale, p.M, N, K, a.y, ldy, p.epi); break;
            case LF_W8_WIDE: sub = true, e = launch_linear_w8_wide(s, a.x, (const int8_t*)w, scale, p.M, N, K, a.y, ldy, p.epi, p.nc); break;
            case LF_GEMV: run_gemv(p, a); break;
            case LF_W8_256: run_w8_256(p, a); break;
            case LF_W8_HALF128: run_w8_half128(p, a); break;
            case LF_RING: run_ring(p, a); break;
            case LF_GENERIC: run_generic(p, a); break;
        }
        if (!sub) e = hipGetLastError();
        if (e != hipSuccess) return e;
        // split-K: the slabs go to the consumer (defer) or through the reduce kernel
        if (p.reduce == LR_DEFERRED) *defer = SplitSlabs{ws, p.splits, rscale, N, p.M};
        else if (p.reduce == LR_KERNEL && (e = launch_splitk_reduce(s, ws, p.splits, p.M, N, rscale, a.y, ldy, p.epi)) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pplhip
