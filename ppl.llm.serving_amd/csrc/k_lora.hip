// Multi-LoRA: the low-rank update of a layer linear for the rows of a step whose request carries an adapter (DESIGN.md "numerics"):
//   shrink  t[m, j] = fp16( sum_k x[m, k] A[j, k] )                                   fp32 sums
//   expand  y[m, n] = fp16( fp32(y[m, n]) + scale * sum_j fp32(t[m, j]) B[n, j] )     fp32 sums, in place
// Both work on the host-built tile list (kernels.h LoraTile): up to 16 row indices that share one adapter slot, padding marked -1.  A
// kernel never searches or sorts; it trusts the list (the host validated slot and row ranges) and touches no row the list does not name:
// padding rows are masked on the loads and on the stores.
//
// The tile is the 16-wide side of mfma_f32_16x16x32_f16.  The factor rows go in as the A operand (A[j, k .. k + 7] for shrink,
// B[n, j .. j + 7] for expand), the token rows as the B operand (x[m, k .. k + 7] / t[m, j .. j + 7]): every fragment is one 16-byte global
// load contiguous along the summed index, so nothing is staged through LDS, and a lane ends up with four consecutive outputs of ONE token
// row (C row = 4 (lane >> 4) + reg on the factor side, C column = lane & 15 on the token side): 8-byte accesses of y.
#include "kernels.h"

namespace pplhip {

namespace {

constexpr int LORA_WAVES = 4;        // shrink: K is split over the block's waves (32 columns a step) and reduced once through LDS
                                     // (measured, profiles/lora_step.jsonl: a launch pair is bound by this loop's K / 128 memory round trips per
                                     // wave, 43 us with 8 tiles and 49 us with 64 -- more waves along K is the next step)
constexpr int LORA_RED_LD = LORA_MAX_RANK + 4;   // floats per token row of a wave's partial sums (+ 4: rows start on different banks)
constexpr int LORA_EXPAND_COLS = 256;            // output columns per expand block: 64 per wave, four 16-column MFMA tiles

__device__ __forceinline__ h8 load_h8(const uint16_t* p) { return __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(p)); }

// a wave's share of the K loop for a tile of NJT 16-rank column tiles, the rank a template argument: with the rank as a run-time bound of
// the unrolled loop the compiler branched around every fragment load and drained vmcnt in front of every MFMA -- NJT + 1 memory round trips
// in series per K step, which is what the launches cost (profiles/lora_step.jsonl, kernels "serial loads")
template <int NJT>
__device__ __forceinline__ void lora_shrink_steps(const uint16_t* __restrict__ xp, bool row_ok, const uint16_t* __restrict__ ap, int K, int wave, f4* acc) {
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    constexpr int STEP = LORA_WAVES * 32;
    int k0 = wave * 32;
    if (k0 >= K) return;
    h8 xv = row_ok ? load_h8(xp + k0) : zero, av[NJT];
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) av[jt] = load_h8(ap + (int64_t)jt * 16 * K + k0);
    for (; k0 < K; k0 += STEP) {
        // the next step's fragments are on their way while this step multiplies (the last step re-reads itself: no branch in the loop)
        const int kn = k0 + STEP < K ? k0 + STEP : k0;
        const h8 xn = row_ok ? load_h8(xp + kn) : zero;
        h8 an[NJT];
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) an[jt] = load_h8(ap + (int64_t)jt * 16 * K + kn);
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[jt], xv, acc[jt], 0, 0, 0);
        xv = xn;
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) av[jt] = an[jt];
    }
}

__global__ __launch_bounds__(LORA_WAVES * WAVE) void lora_shrink_kernel(const LoraTile* __restrict__ tiles, const LoraSlot* __restrict__ slots,
                                                                        const uint16_t* __restrict__ x, int64_t ldx, int K,
                                                                        uint16_t* __restrict__ t) {
    __shared__ float red[LORA_WAVES][16][LORA_RED_LD];
    const LoraTile& tl = tiles[blockIdx.x];
    const LoraSlot sl = slots[tl.slot];
    if (!sl.a) return;   // (block-uniform) this adapter does not touch this linear
    const int rp = sl.rp, njt = rp >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int row = tl.row[l15];
    const uint16_t* xp = x + (int64_t)(row < 0 ? 0 : row) * ldx + kq * 8;
    const uint16_t* ap = sl.a + (int64_t)l15 * K + kq * 8;
    f4 acc[LORA_MAX_RANK / 16];
#pragma unroll
    for (int jt = 0; jt < LORA_MAX_RANK / 16; ++jt) acc[jt] = f4{0.f, 0.f, 0.f, 0.f};
    switch (njt) {   // (block-uniform)
        case 1: lora_shrink_steps<1>(xp, row >= 0, ap, K, wave, acc); break;
        case 2: lora_shrink_steps<2>(xp, row >= 0, ap, K, wave, acc); break;
        case 3: lora_shrink_steps<3>(xp, row >= 0, ap, K, wave, acc); break;
        case 4: lora_shrink_steps<4>(xp, row >= 0, ap, K, wave, acc); break;
        case 5: lora_shrink_steps<5>(xp, row >= 0, ap, K, wave, acc); break;
        case 6: lora_shrink_steps<6>(xp, row >= 0, ap, K, wave, acc); break;
        case 7: lora_shrink_steps<7>(xp, row >= 0, ap, K, wave, acc); break;
        default: lora_shrink_steps<8>(xp, row >= 0, ap, K, wave, acc); break;
    }
#pragma unroll
    for (int jt = 0; jt < LORA_MAX_RANK / 16; ++jt)
        if (jt < njt) *reinterpret_cast<f4*>(&red[wave][l15][jt * 16 + kq * 4]) = acc[jt];
    __syncthreads();
    // 16 tokens x 16 pieces of 8 ranks: one 16-byte store per thread, the waves' partial sums added in wave order
    const int tok = tid >> 4, j8 = (tid & 15) * 8;
    if (j8 >= rp || tl.row[tok] < 0) return;
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = red[0][tok][j8 + i];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w)
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += red[w][tok][j8 + i];
    *reinterpret_cast<uint4*>(t + ((int64_t)blockIdx.x * 16 + tok) * LORA_MAX_RANK + j8) = pack8(s);
}

// the four 16-column tiles of a wave for a rank of NKS steps of 32: all B fragments are requested before the first MFMA; tiles past N
// (i >= nt) re-read the wave's first tile and store nothing
template <int NKS>
__device__ __forceinline__ void lora_expand_tiles(const uint16_t* __restrict__ b, int rp, int nbase, int nt, int l15, int kq, const h8* tf, f4* acc) {
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    h8 bv[4][NKS];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint16_t* bp = b + (int64_t)(nbase + (i < nt ? i : 0) * 16 + l15) * rp + kq * 8;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) bv[i][ks] = ks * 32 + kq * 8 < rp ? load_h8(bp + ks * 32) : zero;   // (the half step of rp % 32 == 16)
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bv[i][ks], tf[ks], acc[i], 0, 0, 0);
}

__global__ __launch_bounds__(4 * WAVE) void lora_expand_kernel(const LoraTile* __restrict__ tiles, const LoraSlot* __restrict__ slots,
                                                               const uint16_t* __restrict__ t, uint16_t* __restrict__ y, int64_t ldy, int N,
                                                               int vec) {
    const LoraTile& tl = tiles[blockIdx.x];
    const LoraSlot sl = slots[tl.slot];
    if (!sl.b) return;
    const int rp = sl.rp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
    const int row = tl.row[l15];
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    // the tile's t rows, rounded to fp16 by the shrink kernel: rank steps of 32, the half step of rp % 32 == 16 masked
    h8 tf[LORA_MAX_RANK / 32];
    const uint16_t* tp = t + ((int64_t)blockIdx.x * 16 + l15) * LORA_MAX_RANK + kq * 8;
#pragma unroll
    for (int ks = 0; ks < LORA_MAX_RANK / 32; ++ks) tf[ks] = (row >= 0 && ks * 32 + kq * 8 < rp) ? load_h8(tp + ks * 32) : zero;
    const int nbase = blockIdx.y * LORA_EXPAND_COLS + wave * 64;
    if (nbase >= N) return;   // (wave-uniform; N % 16 == 0: a tile is inside or outside as a whole)
    const int nt = (N - nbase) / 16 < 4 ? (N - nbase) / 16 : 4;
    f4 accs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) accs[i] = f4{0.f, 0.f, 0.f, 0.f};
    switch ((rp + 31) / 32) {   // (block-uniform)
        case 1: lora_expand_tiles<1>(sl.b, rp, nbase, nt, l15, kq, tf, accs); break;
        case 2: lora_expand_tiles<2>(sl.b, rp, nbase, nt, l15, kq, tf, accs); break;
        case 3: lora_expand_tiles<3>(sl.b, rp, nbase, nt, l15, kq, tf, accs); break;
        default: lora_expand_tiles<4>(sl.b, rp, nbase, nt, l15, kq, tf, accs); break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= nt) break;
        const int n0 = nbase + i * 16;
        const f4 acc = accs[i];
        if (row < 0) continue;
        uint16_t* yp = y + (int64_t)row * ldy + n0 + kq * 4;
        if (vec) {
            const h4 y0 = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(yp));
            h4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = to_h((float)y0[r] + sl.scale * acc[r]);
            *reinterpret_cast<uint2*>(yp) = __builtin_bit_cast(uint2, o);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) yp[r] = f2h(h2f(yp[r]) + sl.scale * acc[r]);
        }
    }
}

}  // namespace

hipError_t launch_lora(hipStream_t s, const LoraTile* tiles, int ntiles, const LoraSlot* slots, const uint16_t* x, int64_t ldx, uint16_t* y,
                       int64_t ldy, int N, int K, uint16_t* t) {
    if (ntiles <= 0) return hipSuccess;
    if (K <= 0 || K % 32 || N <= 0 || N % 16 || ldx < K || ldx % 8 || ldy < N || ((uintptr_t)x & 15) || ((uintptr_t)t & 15) || ((uintptr_t)y & 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lora_shrink_kernel, dim3((unsigned)ntiles), dim3(LORA_WAVES * WAVE), 0, s, tiles, slots, x, ldx, K, t);
    const int vec = ldy % 4 == 0 && ((uintptr_t)y & 7) == 0;   // 8-byte accesses of y
    hipLaunchKernelGGL(lora_expand_kernel, dim3((unsigned)ntiles, (unsigned)((N + LORA_EXPAND_COLS - 1) / LORA_EXPAND_COLS)), dim3(4 * WAVE), 0,
                       s, tiles, slots, t, y, ldy, N, vec);
    return hipGetLastError();
}

}  // namespace pplhip
