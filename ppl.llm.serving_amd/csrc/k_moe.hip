// Mixture-of-experts feed-forward block (Mixtral): router, bucketing, the two grouped GEMMs and the combine.  Numerics: DESIGN.md section 2;
// the kernels' budget and tile order: DESIGN.md section 4.
//
//   moe_route_kernel    one wave per token: E router logits (fp32), k rounds of wave arg-max, softmax over the k winners, per-expert counts
//   moe_bucket_kernel   one block: counts -> padded row ranges and the m-tile table, stable placement of every (token, slot) pair
//   moe_gemm_kernel     ONE launch for all experts on a fixed grid: a block reads the live-tile count and its tile from device memory;
//                       w13 gathers its activation rows through the sorted row list and writes h in sorted order, w2 reads h contiguously,
//                       scales by the routing weight and scatters fp32 rows to y_slots[token k + slot]
//   moe_combine_kernel  fp16(sum of a token's k slot rows, in slot order)
// No floating-point atomics and no host synchronisation: the step stays capturable, and a call repeated gives the same bits.
#include "k_gemm_dev.h"

namespace pplhip {

namespace {

constexpr int MOE_ST = 3;          // ring stages of the grouped GEMM (prefetch distance 2)
constexpr int EPI_SCALED = 3;      // w2's epilogue: fp32 rows times the routing weight, scattered to y_slots
constexpr int BUCKET_NT = 1024;    // threads of the one bucket block (16 waves)

struct MoeTile {                   // one m-tile of the grouped GEMMs: rows [row0, row0 + valid) of the sorted order belong to `expert`
    int32_t expert, row0, valid, pad;
};

// What a call keeps in its workspace.  rows / tiles bound the padded sorted order for EITHER tile height (every expert's range is padded up
// to a multiple of BM <= 128 rows, and the shortest tile has 32), so the layout of a step does not depend on the height it runs with.
struct MoeLayout {
    size_t counts, live, ids, weights, sorted, inv, tiles, h, y, bytes;
    int64_t rows_cap, tiles_cap;
};
MoeLayout moe_layout(int64_t T, int E, int k, int hidden, int inter_p) {
    MoeLayout l;
    const int64_t pairs = T * k;
    l.rows_cap = pairs + (int64_t)(E + 1) * 128;
    l.tiles_cap = (pairs + (int64_t)E * 31) / 32 + 1;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    l.counts = take(64 * 4);
    l.live = take(4);
    l.ids = take((size_t)pairs * 4);
    l.weights = take((size_t)pairs * 4);
    l.sorted = take((size_t)l.rows_cap * 4);
    l.inv = take((size_t)pairs * 4);
    l.tiles = take((size_t)l.tiles_cap * sizeof(MoeTile));
    l.h = take((size_t)l.rows_cap * inter_p * 2);
    l.y = take((size_t)pairs * hidden * 4);
    l.bytes = at;
    return l;
}

__global__ void moe_clear_counts_kernel(int32_t* counts) { counts[threadIdx.x] = 0; }

// ---- router ------------------------------------------------------------------------------------------------------------------------
// r_e = sum_i x_i g_{e,i} in fp32: lane l multiplies the 16-byte pieces l, l + 64, ... of the row, the wave sum leaves r_e in lane e.
// Selection: k rounds of wave arg-max, ties to the lower expert; slot s lives in lane s.  p_s = exp(r_s - r_max) / sum over the k slots.
__global__ __launch_bounds__(256) void moe_route_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ gate, int64_t T, int hidden,
                                                        int E, int k, int32_t* __restrict__ ids, float* __restrict__ weights,
                                                        int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;   // (wave-uniform)
    const uint16_t* xr = x + t * hidden;
    float v = -INFINITY;
    for (int e = 0; e < E; ++e) {
        const uint16_t* g = gate + (int64_t)e * hidden;
        float acc = 0.f;
        for (int i = lane * 8; i < hidden; i += 64 * 8) {
            float a[8], b[8];
            unpack8(*reinterpret_cast<const uint4*>(xr + i), a);
            unpack8(*reinterpret_cast<const uint4*>(g + i), b);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(a[j], b[j], acc);
        }
        acc = wave_sum(acc);
        if (lane == e) v = acc;
    }
    float sel_v = 0.f;
    int sel_e = 0;
    for (int s = 0; s < k; ++s) {
        float bv = v;
        int be = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oe = __shfl_xor(be, o, 64);
            if (ov > bv || (ov == bv && oe < be)) { bv = ov; be = oe; }
        }
        if (lane == s) { sel_v = bv; sel_e = be < E ? be : E - 1; }   // (be >= E only for logits that are not numbers)
        if (lane == be) v = -INFINITY;
    }
    const float rmax = __shfl(sel_v, 0, 64);
    const float ex = lane < k ? expf(sel_v - rmax) : 0.f;
    float sum = 0.f;
    for (int s = 0; s < k; ++s) sum += __shfl(ex, s, 64);
    if (lane < k) {
        ids[t * k + lane] = sel_e;
        weights[t * k + lane] = ex / sum;
        atomicAdd(&counts[sel_e], 1);
    }
}

// ---- buckets -----------------------------------------------------------------------------------------------------------------------
// Expert e owns the sorted rows [row0_e, row0_e + count_e), row0 = exclusive scan of the counts padded up to BM; its m-tiles follow each
// other in the table, so experts nobody chose cost no tile.  Placement is stable: pair p = token k + slot goes behind every pair p' < p of
// the same expert.  The block walks the pairs 1024 at a time; inside a wave a pair's rank among its expert's pairs comes from peeling the
// wave's distinct experts with ballots, across waves from the per-wave counts in LDS.  Rows [count_e, padded) name the expert's first
// pair: the GEMMs read them like any row and store nothing for them.
__global__ __launch_bounds__(BUCKET_NT) void moe_bucket_kernel(const int32_t* __restrict__ ids, int n_pairs, int E, int BM,
                                                               int32_t* __restrict__ counts, int32_t* __restrict__ live,
                                                               MoeTile* __restrict__ tiles, int32_t* sorted, int32_t* __restrict__ inv,
                                                               int rows_cap, int tiles_cap) {
    __shared__ int32_t cnt[64], row0[64], tile0[64], run[64], wcnt[BUCKET_NT / 64][64], n_tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {
        cnt[tid] = tid < E ? counts[tid] : 0;
        run[tid] = 0;
        counts[tid] = 0;   // for the next layer's router
    }
    __syncthreads();
    if (tid == 0) {
        int r = 0, nt = 0;
        for (int e = 0; e < E; ++e) {
            const int te = (cnt[e] + BM - 1) / BM;
            row0[e] = r;
            tile0[e] = nt;
            r += te * BM;
            nt += te;
        }
        n_tiles = nt < tiles_cap ? nt : tiles_cap;
        *live = n_tiles;
    }
    __syncthreads();
    if (tid < E) {
        for (int i = 0, c = cnt[tid]; i * BM < c; ++i) {
            if (tile0[tid] + i >= tiles_cap) break;
            tiles[tile0[tid] + i] = MoeTile{tid, row0[tid] + i * BM, c - i * BM < BM ? c - i * BM : BM, 0};
        }
    }
    for (int base = 0; base < n_pairs; base += BUCKET_NT) {
        wcnt[wave][lane] = 0;
        __syncthreads();
        const int p = base + tid;
        const int e = p < n_pairs ? ids[p] : -1;
        int rank = 0;
        uint64_t todo = __ballot(e >= 0);
        while (todo) {   // (wave-uniform) one round per distinct expert of the wave
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const int el = __shfl(e, lead, 64);
            const uint64_t m = __ballot(e == el);
            if (e == el) rank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == lead) wcnt[wave][el] = __popcll(m);
            todo &= ~m;
        }
        __syncthreads();
        if (e >= 0) {
            int off = run[e] + rank;
            for (int w = 0; w < wave; ++w) off += wcnt[w][e];
            const int r = row0[e] + off;
            if (r < rows_cap) { sorted[r] = p; inv[p] = r; }
        }
        __syncthreads();
        if (tid < E) {
            int s = 0;
            for (int w = 0; w < BUCKET_NT / 64; ++w) s += wcnt[w][tid];
            run[tid] += s;
        }
        __syncthreads();
    }
    __syncthreads();   // every placement is written (n_pairs == 0: the tile table is)
    for (int i = tid; i < n_tiles * BM; i += BUCKET_NT) {
        const MoeTile t = tiles[i / BM];
        const int j = i % BM;
        if (j >= t.valid && t.row0 + j < rows_cap)
            sorted[t.row0 + j] = __hip_atomic_load(&sorted[t.row0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (another wave wrote it)
    }
}

// ---- grouped GEMM ------------------------------------------------------------------------------------------------------------------
// The ring of the dense 128 x 128 x 64 tile kernel (k_gemm_dev.h: LDS-DMA of both operands, swizzled on the source side, int8 weights
// converted in registers, mfma_f32_16x16x32_f16; 4 waves of 32 weight rows x BM activation rows), with three differences: the weight tile
// comes from the tile's expert, every lane's activation address comes from the sorted row list (w13) or the sorted order itself (w2), and
// the grid is fixed -- max_m_tiles is the host's bound, the live count is read here.
// (The ring, the source swizzle, the fragment reads and the W8 conversion are a COPY of gemm_dma_body's WL 1 form -- the dense body takes one
// weight matrix and contiguous rows and is measured instruction by instruction, so it is not parametrised for this: a change to either is
// made in both.)
// Tile order: block b runs on XCD b % 8, which owns the weight column tiles nt == b % 8 (mod 8) and walks, for each of them, all m-tiles.
// The table lists an expert's m-tiles one behind the other, so the m-tiles of one (expert, nt) follow each other on ONE XCD and its L2
// serves that weight tile to all of them: every expert's weights leave HBM once.
template <int WQ, int EPI, int BM>
__global__ __launch_bounds__(256) void moe_gemm_kernel(const uint16_t* __restrict__ x, int64_t ldx, const void* __restrict__ wv, int64_t w_stride,
                                                       const uint16_t* __restrict__ scale, int N, int K, int k_top,
                                                       const int32_t* __restrict__ live, const MoeTile* __restrict__ tiles,
                                                       const int32_t* __restrict__ sorted, const float* __restrict__ weights,
                                                       void* __restrict__ yv, int64_t ldy, int n_tiles, int max_m_tiles) {
    extern __shared__ __attribute__((aligned(16))) char moe_smem[];   // MOE_ST x X, then MOE_ST x W
    constexpr int WB2 = WQ == 8 ? 2 : 4;                  // half-bytes per weight element
    constexpr int W_STAGE = G_BN * G_BK * WB2 / 2;        // 8 KiB (int8) / 16 KiB (fp16)
    constexpr int X_STAGE = BM * G_BK * 2;                // 16 KiB / 4 KiB
    constexpr int NT = 256;
    constexpr int X_DMA = X_STAGE / (NT * 16), W_DMA = W_STAGE / (NT * 16);
    static_assert(BM == 128 || BM == 32, "tile heights");
    static_assert(WQ == 0 || WQ == 8, "fp16 or W8A16");

    const XcdSlot b = xcd_slot((int)blockIdx.x);
    int q, mt;
    walk_plain(b.slot, max_m_tiles, q, mt);
    const int nt = b.xcd + 8 * q;
    if (nt >= n_tiles || mt >= *live) return;
    const MoeTile tile = tiles[mt];
    const int n0 = nt * G_BN;
    const char* w = reinterpret_cast<const char*>(wv) + (int64_t)tile.expert * w_stride;
    const uint16_t* sc = scale ? scale + (int64_t)tile.expert * N : nullptr;

    uint16_t* const Xs0 = reinterpret_cast<uint16_t*>(moe_smem);
    char* const Wq0 = moe_smem + MOE_ST * X_STAGE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    constexpr int NI = 2, NJ = BM / 16;
    const int nb = wave * (NI * 16);

    const uint16_t* xsrc[X_DMA];
    const char* wsrc[W_DMA];
#pragma unroll
    for (int j = 0; j < X_DMA; ++j) {   // (the chunk order of a row: gemm_dma_body)
        const int p = j * NT + tid, row = p >> 3, pos = (p & 7) ^ ((row >> 1) & 7);
        const int c = ((pos & 3) << 1) | (pos >> 2);
        int64_t src = tile.row0 + row;                                    // w2: h is in sorted order
        if constexpr (EPI == EPI_SWIGLU) src = sorted[src] / k_top;       // w13: the pair's token row, gathered
        xsrc[j] = x + src * ldx + c * 8;
    }
#pragma unroll
    for (int j = 0; j < W_DMA; ++j) {
        const int p = j * NT + tid;
        if constexpr (WQ == 8) {
            const int row = p >> 2, c = (p & 3) ^ w_swz(row);
            int n = n0 + row;
            if (n >= N) n = N - 1;
            wsrc[j] = w + (int64_t)n * K + c * 16;
        } else {
            const int row = p >> 3, pos = (p & 7) ^ ((row >> 1) & 7);
            const int c = ((pos & 3) << 1) | (pos >> 2);
            int n = n0 + row;
            if (n >= N) n = N - 1;
            wsrc[j] = w + ((int64_t)n * K + c * 8) * 2;
        }
    }
    const uint32_t xdst = __builtin_amdgcn_readfirstlane(lds_addr(Xs0) + wave * 1024);
    const uint32_t wdst = __builtin_amdgcn_readfirstlane(lds_addr(Wq0) + wave * 1024);
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int j = 0; j < X_DMA; ++j) glds16(xsrc[j] + k0, xdst + stage * X_STAGE + j * (NT * 16));
#pragma unroll
        for (int j = 0; j < W_DMA; ++j) glds16(wsrc[j] + k0 * WB2 / 2, wdst + stage * W_STAGE + j * (NT * 16));
    };

    f4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    constexpr int D = MOE_ST - 1;
    const int ktiles = K / G_BK;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < ktiles) issue(d, d * G_BK);
    int st = 0, stn = D;
    for (int t = 0; t < ktiles; ++t) {
        ring_wait<X_DMA + W_DMA>((ktiles - 1 - t) < (D - 1) ? (ktiles - 1 - t) : (D - 1));
        __syncthreads();   // tile t is published; the stage read during iteration t - 1 is free
        if (t + D < ktiles) issue(stn, (t + D) * G_BK);
        const uint16_t* xs = Xs0 + st * (BM * G_BK);
        const char* wq = Wq0 + st * W_STAGE;
        st = st == MOE_ST - 1 ? 0 : st + 1;
        stn = stn == MOE_ST - 1 ? 0 : stn + 1;
        uint4 wraw[NI];
        if constexpr (WQ == 8) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int row = nb + i * 16 + l15;
                wraw[i] = *reinterpret_cast<const uint4*>(&wq[row * G_BK + (kq ^ w_swz(row)) * 16]);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            h8 a[NI], bfr[NJ];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if constexpr (WQ == 8) {
                    a[i] = cvt_i8x8_f16(ks == 0 ? make_uint2(wraw[i].x, wraw[i].y) : make_uint2(wraw[i].z, wraw[i].w));
                } else {
                    const int row = nb + i * 16 + l15;
                    a[i] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&wq[(row * G_BK + g_swz(row, ks * 4 + kq) * 8) * 2]));
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int row = j * 16 + l15;
                bfr[j] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(&xs[row * G_BK + g_swz(row, ks * 4 + kq) * 8]));
            }
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }

#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int n = n0 + nb + i * 16 + kq * 4;
        if (n >= N) {
            // w13: the columns of h between inter and its padded row stride are w2's zero-padded K range -- zeros, not what the buffer held
            if constexpr (EPI == EPI_SWIGLU) {
                if ((n >> 1) < ldy) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int r = j * 16 + l15;
                        if (r < tile.valid) *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(yv) + (int64_t)(tile.row0 + r) * ldy + (n >> 1)) = 0u;
                    }
                }
            }
            continue;
        }
        h4 sh = {(_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f};
        if constexpr (WQ == 8) sh = __builtin_bit_cast(h4, *reinterpret_cast<const uint2*>(sc + n));
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int r = j * 16 + l15;
            if (r >= tile.valid) continue;
            const float v0 = acc[i][j][0] * (float)sh[0], v1 = acc[i][j][1] * (float)sh[1], v2 = acc[i][j][2] * (float)sh[2],
                        v3 = acc[i][j][3] * (float)sh[3];
            if constexpr (EPI == EPI_SWIGLU) {
                store4<EPI_SWIGLU>(yv, ldy, tile.row0 + r, n, v0, v1, v2, v3);
            } else {
                const int pair = sorted[tile.row0 + r];
                const float p = weights[pair];
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(yv) + (int64_t)pair * ldy + n) = make_float4(v0 * p, v1 * p, v2 * p, v3 * p);
            }
        }
    }
}

// ---- combine -----------------------------------------------------------------------------------------------------------------------
// out[t] = fp16(y_slots[t k] + y_slots[t k + 1] + ...): fp32, slot order, one rounding; a thread owns 8 columns of a token
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y_slots, int64_t T, int hidden, int k, uint16_t* __restrict__ out,
                                                          int64_t ldo) {
    const int per_row = hidden / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * per_row) return;
    const int64_t t = i / per_row;
    const int c = (int)(i - t * per_row) * 8;
    float acc[8];
    for (int s = 0; s < k; ++s) {
        const float* row = y_slots + (t * k + s) * hidden + c;
        const float4 a = *reinterpret_cast<const float4*>(row), b = *reinterpret_cast<const float4*>(row + 4);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = s == 0 ? v[j] : acc[j] + v[j];
    }
    *reinterpret_cast<uint4*>(out + t * ldo + c) = pack8(acc);
}

constexpr int moe_lds_bytes(int wq, int bm) { return MOE_ST * (bm * G_BK * 2 + G_BN * G_BK * (wq == 8 ? 1 : 2)); }

template <int EPI>
hipError_t launch_moe_gemm(hipStream_t s, int wq, int bm, const uint16_t* x, int64_t ldx, const void* w, int64_t w_stride, const uint16_t* scale, int N,
                           int K, int k_top, const int32_t* live, const MoeTile* tiles, const int32_t* sorted, const float* weights, void* y,
                           int64_t ldy, int n_tiles, int max_m_tiles) {
    const int64_t blocks = (int64_t)((n_tiles + 7) / 8 * 8) * max_m_tiles;
    if (blocks <= 0 || blocks > 0x7fffffff) return hipErrorInvalidValue;   // (a 1-D grid)
    const unsigned grid = (unsigned)blocks;
    dispatch_int<8, 0>(wq, [&](auto WQ) {
        dispatch_int<32, 128>(bm, [&](auto BM) {
            static LdsOptIn once;
            if (once.first()) set_max_lds(moe_lds_bytes(WQ, BM), moe_gemm_kernel<WQ, EPI, BM>);
            hipLaunchKernelGGL((moe_gemm_kernel<WQ, EPI, BM>), dim3(grid), dim3(256), moe_lds_bytes(WQ, BM), s, x, ldx, w, w_stride, scale, N, K, k_top,
                               live, tiles, sorted, weights, y, ldy, n_tiles, max_m_tiles);
        });
    });
    return hipGetLastError();
}

bool moe_shape_ok(int64_t T, int E, int k, int hidden) {
    return T >= 0 && T * k < ((int64_t)1 << 30) && E >= 1 && E <= MOE_MAX_EXPERTS && k >= 1 && k <= MOE_MAX_TOP_K && k <= E && hidden > 0 && hidden % 64 == 0;
}

}  // namespace

int moe_tile_rows(int64_t T, int k, int E) { return T * k <= (int64_t)32 * E ? 32 : 128; }

size_t moe_ffn_workspace_bytes(int64_t T, int E, int k, int hidden, int inter) {
    return moe_layout(T, E, k, hidden, (inter + 63) / 64 * 64).bytes;
}

hipError_t launch_moe_route(hipStream_t s, const uint16_t* x, const uint16_t* gate, int64_t T, int hidden, int E, int k, int32_t* ids,
                            float* weights, int32_t* counts, bool counts_clean) {
    if (!moe_shape_ok(T, E, k, hidden)) return hipErrorInvalidValue;
    if (!counts_clean) hipLaunchKernelGGL(moe_clear_counts_kernel, dim3(1), dim3(64), 0, s, counts);
    if (T > 0) hipLaunchKernelGGL(moe_route_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, x, gate, T, hidden, E, k, ids, weights, counts);
    return hipGetLastError();
}

hipError_t launch_moe_ffn(hipStream_t s, const uint16_t* x, const uint16_t* gate, const void* w13, const uint16_t* scale13, const void* w2,
                          const uint16_t* scale2, int wq_bit, int64_t T, int E, int k, int hidden, int inter, void* workspace, bool counts_clean,
                          uint16_t* y, int64_t ldy) {
    if (!moe_shape_ok(T, E, k, hidden) || (wq_bit != 0 && wq_bit != 8) || inter <= 0 || inter % 2) return hipErrorInvalidValue;
    if (T == 0) return hipSuccess;
    const int inter_p = (inter + 63) / 64 * 64;
    const MoeLayout l = moe_layout(T, E, k, hidden, inter_p);
    char* const ws = (char*)workspace;
    int32_t* const counts = (int32_t*)(ws + l.counts);
    int32_t* const live = (int32_t*)(ws + l.live);
    int32_t* const ids = (int32_t*)(ws + l.ids);
    float* const weights = (float*)(ws + l.weights);
    int32_t* const sorted = (int32_t*)(ws + l.sorted);
    MoeTile* const tiles = (MoeTile*)(ws + l.tiles);
    uint16_t* const h = (uint16_t*)(ws + l.h);
    float* const y_slots = (float*)(ws + l.y);
    const int bm = moe_tile_rows(T, k, E);
    const int max_m_tiles = (int)((T * k + (int64_t)E * (bm - 1) + bm - 1) / bm);
    const int64_t elt2 = wq_bit == 8 ? 2 : 4;   // half-bytes per weight element

    hipError_t e = launch_moe_route(s, x, gate, T, hidden, E, k, ids, weights, counts, counts_clean);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(moe_bucket_kernel, dim3(1), dim3(BUCKET_NT), 0, s, ids, (int)(T * k), E, bm, counts, live, tiles, sorted, (int32_t*)(ws + l.inv),
                       (int)l.rows_cap, (int)l.tiles_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // w13 covers the padded width of h, so that the columns past `inter` are written (zeros)
    e = launch_moe_gemm<EPI_SWIGLU>(s, wq_bit, bm, x, hidden, w13, (int64_t)2 * inter * hidden * elt2 / 2, scale13, 2 * inter, hidden, k, live, tiles, sorted,
                                    weights, h, inter_p, (2 * inter_p + G_BN - 1) / G_BN, max_m_tiles);
    if (e != hipSuccess) return e;
    e = launch_moe_gemm<EPI_SCALED>(s, wq_bit, bm, h, inter_p, w2, (int64_t)hidden * inter_p * elt2 / 2, scale2, hidden, inter_p, k, live, tiles, sorted,
                                    weights, y_slots, hidden, (hidden + G_BN - 1) / G_BN, max_m_tiles);
    if (e != hipSuccess) return e;
    const int64_t items = T * (hidden / 8);
    hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, y_slots, T, hidden, k, y, ldy);
    return hipGetLastError();
}

}  // namespace pplhip
