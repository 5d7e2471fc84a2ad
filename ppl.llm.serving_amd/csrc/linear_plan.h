// The launch plan of the weight-only linear layers: what launch_linear (k_gemm.hip) runs for a problem, decided WITHOUT launching.
//   launch_linear = validate -> plan_linear -> format_route (if asked) -> one switch on the family -> the split-K tail.
// Host only: no HIP header, no HIP call, nothing dereferenced -- tests/host/linear_plan_trace.cc builds it with the host compiler and checks
// every plan's invariants over the tests' sweep grid.  DESIGN.md has the table of families, conditions and where each threshold was measured.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "k_gemm_tiles.h"

namespace pplhip {

// Every switch the plan reads, with the compiled-in value as its default.  from_env() fills it once per process: the switches read
// through tune_int / tune_set only in a tuning build (make TUNING=1, k_tune.h), the two product switches always.
struct LinearTuning {
    // largest rest (M mod 1024) of a saturated step that is split off as a second launch (0: never); measured: rest 16 / 76 / 128 / 256
    // -13 / -10 / -11 / -5 %, 384 equal
    int msplit = 256;                    // PPLHIP_GEMM_MSPLIT
    bool no_skinny = false;              // PPLHIP_GEMM_NOSKINNY (set)
    bool force_generic = false;          // PPLHIP_GEMM_GENERIC (set)
    // the MFMA skinny kernel up to 3 rows; from 4 rows the half-height tile kernel (64 activation rows, split-K) is faster: 7B decode step at
    // batch 4 / 8 / 12 / 16 3.64 / 3.90 / 4.40 / 4.74 -> 3.56 / 3.73 / 3.81 / 4.18 ms (profiles/small_batch_latency.py)
    int gemv_max_m = 3;                  // PPLHIP_GEMV_MAX_M
    bool gemv_max_m_set = false;         //   ... was set: int8 weights with K % 128 == 0 then keep it instead of 2 rows
    // row limit of the streaming GEMV (product switch; < 0: 4 rows, 2 for int8 weights with K % 128 == 0 -- with 16-row activation sub-tiles
    // and one block per CU the half-height tile kernel overtakes the GEMV from 3 rows: 7B decode step at batch 2 / 3 / 4 / 5: GEMV 2.48 /
    // 2.75 / 3.00 / -, tiles - / see DESIGN.md / 2.68 / 2.74 ms)
    int gemv_stream_max_m = -1;          // PPLHIP_GEMV_STREAM_MAX_M
    int gemv_waves = 0;                  // PPLHIP_GEMV_WAVES (0: 8 K slices up to 1024 row tiles, else 4; profiles/gemm_microbench.py)
    // W4 producer / consumer kernel (product switch; 0: the ring kernel for everything, A/B runs): measured in the step, 12.70 -> 12.49 ms
    // (profiles/r05_w4_pc_experiments.md)
    int pc_mode = 1;                     // PPLHIP_GEMM_PC
    int wide = 1;                        // PPLHIP_GEMM_WIDE (0: never; 2: experiments -- every eligible shape, any M)
    // measured (7B layer): M = 3584 1435 vs 1501 us, 3072 1277 vs 1264, 2560 equal, 2048 941 vs 851
    int min_m256 = 3584;                 // PPLHIP_GEMM_256_MIN_M
    int gm256 = 0, gn256 = 0;            // PPLHIP_GEMM256_GM / _GN (0: 4 x 8)
    bool direct_epilogue = false;        // PPLHIP_GEMM_DIRECT_EPILOGUE (set; A/B runs)
    // measured (profiles/gemm_microbench.py, M = 1024): weight tiles per XCD (order 0) beats activation slices per XCD (order 1) by 2-4 %
    // on every layer shape
    int map = -1;                        // PPLHIP_GEMM_MAP
    bool gm128_set = false;              // PPLHIP_GEMM128_GM (set): super-tiles at M <= 1024 too (experiments)
    int gm128 = 0, gn128 = 0;            // PPLHIP_GEMM128_GM / _GN (0: 8 x 12)
    int ablate = 0;                      // PPLHIP_GEMM_ABLATE (diagnosis only: wrong results)
    int stages = 0;                      // PPLHIP_GEMM_STAGES (2..4 forces the ring depth)
    int splitk = 0;                      // PPLHIP_GEMM_SPLITK (> 0 forces the slab count)
    int minkt = 0;                       // PPLHIP_GEMM_MINKT (0: 16 / 28 K tiles per split; M = 64 / 256 on the 70B/TP8 shapes, M = 1024 on 7B/TP8 slices)
    // K slabs: two stages when several blocks share a CU; a launch of at most one block per CU keeps the deep ring (the LDS is free anyway):
    // W8 7B at M = 256 wo 21.3 -> 19.8 us, w2 38.8 -> 33.4; 13B / TP2 at M = 512 wo 28.0 -> 24.3, w2 56.8 -> 52.1; fp16 70B / TP8 w2 30.0 ->
    // 26.0; W4 70B / TP8 w2 31.1 -> 30.1 (profiles/r04_splitk_stages_sweep.log).  W4 half-height tiles at M <= 64 are the exception: w2 of
    // the 70B / TP8 slice 19.4 -> 21.0 us with the deep ring.  In the steps: 7B / TP8 slice at 1024 rows 7.97 -> 7.69 ms, config 4 per rank
    // 13.68 -> 13.54, 7B TP 1 at batch 160-512 -0.3..-1.9 % (r04_split_deep_ab.log)
    int split_deep = 1;                  // PPLHIP_GEMM_SPLIT_DEEP (0: always two stages)
    // at most one block per CU (<= 256 blocks): 8 waves, 4 of them producers (wo 59 -> 46 us, w2 120 -> 95 us at M = 1024); W8 with a deep
    // ring and no slabs: eight consumer waves, each group one k-step of a tile (w2 at M = 1024: 100 -> 96 us)
    int wl = 0;                          // PPLHIP_GEMM_WL (1 / 5 / 6)
    int half = -1;                       // PPLHIP_GEMM_HALF (7B layer GEMMs at M = 64: 102 -> 84 us, M = 32: 90 -> 74 us)
    int half128 = 1;                     // PPLHIP_GEMM_HALF128 (0: off; 2: always 64-row sub-tiles)
    // 64 < M <= 128 with 80- .. 128-row sub-tiles for the shapes that need split-K anyway (7B at M = 128, HBM-cold: wqkv 33.1 -> 29.3 us, wo
    // 21.2 -> 18.9, w2 27.9 -> 26.3; w13 -- 172 tiles, no split -- stays on the ring kernel above 80 rows: 34.7 against 42.0 us at 128).
    // Decode step at batch 72 / 96 / 128 6.20 / 6.85 / 7.92 -> 5.70 / 6.53 / 7.76 ms
    int half128_max_m = 128;             // PPLHIP_GEMM_HALF128_MAX_M (64: off)
    // split-K slabs: ONE block per CU, not three.  A slab costs 8 M N bytes (written here, read by the reduce or the consuming kernel)
    // against N K / splits weight bytes.  Measured on the 7B shapes, HBM-cold (profiles/r04_splitk_sweep.log): w13 at M = 64 with 5 / 1 slabs
    // 37.6 / 29.9 us (and no reduce kernel), wqkv 6 / 2 slabs 25.1 / 20.7 us; wo / w2 (32 tiles) keep 8
    int half128_blocks = 256;            // PPLHIP_GEMM_HALF128_BLOCKS
    int half128_unsplit_max_m = 80;      // PPLHIP_GEMM_HALF128_UNSPLIT_MAX_M (w13: 80-row sub-tile 31.0-31.6 vs 32.4-32.6 us at M = 72-80, 96 rows 34.4 vs 33.1)
    int w4_sc16 = 1;                     // PPLHIP_GEMM_W4_SC16 (W4 slabs of <= 32 K tiles: 4 KiB of scales, three blocks per CU)
    static LinearTuning from_env();
};

struct LinearProblem {
    int wq_bit = 0, group = 0;
    int64_t M = 0;
    int N = 0, K = 0;
    int64_t ldy = 0;
    int epi = EPI_F16;
    size_t ws_bytes = 0;          // split-K workspace (0: none)
    bool accept_defer = false;    // the caller takes unreduced slabs (SplitSlabs)
    uintptr_t x = 0, w = 0, scale = 0, y = 0;   // only their alignment is used
};

enum LinearFamily { LF_GEMV_STREAM, LF_GEMV, LF_W4_PC, LF_W8_WIDE, LF_W8_256, LF_W8_HALF128, LF_RING, LF_GENERIC };
enum LinearReduce { LR_NONE, LR_KERNEL, LR_DEFERRED };
// Tile order of a launch.  order 1 (m_tiles % 8 == 0): XCD x owns the activation row-tiles m == x (mod 8); order 0: XCD x owns weight tiles
// n == x (mod 8), walked plainly (gm == 0) or in super-tiles of gn (n) x gm (m).  ablate: PPLHIP_GEMM_ABLATE.  The ring kernel takes it as
// one int (a struct argument costs it 7-9 instructions): map_pack on the host, map_unpack in gemm_dma_body, and nowhere else.
struct MapMode { uint8_t order, ablate, gm, gn; };
constexpr int map_pack(MapMode m) { return (int)(m.order | (unsigned)m.ablate << 8 | (unsigned)m.gm << 16 | (unsigned)m.gn << 24); }
constexpr MapMode map_unpack(int v) { return MapMode{(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)}; }

// One launch.  Template arguments by family:
//   LF_GEMV_STREAM <wq, rows = M, epi, nw>        LF_GEMV <wq, 1, epi, nw>         LF_W4_PC <epi>          LF_W8_WIDE <epi, stages, nc>
//   LF_W8_256 <epi>        LF_W8_HALF128 <epi, stages, bm>        LF_RING <wq, epi, stages, wl, bm, maxg>        LF_GENERIC <wq, epi>
struct LinearPart {
    int64_t m0 = 0, M = 0;        // rows [m0, m0 + M) of the problem
    LinearFamily family = LF_GENERIC;
    int wq = 0, epi = EPI_F16, stages = 0, wl = 0, bm = 0, maxg = 0, nw = 0, nc = 0;
    unsigned grid_x = 0, grid_y = 1, threads = 0;
    size_t lds = 0;               // dynamic LDS bytes
    int bn = 0;                   // weight rows / activation rows (bm) of a block tile
    int n_tiles = 0, m_tiles = 0, splits = 1, kt_per = 0, kt_depth = 0;   // K tiles per split, k per K tile
    MapMode map = {0, 0, 0, 0};   // gm != 0: super-tiles
    int staged = 0;               // LF_W8_256: the output goes through LDS
    LinearReduce reduce = LR_NONE;
    int nwk_log2 = 0, npw = 0, nb = 0;   // LF_GEMV_STREAM: waves along K, pieces per wave and row, 8-row batches per wave
};

struct LinearPlan {
    bool ok = false;              // false: no kernel takes the problem (an argument error)
    int n_parts = 0;              // 2: the M-split of a saturated step
    LinearPart part[2];
};

// the argument rules of launch_linear (M > 0): formats, N and ldy multiples of 4, K a multiple of the format's 16-byte load
bool linear_problem_valid(const LinearProblem& p);
LinearPlan plan_linear(const LinearProblem& p, const LinearTuning& t);
// the parts a sub-launcher plans for itself (launch_gemv_stream, launch_linear_w4_pc, launch_linear_w8_wide); ok false: not its shape
bool plan_gemv_stream(int wq_bit, int64_t M, int N, int K, int epi, LinearPart* part);
bool plan_w4_pc(int64_t M, int N, int epi, LinearPart* part);
bool plan_w8_wide(int64_t M, int N, int epi, int nc, LinearPart* part);

// route text of a part ("kernel=<template<args>> splits= [kchunk=] reduce= order= ...") / of a plan (parts joined by " ; "); returns the length
int format_route(const LinearPart& part, char* buf, int cap);
int format_route(const LinearPlan& plan, char* buf, int cap);

// ---- the quantised-activation linears (launch_linear_i8 / launch_linear_f8, k_gemm_i8.hip): the same seam ------------------------------------
//   launch_linear_q8 = validate -> plan_linear_q8 -> format_route (if asked) -> one switch on the family -> launch.
// The switches it reads (a tuning build only, k_tune.h), with the compiled-in values as defaults; from_env() fills them once per process.
struct Q8Tuning {
    bool force_generic = false;   // PPLHIP_GEMM_GENERIC (set): the skinny / generic kernel for every shape
    // 256 x 256 blocks from this many rows (int8 only); measured: M = 4096 layer 888 us (1.87 POP/s) vs 1110, M = 2048 554 vs 459 us
    int min_m256 = 4096;          // PPLHIP_GEMM_I8_256_MIN_M
    int st256 = 4;                // PPLHIP_GEMM_I8_256_ST (3: a three-stage ring; any other value: four)
    int gm256 = 0, gn256 = 0;     // PPLHIP_GEMM256_GM / _GN (0: 4 x 8)
    int wide = 1;                 // PPLHIP_GEMM_I8_WIDE (0: never the 128 x 384 blocks)
    // ring depth of the 128 x 128 producer / consumer blocks: 3 / 4 force it, any other value >= 0 runs two stages; < 0: four stages for
    // launches of <= 256 tiles, else two
    int pc = -1;                  // PPLHIP_GEMM_I8_PC
    static Q8Tuning from_env();
};

enum Q8Family { QF_GEMV, QF_PC, QF_WIDE, QF_256 };
// One launch.  Template arguments by family (FMT: i8 / f8):
//   QF_GEMV gemv_i8_kernel<mt, epi, nw, FMT>     QF_PC gemm_i8_pc_kernel<epi, stages, FMT>     QF_WIDE gemm_i8_wide_kernel<epi, FMT>
//   QF_256 gemm_i8_256_kernel<epi, stages> (int8 only)
struct Q8Plan {
    bool ok = false;              // false: no kernel takes the problem (an argument error)
    Q8Family family = QF_GEMV;
    bool f8 = false;
    int epi = EPI_F16, stages = 0, mt = 0, nw = 0;   // mt: 16-row activation tiles per block of the skinny kernel
    unsigned grid_x = 0, grid_y = 1, threads = 0;
    size_t lds = 0;               // dynamic LDS bytes
    int bn = 0, bm = 0, bk = 0;   // weight rows / activation rows / k of a block tile (bk 0: the waves split K)
    int n_tiles = 0, m_tiles = 0;
    int gn = 0, gm = 0;           // QF_256: super-tiles of gn (n) x gm (m) tiles
};
// the argument rules of launch_linear_i8 / _f8 (M > 0): N and ldy multiples of 4, K a multiple of the 16-byte load, no fp32 SwiGLU
bool linear_q8_valid(int64_t M, int N, int K, int64_t ldy, int epi);
Q8Plan plan_linear_q8(bool f8, int64_t M, int N, int K, int64_t ldy, int epi, const Q8Tuning& t);
// "kernel=<template<args>> grid= threads= lds= n_tiles= m_tiles= [order=super(gm x gn)]"; returns the length
int format_route(const Q8Plan& plan, char* buf, int cap);

// largest M the streaming GEMV takes for this shape (0: none); env_max_m: LinearTuning::gemv_stream_max_m
int gemv_stream_max_m(int wq_bit, int group, int N, int K, int env_max_m);
// 12 consumer waves when the 128 x 384 tiles fill whole rounds of 256 one-per-CU blocks well enough, else 0
int linear_w8_wide_waves(int64_t M, int N);
// Shapes gemm_w4_pc_kernel takes: int4 weights in groups of 128, K % 128 == 0, N % 4 == 0 (N % 16 == 0 with the fused SwiGLU), 16-byte
// aligned output rows, 32-bit byte offsets inside x and w
bool linear_w4_pc_supported(int group, int64_t M, int N, int K, uintptr_t x, uintptr_t w, uintptr_t scale, uintptr_t y, int64_t ldy, int epi);

}  // namespace pplhip
