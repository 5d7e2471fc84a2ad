// plan_linear: which kernel runs a weight-only linear layer, on what grid, with which template arguments (linear_plan.h).  Pure functions of
// (LinearProblem, LinearTuning): no statics, no environment access outside LinearTuning::from_env, no HIP.
#include "linear_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include "k_tune.h"

namespace pplhip {

LinearTuning LinearTuning::from_env() {
    LinearTuning t;
    t.msplit = tune_int("PPLHIP_GEMM_MSPLIT", t.msplit);
    t.no_skinny = tune_set("PPLHIP_GEMM_NOSKINNY");
    t.force_generic = tune_set("PPLHIP_GEMM_GENERIC");
    t.gemv_max_m = tune_int("PPLHIP_GEMV_MAX_M", t.gemv_max_m);
    t.gemv_max_m_set = tune_set("PPLHIP_GEMV_MAX_M");
    if (const char* v = getenv("PPLHIP_GEMV_STREAM_MAX_M")) t.gemv_stream_max_m = atoi(v);
    t.gemv_waves = tune_int("PPLHIP_GEMV_WAVES", t.gemv_waves);
    if (const char* v = getenv("PPLHIP_GEMM_PC")) t.pc_mode = atoi(v);
    t.wide = tune_int("PPLHIP_GEMM_WIDE", t.wide);
    t.min_m256 = tune_int("PPLHIP_GEMM_256_MIN_M", t.min_m256);
    t.gm256 = tune_int("PPLHIP_GEMM256_GM", t.gm256);
    t.gn256 = tune_int("PPLHIP_GEMM256_GN", t.gn256);
    t.direct_epilogue = tune_set("PPLHIP_GEMM_DIRECT_EPILOGUE");
    t.map = tune_int("PPLHIP_GEMM_MAP", t.map);
    t.gm128_set = tune_set("PPLHIP_GEMM128_GM");
    t.gm128 = tune_int("PPLHIP_GEMM128_GM", t.gm128);
    t.gn128 = tune_int("PPLHIP_GEMM128_GN", t.gn128);
    t.ablate = tune_int("PPLHIP_GEMM_ABLATE", t.ablate);
    t.stages = tune_int("PPLHIP_GEMM_STAGES", t.stages);
    t.splitk = tune_int("PPLHIP_GEMM_SPLITK", t.splitk);
    t.minkt = tune_int("PPLHIP_GEMM_MINKT", t.minkt);
    t.split_deep = tune_int("PPLHIP_GEMM_SPLIT_DEEP", t.split_deep);
    t.wl = tune_int("PPLHIP_GEMM_WL", t.wl);
    t.half = tune_int("PPLHIP_GEMM_HALF", t.half);
    t.half128 = tune_int("PPLHIP_GEMM_HALF128", t.half128);
    t.half128_max_m = tune_int("PPLHIP_GEMM_HALF128_MAX_M", t.half128_max_m);
    t.half128_blocks = tune_int("PPLHIP_GEMM_HALF128_BLOCKS", t.half128_blocks);
    t.half128_unsplit_max_m = tune_int("PPLHIP_GEMM_HALF128_UNSPLIT_MAX_M", t.half128_unsplit_max_m);
    t.w4_sc16 = tune_int("PPLHIP_GEMM_W4_SC16", t.w4_sc16);
    return t;
}

int gemv_stream_max_m(int wq_bit, int group, int N, int K, int env_max_m) {
    const int max_m = env_max_m >= 0 ? env_max_m : (wq_bit == 8 && K % 128 == 0 ? 2 : 4);
    const int kl = wq_bit == 8 ? 16 : (wq_bit == 4 ? 32 : 8);
    if (K % kl) return 0;
    if (wq_bit == 4 && (group % 32 || K % group)) return 0;
    const int pieces = (K / kl + 63) / 64;
    if (pieces > 3 * GV_NW) return 0;  // at most three pieces per wave and row (K <= 24576 int8)
    (void)N;
    return max_m > 4 ? 4 : max_m;
}

// Narrower blocks were measured and lose: w13 at M = 1024 (N = 22016) with 11 consumer waves (504 blocks, two almost full rounds) 205-208 us
// against 191-194 us with 12 (464 blocks) -- the round time does not shrink with the tile.
int linear_w8_wide_waves(int64_t M, int N) {
    const int64_t m_tiles = (M + WD_BM - 1) / WD_BM;
    const int64_t tiles = (N + 383) / 384 * m_tiles, rounds = (tiles + 255) / 256;
    const double eff = (double)N * (double)M / ((double)rounds * 256.0 * 384.0 * WD_BM);
    // measured: with more than two rounds the 128 x 128 kernel catches up (w13 at M = 2048: 4 rounds 382 us against 367 us) unless the fit is exact
    return (eff >= 0.85 && (rounds <= 2 || eff >= 0.97)) ? 12 : 0;
}

bool linear_w4_pc_supported(int group, int64_t M, int N, int K, uintptr_t x, uintptr_t w, uintptr_t scale, uintptr_t y, int64_t ldy, int epi) {
    if (group != 128 || K % 128 || K < 128 || N % 4 || M < 1) return false;
    if (epi != EPI_F16 && epi != EPI_SWIGLU) return false;
    if (epi == EPI_SWIGLU && N % 16) return false;
    if (ldy % 8 || (y & 15)) return false;
    // the LDS-DMA fetches x and w in 16-byte pieces and the scale as the aligned dword around fp16 element n G + g
    if ((x & 15) || (w & 15) || (scale & 3)) return false;
    if ((uint64_t)M * (uint64_t)K * 2 >= (1ull << 32) || (uint64_t)N * (uint64_t)K / 2 >= (1ull << 32)) return false;
    if ((uint64_t)N * (uint64_t)(K / 128) >= (1ull << 30)) return false;
    return true;
}

// blocks of a grid whose XCD x = id % 8 owns the weight tiles n == x (mod 8): the weight tiles padded to 8
static unsigned xcd_grid(int n_tiles, int m_tiles) { return (unsigned)((n_tiles + 7) / 8 * 8 * m_tiles); }

bool plan_gemv_stream(int wq_bit, int64_t M, int N, int K, int epi, LinearPart* p) {
    const int kl = wq_bit == 8 ? 16 : (wq_bit == 4 ? 32 : 8);
    const int pieces = (K / kl + 63) / 64;
    int nwk_log2 = 0;
    while ((1 << nwk_log2) < pieces && nwk_log2 < 3) ++nwk_log2;
    const int nwk = 1 << nwk_log2, npw = (pieces + nwk - 1) / nwk;
    const int nw = nwk <= 4 ? 4 : 8;                                   // small blocks: the grid balances over the 256 CUs
    // 16 rows per wave when that still leaves >= 8 waves per CU, else 8
    const int64_t waves16 = (int64_t)((N + 15) / 16) * nwk;
    const int nb = waves16 >= 2048 ? 2 : 1;
    const int rows = (nw / nwk) * nb * GV_U;
    if (M < 1 || M > 4 || npw > 3) return false;
    if (wq_bit != 8 && wq_bit != 4 && wq_bit != 0) return false;
    p->family = LF_GEMV_STREAM;
    p->M = M, p->wq = wq_bit, p->epi = epi, p->nw = nw;
    p->bn = rows, p->bm = 4;
    p->n_tiles = (N + rows - 1) / rows, p->m_tiles = 1;
    p->grid_x = (unsigned)p->n_tiles, p->threads = (unsigned)nw * 64;
    p->nwk_log2 = nwk_log2, p->npw = npw, p->nb = nb;
    return true;
}

bool plan_w4_pc(int64_t M, int N, int epi, LinearPart* p) {
    p->family = LF_W4_PC;
    p->M = M, p->wq = 4, p->epi = epi;
    p->bn = PC_BN, p->bm = PC_BM;
    p->n_tiles = (N + PC_BN - 1) / PC_BN, p->m_tiles = (int)((M + PC_BM - 1) / PC_BM);
    p->grid_x = xcd_grid(p->n_tiles, p->m_tiles), p->threads = 512, p->lds = PC_LDS;
    return true;
}

bool plan_w8_wide(int64_t M, int N, int epi, int nc, LinearPart* p) {
    if (nc != 12) return false;
    p->family = LF_W8_WIDE;
    p->M = M, p->wq = 8, p->epi = epi, p->stages = WD_ST, p->nc = nc;
    p->bn = 32 * nc, p->bm = WD_BM;
    p->n_tiles = (N + p->bn - 1) / p->bn, p->m_tiles = (int)((M + WD_BM - 1) / WD_BM);
    p->grid_x = xcd_grid(p->n_tiles, p->m_tiles), p->threads = (unsigned)(nc + WD_NP) * 64, p->lds = (size_t)wide_lds_bytes(WD_ST, nc);
    return true;
}

// rows [m0, m0 + M) of the problem as one launch
static bool plan_part(const LinearProblem& pr, const LinearTuning& t, int64_t m0, int64_t M, bool defer, LinearPart* p) {
    const int wq = pr.wq_bit, group = pr.group, N = pr.N, K = pr.K, epi = pr.epi;
    const bool ws = pr.ws_bytes > 0;
    const size_t ws_bytes = pr.ws_bytes;
    const uintptr_t x = pr.x + (uintptr_t)(m0 * K * 2), y = pr.y + (uintptr_t)(m0 * pr.ldy * (epi == EPI_F32 ? 4 : 2));
    *p = LinearPart{};
    p->M = M, p->wq = wq, p->epi = epi;
    bool ok = true;
    // up to 4 rows (LinearTuning::gemv_stream_max_m): the streaming GEMV of k_gemv.hip -- whole 1-KiB row pieces per wave-load, no matrix unit
    if (M <= gemv_stream_max_m(wq, group, N, K, t.gemv_stream_max_m) && !t.no_skinny && !t.force_generic) {
        ok = plan_gemv_stream(wq, M, N, K, epi, p);
    } else if (M <= (ws ? (wq == 8 && K % (G_BK * 2) == 0 && t.gemv_max_m > 2 && !t.gemv_max_m_set ? 2 : t.gemv_max_m) : 16) && M <= 16 && !t.no_skinny) {
        // the MFMA skinny kernel.  Without a split-K workspace the half-height tiles would run as N / 128 unsplit blocks: it keeps its 16 rows
        // there; int8 weights with K % 128 == 0: from 3 rows the half-height tiles with 16-row activation sub-tiles are faster
        p->family = LF_GEMV;
        p->nw = (t.gemv_waves ? t.gemv_waves : ((N + 15) / 16 <= 1024 ? 8 : 4)) == 8 ? 8 : 4;   // every CU needs enough waves streaming
        p->bn = 16, p->bm = 16;
        p->n_tiles = (N + 15) / 16, p->m_tiles = 1;
        p->grid_x = (unsigned)p->n_tiles, p->threads = (unsigned)p->nw * 64;
    } else if (t.pc_mode && wq == 4 && M > 128 && M <= 512 && !t.force_generic && (int64_t)((N + 63) / 64) * ((M + 127) / 128) >= 160 &&
               linear_w4_pc_supported(group, M, N, K, x, pr.w, pr.scale, y, pr.ldy, epi)) {
        // W4A16 at a few hundred rows (config 4: the 70B / TP8 slice at batch 256): 128 x 64 tiles, DMA waves beside MFMA waves whose fragment
        // registers roll (k_gemm_pc.hip) -- for the shapes whose tiles fill most CUs WITHOUT K slabs (wo / w13 / w2 of that slice: 256 / 224 /
        // 256 blocks).  A shape that needs slabs anyway (wqkv: 40 tiles) stays on the ring kernel
        ok = plan_w4_pc(M, N, epi, p);
    } else if (t.wide && wq == 8 && K % G_BK == 0 && M >= 512 && (M < 4096 || t.wide == 2) && N >= 8192 &&
               (t.wide == 2 || linear_w8_wide_waves(M, N) == 12)) {
        // W8A16 at 512 <= M < 4096 with N >= 8192 (wqkv / w13 of a decode step at batch ~1024): one 128 x 384 block per CU whose twelve
        // consumer waves share the activation tile (k_gemm_wide.hip) when its tiles fill the chip's rounds
        ok = plan_w8_wide(M, N, epi, 12, p);
    } else {
        const int n_tiles = (N + G_BN - 1) / G_BN, m_tiles = (int)((M + G_BM - 1) / G_BM);
        // W4: group 128 = two K tiles; one block keeps at most W4_MAXG groups of scales in LDS
        const bool w4_fast = wq == 4 && group == 128 && K % 128 == 0 &&
                             (K / 128 <= W4_MAXG || (ws && (size_t)((K / 128 + W4_MAXG - 1) / W4_MAXG) * M * N * sizeof(float) <= ws_bytes));
        p->n_tiles = n_tiles, p->m_tiles = m_tiles;
        p->bn = G_BN, p->bm = G_BM;
        if (wq == 8 && K % G_BK == 0 && M >= t.min_m256 && N >= 1024 && !t.force_generic) {
            // W8A16, prefill steps: 256 x 256 tiles.  Super-tile shape: gm = the largest divisor of the activation tiles <= 4 (X tiles carry
            // twice the bytes of W tiles), gn = up to 8 weight tiles of the XCD's share; the share is padded to whole super-tiles (the extra
            // blocks return at once).  (A forced value that does not fit MapMode's bytes is ignored.)
            const int nt2 = (N + H_BN - 1) / H_BN, mt2 = (int)((M + H_BM - 1) / H_BM);
            const int nl = (nt2 + 7) / 8;  // weight tiles per XCD
            int gm = t.gm256 > 0 && t.gm256 <= 255 ? t.gm256 : 4;
            while (gm > 1 && mt2 % gm) --gm;
            int gn = t.gn256 > 0 && t.gn256 <= 255 ? t.gn256 : 8;
            if (gn > nl) gn = nl;
            p->family = LF_W8_256;
            p->bn = H_BN, p->bm = H_BM, p->stages = H_ST;
            p->n_tiles = nt2, p->m_tiles = mt2;
            p->map = MapMode{0, 0, (uint8_t)gm, (uint8_t)gn};
            p->grid_x = (unsigned)(8 * ((nl + gn - 1) / gn * gn) * mt2), p->threads = 512, p->lds = H_LDS;
            p->staged = !t.direct_epilogue && pr.ldy % 8 == 0 && (y & 15) == 0 && (epi != EPI_SWIGLU || N % 16 == 0) ? 1 : 0;
        } else if ((wq == 8 || wq == 0 || w4_fast) && K % G_BK == 0 && !t.force_generic) {
            // ---- the 128 x 128 ring kernel, or for W8 at M <= 128 the half-height 128-deep kernel -------------------------------------
            const int64_t tiles = (int64_t)n_tiles * m_tiles;
            const bool st_forced = t.stages >= 2 && t.stages <= 4;
            // few blocks per CU -> deeper ring (latency is hidden inside the block); many -> more blocks per CU (profiles/gemm_microbench.py)
            int stages = st_forced ? t.stages : (tiles <= 256 ? 4 : 2);
            if (wq == 0 && stages == 4) stages = 3;  // fp16 weights: 4 x 32 KiB would leave one block per CU anyway
            // split-K for small M: too few output tiles to pull HBM bandwidth (weights must stream at full rate); also at larger M when a
            // tensor-parallel slice leaves fewer output tiles than CUs
            const int kt_all = K / G_BK;
            int splits = 1;
            if (ws && ((M <= 256 && tiles < 512) || tiles < 200 || t.splitk > 0)) {
                // enough blocks to fill the chip, but every split writes an fp32 slab of the whole output: keep >= min_kt K tiles per split
                const int target = M <= 64 ? 768 : 512;
                splits = (int)((target + tiles - 1) / tiles);
                const int cap = (M <= 64 || tiles <= 32) ? 8 : 4;  // (M = 128..256 sweeps: more than 4 slabs never paid)
                if (splits > cap) splits = cap;
                if (M > 64 && tiles >= 160) splits = 1;             // most CUs busy already: a slab costs more (176 tiles, 7B/TP8 w13: 36 vs 42 us)
                const int min_kt = t.minkt ? t.minkt : ((M <= 64 || tiles <= 64) ? 16 : 28);
                if (splits > kt_all / min_kt) splits = kt_all / min_kt > 0 ? kt_all / min_kt : 1;
                if (t.splitk > 0) splits = t.splitk;
                while (splits > 1 && (size_t)splits * M * N * sizeof(float) > ws_bytes) --splits;
            }
            if (wq == 4 && splits < (kt_all + 2 * W4_MAXG - 1) / (2 * W4_MAXG)) splits = (kt_all + 2 * W4_MAXG - 1) / (2 * W4_MAXG);
            int kt_per = (kt_all + splits - 1) / splits;
            if (wq == 4) kt_per = (kt_per + 1) & ~1;  // whole quantisation groups per split
            splits = (kt_all + kt_per - 1) / kt_per;  // no empty split
            if (splits > 1 && !st_forced) stages = (t.split_deep && tiles * splits <= 256 && !(wq == 4 && M <= 64)) ? (wq == 0 ? 3 : 4) : 2;
            // at most one block per CU: 8 waves, 4 of them producers; more blocks: 4 waves of 32 (n) x 128 (m), two blocks per CU
            int wl = (t.wl == 1 || t.wl == 5) ? t.wl : (tiles * splits <= 256 ? 5 : 1);
            const bool half = t.half >= 0 ? (t.half == 1 && M <= 64) : M <= 64;   // 16 < M <= 64: half-height tiles, 4-wave blocks
            if (half) wl = 1;
            if ((t.wl == 6 || (t.wl == 0 && wl == 5)) && wq == 8 && stages >= 3 && splits == 1) wl = 6;
            // the half-height kernel's own slab count: one block per CU
            int sp = splits;
            const int kt128 = K / (G_BK * S_KS);
            if (ws && t.splitk <= 0) {
                sp = t.half128_blocks / n_tiles;
                if (sp > 8) sp = 8;
                if (sp < 1) sp = 1;
                while (sp > 1 && (size_t)sp * M * N * sizeof(float) > ws_bytes) --sp;
            }
            if (sp > kt128) sp = kt128 > 0 ? kt128 : 1;
            if (t.half128 && (half || (M <= 128 && M <= t.half128_max_m && (sp > 1 || M <= t.half128_unsplit_max_m) && m_tiles == 1)) && wq == 8 &&
                K % (G_BK * S_KS) == 0) {
                // W8, half-height tiles: the 128-deep K tile (whole 128-byte lines of every weight row per LDS-DMA piece), activation sub-tile
                // 16 / 32 / 64 rows, above 64 rows in steps of 16 (a 72-row step on a 128-row sub-tile would pay 128 rows of LDS traffic and
                // MFMAs); three stages when two blocks of them fit a CU (BM <= 32) or the grid is one block per CU
                const int kt_per128 = (kt128 + sp - 1) / sp;
                sp = (kt128 + kt_per128 - 1) / kt_per128;
                const int bm = M > 64 ? (int)((M + 15) / 16 * 16) : (t.half128 == 2 ? 64 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64)));
                p->family = LF_W8_HALF128;
                p->bm = bm, p->stages = (bm <= 32 || bm > 64 || (int64_t)n_tiles * sp <= 256) ? 3 : 2;
                p->splits = sp, p->kt_per = kt_per128, p->kt_depth = G_BK * S_KS;
                p->grid_x = (unsigned)n_tiles, p->grid_y = (unsigned)sp, p->threads = 256, p->lds = (size_t)half128_lds_bytes(p->stages, bm);
            } else {
                // W4 with K slabs of at most 32 tiles (16 quantisation groups): the scale area shrinks from 16 to 4 KiB and three blocks fit a CU
                const bool w4_small_sc = t.w4_sc16 && wq == 4 && splits > 1 && kt_per <= 32 && wl == 1 && !half && stages == 2;
                p->family = LF_RING;
                p->stages = stages, p->wl = 1, p->bm = G_BM, p->maxg = W4_MAXG;
                if (wl == 6 && wq == 8 && stages >= 3) p->wl = 6;
                else if (wl == 5) p->wl = 5;
                else if (half) p->bm = 64;
                else if (w4_small_sc) p->maxg = 16;
                p->splits = splits, p->kt_per = kt_per, p->kt_depth = G_BK;
                p->threads = p->wl == 6 ? 768 : (p->wl == 5 ? 512 : 256);
                p->grid_x = xcd_grid(n_tiles, m_tiles), p->grid_y = (unsigned)splits;
                p->map.ablate = (uint8_t)t.ablate;
                if (t.map == 1 && m_tiles % 8 == 0) {
                    p->map.order = 1;
                    p->grid_x = (unsigned)(n_tiles * m_tiles);
                } else if (m_tiles > 8 || t.gm128_set) {
                    // more than 8 activation tiles (M > 1024): walk the XCD's weight tiles in super-tiles of 12 (n) x 8 (m) -- at M = 1024 the
                    // plain order already is that shape; at M = 8192 it degenerates to 1.5 weight tiles x 64 activation tiles in flight per XCD
                    int gm = t.gm128 > 0 ? t.gm128 : 8;
                    while (gm > 1 && m_tiles % gm) --gm;
                    const int nl = (n_tiles + 7) / 8;
                    int gn = t.gn128 > 0 ? t.gn128 : 12;
                    if (gn > nl) gn = nl;
                    if (gm > 1 && gn <= 255 && gm <= 255) {
                        p->map.gm = (uint8_t)gm, p->map.gn = (uint8_t)gn;
                        p->grid_x = (unsigned)(8 * ((nl + gn - 1) / gn * gn) * m_tiles);
                    }
                }
            }
            if (p->splits > 1) p->reduce = defer && epi == EPI_F16 && N % 8 == 0 && p->splits <= 8 ? LR_DEFERRED : LR_KERNEL;
        } else {
            p->family = LF_GENERIC;
            p->grid_x = xcd_grid(n_tiles, m_tiles), p->threads = 256;
        }
    }
    p->m0 = m0;
    return ok;
}

bool linear_problem_valid(const LinearProblem& p) {
    if (p.epi != EPI_F16 && p.epi != EPI_F32 && p.epi != EPI_SWIGLU) return false;
    if (p.N % 4 || p.ldy % 4) return false;
    if (p.wq_bit == 0) return p.K % 8 == 0;
    if (p.wq_bit == 8) return p.K % 16 == 0;
    if (p.wq_bit == 4) return !(p.K % 32 || p.group % 32 || p.K % p.group);
    return false;
}

LinearPlan plan_linear(const LinearProblem& pr, const LinearTuning& t) {
    LinearPlan plan;
    const int64_t M = pr.M;
    // A few rows above a multiple of 1024 (a saturated continuous-batching step: 1024 decode rows + the prompt chunk of a newly admitted
    // request) would add a ninth / seventeenth 128-row tile to every column block -- a whole extra round of tiles for a few rows (7B layer
    // GEMMs at M = 1040: 555 us against 414 us at M = 1024).  The rows up to the multiple go through the shapes that fit, the rest as a
    // second, small launch; neither part defers its slabs.
    if (t.msplit && M > 1024 && M < 3584 && (M & 1023) != 0 && (M & 1023) <= t.msplit) {
        const int64_t m_main = M & ~(int64_t)1023;
        plan.n_parts = 2;
        plan.ok = plan_part(pr, t, 0, m_main, false, &plan.part[0]) && plan_part(pr, t, m_main, M - m_main, false, &plan.part[1]);
    } else {
        plan.n_parts = 1;
        plan.ok = plan_part(pr, t, 0, M, pr.accept_defer, &plan.part[0]);
    }
    return plan;
}

int format_route(const LinearPart& p, char* buf, int cap) {
    char kernel[96], tail[48] = "";
    const char* e = epi_name(p.epi);
    switch (p.family) {
        case LF_GEMV_STREAM: snprintf(kernel, sizeof kernel, "gemv_stream_kernel<%d,%d,%s,%d>", p.wq, (int)p.M, e, p.nw); break;
        case LF_GEMV: snprintf(kernel, sizeof kernel, "gemv_kernel<%d,1,%s,%d>", p.wq, e, p.nw); break;
        case LF_W4_PC: snprintf(kernel, sizeof kernel, "gemm_w4_pc_kernel<%s>", e); break;
        case LF_W8_WIDE: snprintf(kernel, sizeof kernel, "gemm_w8_wide_kernel<%s,%d,%d>", e, p.stages, p.nc); break;
        case LF_W8_256: snprintf(kernel, sizeof kernel, "gemm_w8_dma256_kernel<%s>", e); break;
        case LF_W8_HALF128: snprintf(kernel, sizeof kernel, "gemm_w8_half128_kernel<%s,%d,%d>", e, p.stages, p.bm); break;
        case LF_RING:  // the defaulted arguments BM and MAXG appear only where they differ
            if (p.maxg != W4_MAXG) snprintf(tail, sizeof tail, ",%d,%d", p.bm, p.maxg);
            else if (p.bm != G_BM) snprintf(tail, sizeof tail, ",%d", p.bm);
            snprintf(kernel, sizeof kernel, "gemm_dma_kernel<%d,%s,%d,%d%s>", p.wq, e, p.stages, p.wl, tail);
            break;
        case LF_GENERIC: snprintf(kernel, sizeof kernel, "gemm_kernel<%d,%s>", p.wq, e); break;
    }
    char kchunk[32] = "", reduce[48] = "reduce=none", order[32] = "order=plain";
    if (p.kt_depth) snprintf(kchunk, sizeof kchunk, " kchunk=%d", p.kt_per * p.kt_depth);
    if (p.reduce == LR_DEFERRED) snprintf(reduce, sizeof reduce, "reduce=deferred");
    else if (p.reduce == LR_KERNEL) snprintf(reduce, sizeof reduce, "reduce=splitk_reduce_kernel<%s>", e);
    if (p.map.order == 1) snprintf(order, sizeof order, "order=xcd_m");
    else if (p.map.gm) snprintf(order, sizeof order, "order=super(%dx%d)", p.map.gm, p.map.gn);
    tail[0] = 0;
    if (p.family == LF_GEMV_STREAM) snprintf(tail, sizeof tail, " nwk=%d nb=%d", 1 << p.nwk_log2, p.nb);
    else if (p.family == LF_W8_256) snprintf(tail, sizeof tail, " epilogue=%s", p.staged ? "staged" : "direct");
    const int n = snprintf(buf, (size_t)cap, "kernel=%s splits=%d%s %s %s%s", kernel, p.splits, kchunk, reduce, order, tail);
    return n < cap ? n : cap - 1;
}

// ---- the quantised-activation linears --------------------------------------------------------------------------------------------------
Q8Tuning Q8Tuning::from_env() {
    Q8Tuning t;
    t.force_generic = tune_set("PPLHIP_GEMM_GENERIC");
    t.min_m256 = tune_int("PPLHIP_GEMM_I8_256_MIN_M", t.min_m256);
    t.st256 = tune_int("PPLHIP_GEMM_I8_256_ST", t.st256);
    t.gm256 = tune_int("PPLHIP_GEMM256_GM", t.gm256);
    t.gn256 = tune_int("PPLHIP_GEMM256_GN", t.gn256);
    t.wide = tune_int("PPLHIP_GEMM_I8_WIDE", t.wide);
    t.pc = tune_int("PPLHIP_GEMM_I8_PC", t.pc);
    return t;
}

bool linear_q8_valid(int64_t M, int N, int K, int64_t ldy, int epi) {
    if (M < 1 || (epi != EPI_F16 && epi != EPI_F32 && epi != EPI_SWIGLU)) return false;
    return !(N % 4 || ldy % 4 || K % 16);
}

// int8 and fp8 share one dispatch table, except that fp8 has no 256 x 256 form (steps of M >= 4096 take the 128 x 128 producer / consumer
// form)
Q8Plan plan_linear_q8(bool f8, int64_t M, int N, int K, int64_t ldy, int epi, const Q8Tuning& t) {
    Q8Plan p;
    (void)ldy;
    p.ok = true, p.f8 = f8, p.epi = epi;
    if (M > 32 && K % I_BK == 0 && !t.force_generic) {
        const int n_tiles = (N + I_BN - 1) / I_BN, m_tiles = (int)((M + I_BM - 1) / I_BM);
        if (!f8 && M >= t.min_m256 && N >= 1024) {
            // super-tile shape: gm = the largest divisor of the activation tiles <= 4, gn = up to 8 weight tiles of the XCD's share; the share
            // is padded to whole super-tiles (the extra blocks return at once)
            const int nt2 = (N + I2_BN - 1) / I2_BN, mt2 = (int)((M + I2_BM - 1) / I2_BM);
            const int nl = (nt2 + 7) / 8;
            int gm = t.gm256 > 0 ? t.gm256 : 4;
            while (gm > 1 && mt2 % gm) --gm;
            int gn = t.gn256 > 0 ? t.gn256 : 8;
            if (gn > nl) gn = nl;
            p.family = QF_256;
            p.stages = t.st256 == 3 ? 3 : 4;
            p.bn = I2_BN, p.bm = I2_BM, p.bk = I2_BK;
            p.n_tiles = nt2, p.m_tiles = mt2, p.gn = gn, p.gm = gm;
            p.grid_x = (unsigned)(8 * ((nl + gn - 1) / gn * gn) * mt2), p.threads = 512, p.lds = (size_t)i8_256_lds_bytes(p.stages);
            return p;
        }
        // 128 x 384 tiles when they fill rounds of 256 one-per-CU blocks (the rule of linear_w8_wide_waves)
        if (t.wide && M >= 512 && N >= 8192 && linear_w8_wide_waves(M, N) == 12) {
            p.family = QF_WIDE;
            p.stages = IW_ST;
            p.bn = IW_BN, p.bm = I_BM, p.bk = I_BK;
            p.n_tiles = (N + IW_BN - 1) / IW_BN, p.m_tiles = m_tiles;
            p.grid_x = xcd_grid(p.n_tiles, m_tiles), p.threads = (unsigned)(IW_NC + IW_NP) * 64, p.lds = (size_t)i8_wide_lds_bytes();
            return p;
        }
        // 8-wave producer / consumer blocks for everything else (measured at M = 1024 against the 4-wave kernel k_gemm_i8.hip held until it
        // had lost on every shape: wo 32.5 -> 28.6 us and w2 76.0 -> 51.4 us with a 4-stage ring, one block per CU; w13 116.6 -> 106.0 us
        // with two stages, two blocks per CU; wqkv 62.1 vs 63.6 us; M = 2048 layer 502 -> 459 us, M = 8192 equal)
        int pc = t.pc >= 0 ? t.pc : ((int64_t)n_tiles * m_tiles <= 256 ? 4 : 2);
        if (pc != 3 && pc != 4) pc = 2;
        p.family = QF_PC;
        p.stages = pc;
        p.bn = I_BN, p.bm = I_BM, p.bk = I_BK;
        p.n_tiles = n_tiles, p.m_tiles = m_tiles;
        p.grid_x = xcd_grid(n_tiles, m_tiles), p.threads = 512, p.lds = (size_t)i8_pc_lds_bytes(pc);
        return p;
    }
    // skinny / generic: one 16-row activation tile per block up to 16 rows (eight K slices while the row tiles are few), else two
    const int nblk = (N + IV_BN - 1) / IV_BN;
    p.family = QF_GEMV;
    p.mt = M > 16 ? 2 : 1;
    p.nw = M > 16 ? 4 : (nblk <= 1024 ? 8 : 4);
    p.bn = IV_BN, p.bm = p.mt * IV_BM;
    p.n_tiles = nblk, p.m_tiles = M <= 16 ? 1 : (int)((M + 31) / 32);
    p.grid_x = (unsigned)nblk, p.grid_y = (unsigned)p.m_tiles, p.threads = (unsigned)p.nw * 64;
    return p;
}

int format_route(const Q8Plan& p, char* buf, int cap) {
    char kernel[96], order[32] = "";
    const char *e = epi_name(p.epi), *f = p.f8 ? "f8" : "i8";
    switch (p.family) {
        case QF_GEMV: snprintf(kernel, sizeof kernel, "gemv_i8_kernel<%d,%s,%d,%s>", p.mt, e, p.nw, f); break;
        case QF_PC: snprintf(kernel, sizeof kernel, "gemm_i8_pc_kernel<%s,%d,%s>", e, p.stages, f); break;
        case QF_WIDE: snprintf(kernel, sizeof kernel, "gemm_i8_wide_kernel<%s,%s>", e, f); break;
        case QF_256:
            snprintf(kernel, sizeof kernel, "gemm_i8_256_kernel<%s,%d>", e, p.stages);
            snprintf(order, sizeof order, " order=super(%dx%d)", p.gm, p.gn);
            break;
    }
    const int n = snprintf(buf, (size_t)cap, "kernel=%s grid=%ux%u threads=%u lds=%zu n_tiles=%d m_tiles=%d%s", kernel, p.grid_x, p.grid_y,
                           p.threads, p.lds, p.n_tiles, p.m_tiles, order);
    return n < cap ? n : cap - 1;
}

int format_route(const LinearPlan& plan, char* buf, int cap) {
    int len = 0;
    if (cap > 0) buf[0] = 0;
    for (int i = 0; i < plan.n_parts && len < cap - 1; ++i) {
        if (i) len += snprintf(buf + len, (size_t)(cap - len), " ; ");
        if (len < cap - 1) len += format_route(plan.part[i], buf + len, cap - len);
    }
    return len < cap ? len : cap - 1;
}

}  // namespace pplhip
