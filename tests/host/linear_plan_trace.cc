// Test driver of the linear launch plan (csrc/linear_plan.cc, built with the host compiler alone: no HIP, no device).
// stdin, one problem per line:   wq group M N K epi ws_bytes defer ldy y_addr
// stdout, one line per problem:  <status>\t<route text>\t<the numbers of every part>      status 0: planned (or M = 0), -2: refused
// Every plan is checked against the conditions the kernels rely on (check_part / check_plan below); the first plan that breaks one is
// named on stderr with its input line and the program exits 1.
// The x / w / scale addresses are the aligned fake ones of tests/gemm_exact.py dry_route (scale 0 for fp16 weights).
// `linear_plan_trace q8`: the plan of the quantised-activation linears (plan_linear_q8) instead.
// stdin, one problem per line:   act_fmt(8 | 264) M N K epi ldy          stdout and the checks (check_q8 below): as above
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../ppl.llm.serving_amd/csrc/linear_plan.h"

using namespace pplhip;

static const char* kFamily[] = {"gemv_stream", "gemv", "w4_pc", "w8_wide", "w8_256", "w8_half128", "ring", "generic"};

// the tile a block takes, as the kernels compute it (k_gemm_dev.h xcd_tile / xcd_super_tile, gemm_dma_body); false: the block returns at once
static bool block_tile(const LinearPart& p, unsigned id, int* nt, int* mt) {
    if (p.family == LF_GEMV_STREAM || p.family == LF_GEMV || p.family == LF_W8_HALF128) {   // blockIdx.x is the weight tile
        *nt = (int)id, *mt = 0;
        return *nt < p.n_tiles;
    }
    const int xcd = (int)(id & 7), slot = (int)(id >> 3);
    if (p.map.order == 1) {
        const int mg = p.m_tiles >> 3;
        *mt = xcd + 8 * (slot % mg), *nt = slot / mg;
    } else if (p.map.gm == 0) {
        *nt = xcd + 8 * (slot / p.m_tiles), *mt = slot % p.m_tiles;
    } else {
        const int gm = p.map.gm, gn = p.map.gn, per_super = gn * gm, sm_count = p.m_tiles / gm;
        const int sup = slot / per_super, within = slot % per_super;
        *nt = xcd + 8 * ((sup / sm_count) * gn + within / gm), *mt = (sup % sm_count) * gm + within % gm;
    }
    return *nt < p.n_tiles;
}

static size_t family_lds(const LinearPart& p) {
    switch (p.family) {
        case LF_W4_PC: return PC_LDS;
        case LF_W8_WIDE: return (size_t)wide_lds_bytes(p.stages, p.nc);
        case LF_W8_256: return H_LDS;
        case LF_W8_HALF128: return (size_t)half128_lds_bytes(p.stages, p.bm);
        default: return 0;   // static LDS only
    }
}

static unsigned family_threads(const LinearPart& p) {   // the kernels' __launch_bounds__
    switch (p.family) {
        case LF_GEMV_STREAM: case LF_GEMV: return (unsigned)p.nw * 64;
        case LF_W4_PC: case LF_W8_256: return 512;
        case LF_W8_WIDE: return (unsigned)(p.nc + WD_NP) * 64;
        case LF_RING: return p.wl == 6 ? 768 : (p.wl == 5 ? 512 : 256);
        default: return 256;
    }
}

#define REQUIRE(cond)                          \
    do {                                       \
        if (!(cond)) return std::string(#cond); \
    } while (0)

// "" or the condition a part breaks
static std::string check_part(const LinearProblem& pr, const LinearPart& p) {
    REQUIRE(p.M >= 1 && p.grid_x >= 1 && p.grid_y >= 1);
    // the grid covers every tile, each by exactly one block
    REQUIRE((int64_t)p.n_tiles * p.bn >= pr.N && (int64_t)p.m_tiles * p.bm >= p.M);
    REQUIRE((uint64_t)p.grid_x >= (uint64_t)p.n_tiles * (uint64_t)p.m_tiles);
    REQUIRE(p.map.gm == 0 || p.m_tiles % p.map.gm == 0);
    REQUIRE(p.map.order == 0 || p.m_tiles % 8 == 0);
    if (p.grid_x <= 4096) {
        std::vector<int> hits((size_t)p.n_tiles * p.m_tiles, 0);
        for (unsigned id = 0; id < p.grid_x; ++id) {
            int nt, mt;
            if (!block_tile(p, id, &nt, &mt)) continue;
            REQUIRE(nt >= 0 && mt >= 0 && mt < p.m_tiles);
            ++hits[(size_t)nt * p.m_tiles + mt];
        }
        for (int h : hits) REQUIRE(h == 1);
    }
    // K slabs: none empty, a workspace that holds them
    REQUIRE(p.splits >= 1 && p.grid_y == (unsigned)p.splits);
    if (p.kt_depth) {
        const int kt_all = pr.K / p.kt_depth;
        REQUIRE(pr.K % p.kt_depth == 0);
        REQUIRE((int64_t)(p.splits - 1) * p.kt_per < kt_all && kt_all <= (int64_t)p.splits * p.kt_per);
    } else {
        REQUIRE(p.splits == 1);
    }
    if (p.family == LF_RING && p.wq == 4) REQUIRE(p.kt_per % 2 == 0 && p.kt_per / 2 <= p.maxg);
    REQUIRE((p.splits > 1) == (p.reduce != LR_NONE));
    if (p.splits > 1) REQUIRE(pr.ws_bytes > 0 && (uint64_t)p.splits * (uint64_t)p.M * (uint64_t)pr.N * 4 <= pr.ws_bytes);
    if (p.reduce == LR_DEFERRED) REQUIRE(pr.accept_defer && p.epi == EPI_F16 && pr.N % 8 == 0 && p.splits <= 8);
    // LDS and block size
    REQUIRE(p.lds == family_lds(p) && p.lds <= (size_t)LDS_PER_CU);
    if (p.family == LF_RING) REQUIRE(gemm_dma_lds_bytes(p.wq, p.stages, p.bm, p.maxg) <= LDS_PER_CU);   // (its static LDS)
    REQUIRE(p.threads == family_threads(p) && p.threads <= 1024);
    return "";
}

static std::string check_plan(const LinearProblem& pr, const LinearPlan& plan) {
    REQUIRE(plan.n_parts == 1 || plan.n_parts == 2);
    int64_t next = 0;
    for (int i = 0; i < plan.n_parts; ++i) {   // the parts are disjoint and cover [0, M)
        REQUIRE(plan.part[i].m0 == next);
        next += plan.part[i].M;
        const std::string bad = check_part(pr, plan.part[i]);
        if (!bad.empty()) return "part " + std::to_string(i) + ": " + bad;
    }
    REQUIRE(next == pr.M);
    if (plan.n_parts == 2) REQUIRE(plan.part[0].M % 1024 == 0 && plan.part[1].reduce != LR_DEFERRED && plan.part[0].reduce != LR_DEFERRED);
    return "";
}

// the quantised-activation kernels (k_gemm_i8.hip): "" or the condition a plan breaks
static std::string check_q8(int64_t M, int N, int K, const Q8Plan& p) {
    REQUIRE(p.grid_x >= 1 && p.grid_y >= 1 && p.n_tiles >= 1 && p.m_tiles >= 1);
    REQUIRE((int64_t)p.n_tiles * p.bn >= N && (int64_t)(p.n_tiles - 1) * p.bn < N);
    REQUIRE((int64_t)p.m_tiles * p.bm >= M && (int64_t)(p.m_tiles - 1) * p.bm < M);
    REQUIRE(p.lds <= (size_t)LDS_PER_CU && p.threads <= 1024);
    if (p.family == QF_GEMV) {
        // any M, K % 16 == 0: blockIdx.x walks 16 weight rows, blockIdx.y the 16 / 32-row activation groups; static LDS only
        REQUIRE(K % 16 == 0);
        REQUIRE(p.grid_x == (unsigned)p.n_tiles && p.grid_y == (unsigned)p.m_tiles && p.lds == 0);
        REQUIRE((p.mt == 1 && (p.nw == 4 || p.nw == 8) && M <= 16) || (p.mt == 2 && p.nw == 4 && M > 16));
        REQUIRE(p.bn == IV_BN && p.bm == p.mt * IV_BM && p.threads == (unsigned)p.nw * 64);
        REQUIRE(i8_gemv_lds_bytes(p.mt, p.nw) <= 64 * 1024);
        return "";
    }
    // the tile kernels: M > 32 and whole 128-deep K tiles only
    REQUIRE(M > 32 && K % 128 == 0 && K % p.bk == 0 && p.grid_y == 1);
    // the grid covers n_tiles * m_tiles after the round-up to the 8 XCDs, each tile by exactly one block
    REQUIRE((uint64_t)p.grid_x >= (uint64_t)p.n_tiles * (uint64_t)p.m_tiles && p.grid_x % 8 == 0);
    if (p.family != QF_256) REQUIRE(p.grid_x == (unsigned)((p.n_tiles + 7) / 8 * 8 * p.m_tiles));
    if (p.family == QF_256) REQUIRE(p.gm >= 1 && p.gn >= 1 && p.m_tiles % p.gm == 0 && p.grid_x % (8u * p.gn * p.gm) == 0);
    if (p.grid_x <= 8192) {
        LinearPart q;   // (block_tile's fields)
        q.family = LF_RING, q.n_tiles = p.n_tiles, q.m_tiles = p.m_tiles;
        q.map = MapMode{0, 0, (uint8_t)p.gm, (uint8_t)p.gn};
        std::vector<int> hits((size_t)p.n_tiles * p.m_tiles, 0);
        for (unsigned id = 0; id < p.grid_x; ++id) {
            int nt, mt;
            if (!block_tile(q, id, &nt, &mt)) continue;
            REQUIRE(nt >= 0 && mt >= 0 && mt < p.m_tiles);
            ++hits[(size_t)nt * p.m_tiles + mt];
        }
        for (int h : hits) REQUIRE(h == 1);
    }
    // dynamic LDS = stages x (activation + weight bytes of a stage)
    REQUIRE(p.stages >= 2 && p.lds == (size_t)p.stages * (size_t)(p.bm + p.bn) * p.bk);
    switch (p.family) {
        case QF_PC:
            REQUIRE(p.bn == 128 && p.bm == 128 && p.bk == 128 && p.threads == 512 && p.stages <= 4);
            REQUIRE(p.lds == (size_t)i8_pc_lds_bytes(p.stages));
            break;
        case QF_WIDE:
            REQUIRE(p.bn == 384 && p.bm == 128 && p.bk == 128 && p.stages == IW_ST && p.threads == (unsigned)(IW_NC + IW_NP) * 64);
            REQUIRE(M >= 512 && N >= 8192 && linear_w8_wide_waves(M, N) == 12);
            REQUIRE(p.lds == (size_t)i8_wide_lds_bytes());
            break;
        case QF_256:
            REQUIRE(!p.f8 && N >= 1024);
            REQUIRE(p.bn == 256 && p.bm == 256 && p.bk == 64 && p.threads == 512 && (p.stages == 3 || p.stages == 4));
            REQUIRE(p.lds == (size_t)i8_256_lds_bytes(p.stages));
            break;
        default: return "family";
    }
    return "";
}

static int main_q8() {
    const Q8Tuning tuning = Q8Tuning::from_env();
    static const char* kQ8Family[] = {"gemv", "pc", "wide", "256"};
    char line[256], route[256];
    long lineno = 0;
    while (fgets(line, sizeof line, stdin)) {
        ++lineno;
        int fmt, N, K, epi;
        long long M, ldy;
        if (sscanf(line, "%d %lld %d %d %d %lld", &fmt, &M, &N, &K, &epi, &ldy) != 6) {
            fprintf(stderr, "line %ld: expected 'act_fmt M N K epi ldy': %s", lineno, line);
            return 2;
        }
        if (M == 0 && (fmt == 8 || fmt == 0x108) && epi >= 0 && epi <= 2) {
            printf("0\t\t\n");
            continue;
        }
        if ((fmt != 8 && fmt != 0x108) || !linear_q8_valid(M, N, K, ldy, epi)) {
            printf("-2\t\t\n");
            continue;
        }
        const Q8Plan p = plan_linear_q8(fmt == 0x108, M, N, K, ldy, epi, tuning);
        if (!p.ok) {
            printf("-2\t\t\n");
            continue;
        }
        format_route(p, route, (int)sizeof route);
        printf("0\t%s\tfamily=%s stages=%d bn=%d bm=%d bk=%d\n", route, kQ8Family[p.family], p.stages, p.bn, p.bm, p.bk);
        const std::string bad = check_q8(M, N, K, p);
        if (!bad.empty()) {
            fflush(stdout);
            fprintf(stderr, "line %ld breaks an invariant: %s\n  %s", lineno, bad.c_str(), line);
            return 1;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "q8") return main_q8();
    const LinearTuning tuning = LinearTuning::from_env();
    char line[512], route[512];
    long lineno = 0;
    while (fgets(line, sizeof line, stdin)) {
        ++lineno;
        LinearProblem pr;
        long long M, ws_bytes, ldy, y_addr;
        int defer;
        if (sscanf(line, "%d %d %lld %d %d %d %lld %d %lld %lld", &pr.wq_bit, &pr.group, &M, &pr.N, &pr.K, &pr.epi, &ws_bytes, &defer, &ldy, &y_addr) != 10) {
            fprintf(stderr, "line %ld: expected 'wq group M N K epi ws_bytes defer ldy y_addr': %s", lineno, line);
            return 2;
        }
        pr.M = M, pr.ws_bytes = (size_t)ws_bytes, pr.accept_defer = defer != 0, pr.ldy = ldy, pr.y = (uintptr_t)y_addr;
        pr.x = (uintptr_t)1 << 21, pr.w = (uintptr_t)1 << 22, pr.scale = pr.wq_bit ? (uintptr_t)1 << 23 : 0;
        if (pr.M == 0) {
            printf("0\t\t\n");
            continue;
        }
        if (!linear_problem_valid(pr)) {
            printf("-2\t\t\n");
            continue;
        }
        const LinearPlan plan = plan_linear(pr, tuning);
        if (!plan.ok) {
            printf("-2\t\t\n");
            continue;
        }
        format_route(plan, route, (int)sizeof route);
        printf("0\t%s\t", route);
        for (int i = 0; i < plan.n_parts; ++i) {
            const LinearPart& p = plan.part[i];
            printf("%sfamily=%s m0=%lld M=%lld grid=%ux%u threads=%u lds=%zu n_tiles=%d m_tiles=%d splits=%d kt_per=%d", i ? " ; " : "", kFamily[p.family],
                   (long long)p.m0, (long long)p.M, p.grid_x, p.grid_y, p.threads, p.lds, p.n_tiles, p.m_tiles, p.splits, p.kt_per);
        }
        printf("\n");
        const std::string bad = check_plan(pr, plan);
        if (!bad.empty()) {
            fflush(stdout);
            fprintf(stderr, "line %ld breaks an invariant: %s\n  %s", lineno, bad.c_str(), line);
            return 1;
        }
    }
    return 0;
}
