// Shared-prefix decode attention, host side (k_attn_decode_shared.hip has the kernels): which decode rows share leading pages, the tile list
// of the shared launch and the shifted page table of the own launch.  Pure functions on host arrays: no HIP call, no context.
#include "rt_internal.h"

namespace pplhip {

int shared_prefix_groups(const int64_t* pages, int64_t max_pages, const int64_t* start_pos, int64_t nb, int page_size, int min_rows,
                         int64_t min_tokens, int32_t* group, int64_t* group_tokens) {
    for (int64_t b = 0; b < nb; ++b) group[b] = -1;
    if (nb <= 0 || max_pages <= 0 || page_size <= 0 || page_size % 16 || min_rows <= 0) return 0;
    // buckets by page 0, in order of their first row: lead row, rows, pages that may be shared (the clamp), pages equal so far
    struct Bucket {
        int64_t lead, rows, clamp, equal;
    };
    std::unordered_map<int64_t, int32_t> by_page0;
    std::vector<Bucket> buckets;
    std::vector<int32_t> bucket_of((size_t)nb);
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t own = std::min<int64_t>(std::max<int64_t>(start_pos[b], 0) / page_size, max_pages);   // full pages in front of the current token's
        const auto it = by_page0.find(pages[b * max_pages]);
        if (it == by_page0.end()) {
            by_page0.emplace(pages[b * max_pages], (int32_t)buckets.size());
            bucket_of[(size_t)b] = (int32_t)buckets.size();
            buckets.push_back(Bucket{b, 1, own, own});
            continue;
        }
        Bucket& k = buckets[(size_t)it->second];
        bucket_of[(size_t)b] = it->second;
        k.rows++;
        k.clamp = std::min(k.clamp, own);
        k.equal = std::min(k.equal, k.clamp);
        const int64_t *x = pages + k.lead * max_pages, *y = pages + b * max_pages;
        int64_t e = 0;
        while (e < k.equal && x[e] == y[e]) ++e;
        k.equal = e;
    }
    int n_groups = 0;
    std::vector<int32_t> id(buckets.size(), -1);
    for (size_t i = 0; i < buckets.size(); ++i) {
        const int64_t P = buckets[i].equal * page_size / 16 * 16;
        if (buckets[i].rows < min_rows || P < std::max<int64_t>(min_tokens, 16) || P > INT32_MAX) continue;
        id[i] = n_groups;
        group_tokens[n_groups++] = P;
    }
    for (int64_t b = 0; b < nb; ++b) group[b] = id[(size_t)bucket_of[(size_t)b]];
    return n_groups;
}

int shared_build_tiles(const int32_t* group, const int64_t* group_tokens, int n_groups, int64_t nb, int grp, SharedTile* out) {
    const int per = 16 / grp;   // requests per tile
    std::vector<int32_t> open((size_t)std::max(n_groups, 0), -1);   // the group's tile that still has room
    int n = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int g = group[b];
        if (g < 0) continue;
        if (open[(size_t)g] < 0) {
            SharedTile& t = out[n];
            t.n = 0; t.tokens = (int32_t)group_tokens[g]; t.lead = (int32_t)b;
            for (int c = 0; c < 16; ++c) t.row[c] = -1;
            open[(size_t)g] = n++;
        }
        SharedTile& t = out[open[(size_t)g]];
        t.lead = (int32_t)b;   // (any member serves: the tile's last one)
        for (int j = 0; j < grp; ++j) t.row[t.n * grp + j] = (int32_t)b;
        if (++t.n == per) open[(size_t)g] = -1;
    }
    // a group's tiles side by side: they read the same keys, and the kernel's grid order runs neighbours on one XCD
    std::stable_sort(out, out + n, [&](const SharedTile& a, const SharedTile& b) { return group[a.lead] < group[b.lead]; });
    return n;
}

int shared_plan_fill(const SharedPlanBlock& h, const int64_t* pages, int64_t max_pages, int64_t nb, int page_size, int grp,
                     const int32_t* group, const int64_t* group_tokens, int n_groups) {
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t P = group[b] >= 0 ? group_tokens[group[b]] : 0;
        const int64_t sh = P / page_size;
        h.row_tokens[b] = (int32_t)P;
        for (int64_t j = 0; j < max_pages; ++j) h.own_pages[b * max_pages + j] = j + sh < max_pages ? pages[b * max_pages + j + sh] : 0;
    }
    return shared_build_tiles(group, group_tokens, n_groups, nb, grp, h.tiles);
}

}  // namespace pplhip

// ---- the runtime's use of it ----------------------------------------------------------------------------------------------------------

int pplhip_shared_prefix(pplhip_ctx* c, int32_t min_rows, int64_t min_tokens) {
    if (!c || min_rows < 0 || min_tokens < 0) return PPLHIP_INVALID_VALUE;
    if (min_rows > 0 && !attn_shared_supported(c->kv_fmt, c->d.cache_mode, c->d.page_size, c->H, c->Hkv, c->D)) return PPLHIP_UNSUPPORTED;
    if (min_rows > 0 && c->window > 0) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_shared_prefix: a sliding window is set in this context");
    if (min_rows > 0 && c->alibi) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_shared_prefix: this context runs under ALiBi");
    for (int r = 0; r < (int)c->ranks.size(); ++r) {
        Rank& R = c->ranks[r];
        if (min_rows > 0 && !R.sp_ws) {   // everything whose size max_running_batch decides; the plan block follows the page-table width
            HIPCK(c, r, hipSetDevice(R.device));
            if (int rc = dev_alloc(c, r, (void**)&R.sp_ws, (uint64_t)R.cap_B * c->H * SP_SPLIT_MAX * (c->D + 2) * 4)) return rc;
            for (Stage& st : R.st_sp_pos) HIPCK(c, r, st.allocate((size_t)R.cap_B * 8));
        }
        R.sp_min_rows = min_rows;
        R.sp_min_tokens = min_tokens;
        R.sp_dirty = true;   // (groups are formed with the next run)
        R.sp_chunk[0] = R.sp_chunk[1] = Rank::SpChunk{};
        R.sp_last[0] = R.sp_last[1] = R.sp_last[2] = 0;
    }
    return 0;
}

int pplhip_shared_prefix_info(pplhip_ctx* c, int rank, int64_t* groups, int64_t* rows_in_groups, int64_t* shared_tokens) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    const Rank& R = c->ranks[rank];
    if (groups) *groups = R.sp_last[0];
    if (rows_in_groups) *rows_in_groups = R.sp_last[1];
    if (shared_tokens) *shared_tokens = R.sp_last[2];
    return 0;
}

void shared_prefix_release(Rank& R) {
    for (Stage* st : {&R.st_sp_pos[0], &R.st_sp_pos[1], &R.st_sp_plan[0], &R.st_sp_plan[1]}) st->release();
    if (R.sp_dev) (void)hipFree(R.sp_dev);
    R.sp_dev = nullptr;
    R.sp_cap = 0;
}

void shared_prefix_stage(Rank& R, const pplhip_step* st) {
    R.sp_start_pos.assign(st->start_pos, st->start_pos + st->batch);
    if (st->req_list_changed) R.sp_dirty = true;
}

const Rank::SpChunk* shared_prefix_chunk(const pplhip_ctx* c, const Rank& R, const pplhip_chunk& k, int split, size_t attn_ws_bytes) {
    if (R.sp_min_rows <= 0 || k.nd <= 0) return nullptr;
    // (the own launch runs at split >= 2; a lane whose workspace cannot hold that keeps the ordinary path -- not with the sizes the runtime
    // allocates: 32 splits of every row)
    if (attn_decode_workspace_bytes(k.nd, c->H, c->D, std::max(split, 2)) > attn_ws_bytes) return nullptr;
    for (const Rank::SpChunk& sc : R.sp_chunk)
        if (sc.n_groups > 0 && sc.b0 == k.b0 && sc.nd == k.nd) return &sc;
    return nullptr;
}

static uint64_t up256(uint64_t v) { return (v + 255) / 256 * 256; }

int shared_prefix_plan(pplhip_ctx* c, int rank, const pplhip_step_plan& p) {
    Rank& R = c->ranks[rank];
    R.sp_last[0] = R.sp_last[1] = R.sp_last[2] = 0;
    if (R.sp_min_rows <= 0 || !R.pages_host || R.max_pages <= 0 || (int64_t)R.sp_start_pos.size() != R.B) return 0;
    const int64_t B = R.B, mp = R.max_pages;
    int64_t b0[2] = {0, 0}, nd[2] = {0, 0};
    bool same = !R.sp_dirty && (int64_t)R.sp_row_tokens.size() == B;   // (another batch size without a changed list: regroup)
    for (int i = 0; i < 2; ++i) {
        if (i < p.num_chunks) { b0[i] = p.chunk[i].b0; nd[i] = p.chunk[i].nd; }
        same = same && R.sp_chunk[i].b0 == b0[i] && R.sp_chunk[i].nd == nd[i];
    }
    const uint64_t pos_bytes = up256((uint64_t)B * 8);
    if (same) {   // the groups stand: this step's shifted positions alone
        if (R.sp_chunk[0].n_groups + R.sp_chunk[1].n_groups == 0) return 0;
        Stage& stage = R.st_sp_pos[R.st_sp_cur];
        R.st_sp_cur ^= 1;
        char* buf;
        HIPCK(c, rank, stage.begin(&buf));
        int64_t* own = (int64_t*)buf;
        for (int64_t b = 0; b < B; ++b) {
            own[b] = R.sp_start_pos[(size_t)b] - R.sp_row_tokens[(size_t)b];
            if (own[b] < 0) same = false;   // a position in front of the shared keys: not the requests the groups were formed over
        }
        if (same) HIPCK(c, rank, stage.upload(R.sp_dev, (size_t)B * 8, R.stream));
    }
    if (!same) {
        R.sp_row_tokens.assign((size_t)B, 0);
        std::vector<int32_t> group[2];
        std::vector<int64_t> tokens[2];
        uint64_t total = pos_bytes;
        for (int i = 0; i < 2; ++i) {
            Rank::SpChunk& sc = R.sp_chunk[i];
            sc = Rank::SpChunk{};
            sc.b0 = b0[i]; sc.nd = nd[i];
            if (nd[i] < R.sp_min_rows) continue;
            group[i].resize((size_t)nd[i]);
            tokens[i].resize((size_t)nd[i]);
            sc.n_groups = shared_prefix_groups(R.pages_host + b0[i] * mp, mp, R.sp_start_pos.data() + b0[i], nd[i], c->d.page_size, R.sp_min_rows,
                                               R.sp_min_tokens, group[i].data(), tokens[i].data());
            if (sc.n_groups == 0) continue;
            sc.off = total;
            total += up256(SharedPlanBlock(nullptr, nd[i], mp).bytes);
        }
        R.sp_dirty = false;
        if (R.sp_chunk[0].n_groups + R.sp_chunk[1].n_groups == 0) return 0;
        if (total > R.sp_cap) {   // (rare: a wider page table or a larger batch; hipFree waits for the launches that read the old block)
            for (Stage& s2 : R.st_sp_plan) s2.release();
            if (R.sp_dev) (void)hipFree(R.sp_dev);
            R.sp_dev = nullptr;
            R.sp_cap = 0;
            HIPCK(c, rank, hipMalloc((void**)&R.sp_dev, total * 2));
            for (Stage& s2 : R.st_sp_plan) HIPCK(c, rank, s2.allocate((size_t)total * 2));
            R.sp_cap = total * 2;
        }
        Stage& stage = R.st_sp_plan[R.st_sp_plan_cur];
        R.st_sp_plan_cur ^= 1;
        char* img;
        HIPCK(c, rank, stage.begin(&img));
        for (int i = 0; i < 2; ++i) {
            Rank::SpChunk& sc = R.sp_chunk[i];
            if (sc.n_groups == 0) continue;
            const SharedPlanBlock h(img + sc.off, sc.nd, mp);
            sc.ntiles = shared_plan_fill(h, R.pages_host + sc.b0 * mp, mp, sc.nd, c->d.page_size, c->H / c->Hkv, group[i].data(), tokens[i].data(),
                                         sc.n_groups);
            for (int64_t b = 0; b < sc.nd; ++b) {
                R.sp_row_tokens[(size_t)(sc.b0 + b)] = h.row_tokens[b];
                sc.rows += group[i][(size_t)b] >= 0;
            }
            for (int g = 0; g < sc.n_groups; ++g) sc.tokens += tokens[i][(size_t)g];
        }
        int64_t* own = (int64_t*)img;
        for (int64_t b = 0; b < B; ++b) own[b] = R.sp_start_pos[(size_t)b] - R.sp_row_tokens[(size_t)b];   // >= 1: the grouping rule's clamp
        HIPCK(c, rank, stage.upload(R.sp_dev, (size_t)total, R.stream));
    }
    for (const Rank::SpChunk& sc : R.sp_chunk) {
        R.sp_last[0] += sc.n_groups; R.sp_last[1] += sc.rows; R.sp_last[2] += sc.tokens;
    }
    return 0;
}

int shared_prefix_attention(pplhip_ctx* c, int rank, Lane& lane, const KvAddr& kv, const Rank::SpChunk& sc, int split, int threads) {
    Rank& R = c->ranks[rank];
    const int H = c->H, Hkv = c->Hkv, D = c->D;
    const int own_split = std::max(split, 2);   // the own launch leaves partial rows for the merge
    const SharedPlanBlock d(R.sp_dev + sc.off, sc.nd, R.max_pages);
    const int64_t* own_pos = (const int64_t*)R.sp_dev + sc.b0;
    float* ws_shared = R.sp_ws + sc.b0 * (int64_t)H * SP_SPLIT_MAX * (D + 2);
    uint16_t* out = R.att + sc.b0 * (int64_t)H * D;
    // enough work items for the chip (256 CUs, two blocks each) where the tiles alone are few
    const int64_t base = (int64_t)Hkv * sc.ntiles;
    const int shared_split = (int)std::min<int64_t>(std::max<int64_t>((512 + base - 1) / base, 1), SP_SPLIT_MAX);
    hipStream_t s = lane.stream;
    // (the per-request arrays shifted to the chunk, as the ordinary launch takes them; the tiles' rows count from the chunk's first row)
    HIPCK(c, rank, launch_attn_decode(s, R.qkv, kv, c->kv_fmt, R.d_seq + sc.b0, own_pos, d.own_pages, R.max_pages, sc.nd, H, Hkv, D, R.max_kv_len,
                                      own_split, threads, lane.attn_ws, out, nullptr, nullptr, /*reduce=*/false));
    HIPCK(c, rank, launch_attn_decode_shared(s, R.qkv, kv, c->kv_fmt, R.d_seq + sc.b0, R.d_ci + sc.b0 * R.max_pages, R.max_pages, d.tiles, sc.ntiles,
                                             H, Hkv, D, shared_split, ws_shared));
    HIPCK(c, rank, launch_attn_shared_merge(s, lane.attn_ws, own_split, ws_shared, shared_split, d.row_tokens, sc.nd, H, D, out));
    return 0;
}

