// Multi-LoRA (k_lora.hip): adapter slots loaded, committed and unloaded at run time, and the tile list of a step's adapter assignment
// (pplhip_set_adapters).  The step applies them: pplhip.cc layer_lora.
#include "rt_internal.h"

// Tile list of a row -> slot map (-1: no adapter): every assigned row in exactly one tile, a tile's rows share one slot, unassigned rows in
// none.  Slots in ascending order, rows of a slot in ascending order, 16 to a tile, the last tile of a slot padded with -1.
void lora_build_tiles(const int32_t* row_slots, int64_t T, std::vector<LoraTile>& out) {
    int64_t cnt[LORA_MAX_SLOTS] = {0}, first[LORA_MAX_SLOTS];
    for (int64_t m = 0; m < T; ++m) if (row_slots[m] >= 0) ++cnt[row_slots[m]];
    int64_t nt = 0;
    for (int s = 0; s < LORA_MAX_SLOTS; ++s) { first[s] = nt; nt += (cnt[s] + 15) / 16; }
    LoraTile blank;
    blank.slot = 0; blank.n = 0;
    for (int i = 0; i < 16; ++i) blank.row[i] = -1;
    out.assign((size_t)nt, blank);
    int64_t pos[LORA_MAX_SLOTS] = {0};
    for (int64_t m = 0; m < T; ++m) {
        const int s = row_slots[m];
        if (s < 0) continue;
        LoraTile& tl = out[(size_t)(first[s] + pos[s] / 16)];
        tl.slot = s;
        tl.row[tl.n++] = (int32_t)m;
        ++pos[s];
    }
}

// what every adapter entry point refuses: tensor parallelism and quantised activations (include/pplhip.h)
static int lora_guard(pplhip_ctx* c, int rank) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    if (c->tp > 1) return fail(c, rank, PPLHIP_UNSUPPORTED, "LoRA adapters under tensor parallelism (world_size > 1) are not supported");
    if (c->act_fmt != ACT_FP16) return fail(c, rank, PPLHIP_UNSUPPORTED, "LoRA adapters need fp16 activations (act_quant_bit 0): online_i8i8 / online_f8f8 keep no fp16 input of the linears");
    return 0;
}

// the device buffers every adapter step shares, allocated when the first factor arrives
static int lora_ensure_buffers(pplhip_ctx* c, int rank) {
    Rank& R = c->ranks[rank];
    if (R.lora_tab) return 0;
    const size_t ntab = (size_t)c->d.num_layers * LORA_TARGETS * LORA_MAX_SLOTS;
    const int64_t cap = R.cap_T / 16 + LORA_MAX_SLOTS + 1;
    void *tab = nullptr, *tiles = nullptr, *t = nullptr;
    hipError_t e = hipMalloc(&tab, ntab * sizeof(LoraSlot));
    if (e == hipSuccess) e = hipMemset(tab, 0, ntab * sizeof(LoraSlot));
    if (e == hipSuccess) e = hipMalloc(&tiles, (size_t)cap * sizeof(LoraTile));
    if (e == hipSuccess) e = hipMalloc(&t, (size_t)cap * 16 * LORA_MAX_RANK * 2);
    if (e == hipSuccess) e = R.st_lora_tiles.allocate((size_t)cap * sizeof(LoraTile));   // (last: all or nothing itself)
    if (e != hipSuccess) {
        if (tab) hipFree(tab);
        if (tiles) hipFree(tiles);
        if (t) hipFree(t);
        (void)hipGetLastError();
        return fail(c, rank, PPLHIP_OUT_OF_MEMORY, std::string("adapter buffers: ") + hipGetErrorString(e));
    }
    R.lora_tab = (LoraSlot*)tab; R.lora_tiles = (LoraTile*)tiles; R.lora_t = (uint16_t*)t;
    R.lora_tile_cap = cap;
    R.lora_tab_host.assign(ntab, LoraSlot{nullptr, nullptr, 0, 0.f});
    R.lora_touch.assign((size_t)c->d.num_layers * LORA_TARGETS, 0);
    return 0;
}

static void lora_free_slot(Rank& R, int slot) {
    LoraAdapter& ad = R.lora[slot];
    for (auto& f : ad.f) { if (f.a) hipFree(f.a); if (f.b) hipFree(f.b); }
    ad.f.clear();
    if (ad.committed) --R.lora_committed;
    ad.committed = false;
    ad.scale = 0.f;
}

// the slot's column of the kernels' table, on the host mirror and the device (the stream is idle: nothing reads the table meanwhile)
static int lora_publish_slot(pplhip_ctx* c, int rank, int slot) {
    Rank& R = c->ranks[rank];
    const LoraAdapter& ad = R.lora[slot];
    const size_t n = (size_t)c->d.num_layers * LORA_TARGETS;
    for (size_t i = 0; i < n; ++i) {
        LoraSlot e{nullptr, nullptr, 0, 0.f};
        if (ad.committed && ad.f[i].a) e = LoraSlot{ad.f[i].a, ad.f[i].b, (ad.f[i].ra + 15) / 16 * 16, ad.scale};
        R.lora_tab_host[i * LORA_MAX_SLOTS + slot] = e;
    }
    HIPCK(c, rank, hipMemcpy(R.lora_tab, R.lora_tab_host.data(), R.lora_tab_host.size() * sizeof(LoraSlot), hipMemcpyHostToDevice));
    return 0;
}

int pplhip_lora_set_tensor(pplhip_ctx* c, int rank, int slot, const char* name, const void* data, uint64_t bytes, int32_t r) {
    if (int rc = lora_guard(c, rank)) return rc;
    if (!name || !data) return PPLHIP_INVALID_VALUE;
    if (slot < 0 || slot >= LORA_MAX_SLOTS) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " out of range");
    if (r < 1 || r > LORA_MAX_RANK) return fail(c, rank, PPLHIP_INVALID_VALUE, std::string(name) + ": rank " + std::to_string(r) + " outside 1 .. " + std::to_string(LORA_MAX_RANK));
    Rank& R = c->ranks[rank];
    int l = -1;
    char rest[128];
    if (sscanf(name, "layers.%d.%127s", &l, rest) != 2 || l < 0 || l >= c->d.num_layers) return fail(c, rank, PPLHIP_NOT_FOUND, std::string("unknown adapter tensor ") + name);
    if (!strncmp(rest, "feed_forward.w13.", 17))
        return fail(c, rank, PPLHIP_UNSUPPORTED, std::string(name) + ": adapters on feed_forward.w13 (gate / up) are not supported, the fused SwiGLU epilogue never materialises them");
    Layer& L = R.layers[l];
    struct { const char* n; Linear* lin; } tab[LORA_TARGETS] = {{"attention.wqkv.", &L.wqkv}, {"attention.wo.", &L.wo}, {"feed_forward.w2.", &L.w2}};
    int target = -1, is_b = -1;
    for (int i = 0; i < LORA_TARGETS; ++i) {
        const size_t nl = strlen(tab[i].n);
        if (strncmp(rest, tab[i].n, nl)) continue;
        if (!strcmp(rest + nl, "lora_a")) { target = i; is_b = 0; }
        if (!strcmp(rest + nl, "lora_b")) { target = i; is_b = 1; }
    }
    if (target < 0) return fail(c, rank, PPLHIP_NOT_FOUND, std::string("unknown adapter tensor ") + name);
    const Linear& lin = *tab[target].lin;
    if (lin.Kp % 32 || lin.N % 16) return fail(c, rank, PPLHIP_UNSUPPORTED, std::string(name) + ": the adapter kernels need K % 32 == 0 and N % 16 == 0");
    const uint64_t want = is_b ? (uint64_t)lin.N * r * 2 : (uint64_t)r * lin.K * 2;
    if (bytes != want) return fail(c, rank, PPLHIP_INVALID_VALUE, std::string("tensor ") + name + ": got " + std::to_string(bytes) + " bytes, want " + std::to_string(want));
    LoraAdapter& ad = R.lora[slot];
    if (ad.committed) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " is committed: unload it first");
    HIPCK(c, rank, hipSetDevice(R.device));
    if (int rc = lora_ensure_buffers(c, rank)) return rc;
    if (ad.f.empty()) ad.f.resize((size_t)c->d.num_layers * LORA_TARGETS);
    LoraFactor& f = ad.f[(size_t)l * LORA_TARGETS + target];
    const int rp = (r + 15) / 16 * 16;
    // zero-padded on the device: A [rp, Kp] (rows past r and columns past K zero), B [N, rp] (columns past r zero)
    const size_t pitch = is_b ? (size_t)rp * 2 : (size_t)lin.Kp * 2, rows = is_b ? (size_t)lin.N : (size_t)rp;
    const size_t src_pitch = is_b ? (size_t)r * 2 : (size_t)lin.K * 2, src_rows = is_b ? (size_t)lin.N : (size_t)r;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, pitch * rows);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, rank, PPLHIP_OUT_OF_MEMORY, std::string("tensor ") + name + ": " + hipGetErrorString(e)); }
    e = hipMemset(p, 0, pitch * rows);
    if (e == hipSuccess) e = hipMemcpy2D(p, pitch, data, src_pitch, src_pitch, src_rows, hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(p); return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, std::string("tensor ") + name + ": " + hipGetErrorString(e)); }
    uint16_t*& dst = is_b ? f.b : f.a;
    if (dst) hipFree(dst);
    dst = (uint16_t*)p;
    (is_b ? f.rb : f.ra) = r;
    return 0;
}

int pplhip_lora_commit(pplhip_ctx* c, int rank, int slot, float scale) {
    if (int rc = lora_guard(c, rank)) return rc;
    if (slot < 0 || slot >= LORA_MAX_SLOTS) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " out of range");
    Rank& R = c->ranks[rank];
    LoraAdapter& ad = R.lora[slot];
    if (ad.committed) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " is committed already");
    if (!std::isfinite(scale)) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter scale is not finite");
    int pairs = 0;
    for (size_t i = 0; i < ad.f.size(); ++i) {
        const LoraFactor& f = ad.f[i];
        if (!f.a && !f.b) continue;
        const std::string where = "layer " + std::to_string(i / LORA_TARGETS) + " target " + std::to_string(i % LORA_TARGETS);
        if (!f.a || !f.b) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + ": " + where + " has one factor of two");
        if (f.ra != f.rb) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + ": " + where + " has factors of ranks " + std::to_string(f.ra) + " and " + std::to_string(f.rb));
        ++pairs;
    }
    if (!pairs) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " holds no factors");
    HIPCK(c, rank, hipSetDevice(R.device));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    ad.committed = true;
    ad.scale = scale;
    ++R.lora_committed;
    const int rc = lora_publish_slot(c, rank, slot);
    if (rc) {   // the device table did not take it: not committed, and the host mirror names none of its factors
        ad.committed = false;
        --R.lora_committed;
        for (size_t i = 0; i < ad.f.size(); ++i) R.lora_tab_host[i * LORA_MAX_SLOTS + slot] = LoraSlot{nullptr, nullptr, 0, 0.f};
    }
    return rc;
}

int pplhip_lora_unload(pplhip_ctx* c, int rank, int slot) {
    if (int rc = lora_guard(c, rank)) return rc;
    if (slot < 0 || slot >= LORA_MAX_SLOTS) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " out of range");
    Rank& R = c->ranks[rank];
    if (R.lora[slot].f.empty()) return fail(c, rank, PPLHIP_NOT_FOUND, "adapter slot " + std::to_string(slot) + " is not loaded");
    HIPCK(c, rank, hipSetDevice(R.device));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    const bool was = R.lora[slot].committed;
    lora_free_slot(R, slot);
    if (R.lora_ntiles > 0) { R.lora_ntiles = 0; R.lora_stale = true; }
    return was ? lora_publish_slot(c, rank, slot) : 0;
}

// container: pplhip_rank_load's, with the adapter names and lora.scale (fp32 [1]); the rank of a factor follows from its size
int pplhip_lora_load(pplhip_ctx* c, int rank, int slot, const char* dir) {
    if (int rc = lora_guard(c, rank)) return rc;
    if (!dir) return PPLHIP_INVALID_VALUE;
    if (slot < 0 || slot >= LORA_MAX_SLOTS) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " out of range");
    Rank& R = c->ranks[rank];
    if (!R.lora[slot].f.empty()) return fail(c, rank, PPLHIP_INVALID_VALUE, "adapter slot " + std::to_string(slot) + " is in use: unload it first");
    const std::string path = std::string(dir) + "/lora.pplhip";
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return fail(c, rank, PPLHIP_NOT_FOUND, "cannot open " + path);
    char magic[8];
    uint32_t count = 0;
    int rc = 0;
    bool have_scale = false;
    float scale = 0.f;
    std::vector<char> buf;
    uint64_t max_bytes = 4;
    for (const Layer& L : R.layers)
        for (const Linear* lin : {&L.wqkv, &L.wo, &L.w2}) max_bytes = std::max<uint64_t>(max_bytes, (uint64_t)LORA_MAX_RANK * std::max(lin->N, lin->K) * 2);
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "PPLHIPW1", 8) || fread(&count, 4, 1, f) != 1) {
        fclose(f);
        return fail(c, rank, PPLHIP_INVALID_VALUE, "bad header in " + path);
    }
    for (uint32_t i = 0; i < count && !rc; ++i) {
        uint32_t nl = 0; uint64_t nb = 0;
        char name[256];
        if (fread(&nl, 4, 1, f) != 1 || nl >= sizeof(name) || fread(name, 1, nl, f) != nl || fread(&nb, 8, 1, f) != 1) { rc = fail(c, rank, PPLHIP_INVALID_VALUE, "truncated container " + path); break; }
        name[nl] = 0;
        const long pos = ftell(f);
        fseek(f, (64 - pos % 64) % 64, SEEK_CUR);
        // (no factor is larger than LORA_MAX_RANK rows or columns of the widest target linear: a corrupt size is refused, not allocated)
        if (nb > max_bytes) { rc = fail(c, rank, PPLHIP_INVALID_VALUE, std::string("tensor ") + name + " in " + path + ": " + std::to_string(nb) + " bytes is larger than any adapter tensor"); break; }
        buf.resize(nb);
        if (fread(buf.data(), 1, nb, f) != nb) { rc = fail(c, rank, PPLHIP_INVALID_VALUE, "truncated container " + path); break; }
        if (!strcmp(name, "lora.scale")) {
            if (nb != 4) { rc = fail(c, rank, PPLHIP_INVALID_VALUE, "lora.scale must be one fp32"); break; }
            memcpy(&scale, buf.data(), 4);
            have_scale = true;
            continue;
        }
        // rank from the size: lora_a is [r, K], lora_b [N, r] of the target linear
        int l = -1;
        char rest[128];
        int64_t unit = 0;
        if (sscanf(name, "layers.%d.%127s", &l, rest) == 2 && l >= 0 && l < c->d.num_layers) {
            const Layer& L = R.layers[l];
            const bool b = strstr(rest, ".lora_b") != nullptr;
            if (!strncmp(rest, "attention.wqkv.", 15)) unit = b ? L.wqkv.N : L.wqkv.K;
            else if (!strncmp(rest, "attention.wo.", 13)) unit = b ? L.wo.N : L.wo.K;
            else if (!strncmp(rest, "feed_forward.w2.", 16)) unit = b ? L.w2.N : L.w2.K;
        }
        const int64_t r = unit > 0 && nb % (uint64_t)(unit * 2) == 0 ? (int64_t)(nb / (uint64_t)(unit * 2)) : 1;   // (a wrong size or name: set_tensor says which)
        rc = pplhip_lora_set_tensor(c, rank, slot, name, buf.data(), nb, (int32_t)std::min<int64_t>(r, INT32_MAX));
    }
    fclose(f);
    if (!rc && !have_scale) rc = fail(c, rank, PPLHIP_INVALID_VALUE, path + " has no lora.scale");
    if (!rc) rc = pplhip_lora_commit(c, rank, slot, scale);
    if (rc && !R.lora[slot].f.empty()) {   // nothing half loaded stays behind
        const std::string msg = R.err;
        lora_free_slot(R, slot);
        R.err = msg;
    }
    return rc;
}

int pplhip_set_adapters(pplhip_ctx* c, int rank, const int32_t* slots, int64_t batch) {
    if (int rc = lora_guard(c, rank)) return rc;
    Rank& R = c->ranks[rank];
    if (!slots || batch != R.B) return fail(c, rank, PPLHIP_INVALID_VALUE, "pplhip_set_adapters: one slot per request of the staged step");
    R.lora_ntiles = 0;
    R.lora_stale = false;
    bool any = false;
    for (int64_t b = 0; b < batch; ++b) {
        const int s = slots[b];
        if (s == -1) continue;
        if (s < 0 || s >= LORA_MAX_SLOTS) return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + ": adapter slot " + std::to_string(s) + " out of range");
        if (!R.lora[s].committed) return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + ": adapter slot " + std::to_string(s) + " is not loaded");
        any = true;
    }
    if (!any) return 0;   // exactly the step without adapters
    if (!R.h_seq) return fail(c, rank, PPLHIP_INVALID_VALUE, "pplhip_set_adapters before pplhip_set_inputs");
    std::vector<int32_t> row_slots((size_t)R.T, -1);
    for (int64_t b = 0; b < batch; ++b)
        for (int64_t m = R.h_seq[b]; m < R.h_seq[b + 1]; ++m) row_slots[(size_t)m] = slots[b];   // (seq_starts validated by pplhip_set_inputs)
    std::vector<LoraTile> tiles;
    lora_build_tiles(row_slots.data(), R.T, tiles);
    if ((int64_t)tiles.size() > R.lora_tile_cap) return fail(c, rank, PPLHIP_OTHER_ERROR, "adapter tile list exceeds its buffer");
    std::fill(R.lora_touch.begin(), R.lora_touch.end(), 0);
    for (int64_t b = 0; b < batch; ++b) {
        if (slots[b] < 0) continue;
        const LoraAdapter& ad = R.lora[slots[b]];
        for (size_t i = 0; i < ad.f.size(); ++i) if (ad.f[i].a) R.lora_touch[i] = 1;
    }
    HIPCK(c, rank, hipSetDevice(R.device));
    char* h;
    HIPCK(c, rank, R.st_lora_tiles.begin(&h));
    memcpy(h, tiles.data(), tiles.size() * sizeof(LoraTile));
    HIPCK(c, rank, R.st_lora_tiles.upload(R.lora_tiles, tiles.size() * sizeof(LoraTile), R.stream));
    R.lora_ntiles = (int)tiles.size();
    return 0;
}
