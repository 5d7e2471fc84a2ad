// Mixture-of-experts models (pplhip_moe; kernels: k_moe.hip).  Opt-in: a context that never calls pplhip_moe allocates and launches what it
// always did.  With it on, Layer::w13 / w2 describe ONE expert and point at E of them stacked (expert j at j * alloc_bytes(), its scales at
// j * N), Layer::moe_gate is the router matrix, and the feed-forward block of a chunk is launch_moe_ffn (moe_ffn_part, called by pplhip.cc).
#include "rt_internal.h"

static void release_alloc(Rank& R, void* p) {
    if (!p) return;
    R.allocs.erase(std::remove(R.allocs.begin(), R.allocs.end(), p), R.allocs.end());
    (void)hipFree(p);
}

// what a layer gets in place of its dense pair: E stacked copies of each Linear's shape (zeroed where w2's K is padded, like linear_alloc)
struct MoeLayerAlloc {
    void *w13 = nullptr, *s13 = nullptr, *w2 = nullptr, *s2 = nullptr, *gate = nullptr;
};

int pplhip_moe(pplhip_ctx* c, int32_t num_experts, int32_t experts_per_token) {
    if (!c || num_experts < 1 || experts_per_token < 1) return PPLHIP_INVALID_VALUE;
    const int E = num_experts, k = experts_per_token;
    auto refuse = [&](const std::string& why) { return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_moe: " + why); };
    if (c->moe_E) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_moe: already called");
    if (c->weights_touched) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_moe: call it before any weight is loaded");
    if (E > MOE_MAX_EXPERTS) return refuse(std::to_string(E) + " experts, at most " + std::to_string(MOE_MAX_EXPERTS) + " (a router logit per lane of a wave)");
    if (k > MOE_MAX_TOP_K) return refuse(std::to_string(k) + " experts per token, at most " + std::to_string(MOE_MAX_TOP_K));
    if (k > E) return refuse(std::to_string(k) + " experts per token of " + std::to_string(E));
    if (c->d.weight_quant_bit == 4) return refuse("W4A16 experts are not supported (fp16 or W8A16)");
    if (c->act_fmt != ACT_FP16) return refuse("online_i8i8 / online_f8f8 activations are not supported");
    if (c->tp > 1 || c->emulate_tp) return refuse("tensor parallelism (world_size > 1) is not supported");
    if (c->d.hidden_dim % 64) return refuse("hidden_dim must be a multiple of 64");
    for (Rank& R : c->ranks)
        for (const LoraAdapter& ad : R.lora)
            for (size_t i = 0; i < ad.f.size(); ++i)
                if (i % LORA_TARGETS == LORA_W2 && (ad.f[i].a || ad.f[i].b)) return refuse("an adapter on feed_forward.w2 is loaded");
    // All or nothing: everything new is allocated beside the dense tensors first; only when all of it exists are the dense pairs released
    // and the layers repointed.  A failure frees what was allocated and leaves the context the dense one it was.
    std::vector<std::vector<MoeLayerAlloc>> fresh(c->ranks.size());
    std::vector<void*> ws(c->ranks.size(), nullptr);
    hipError_t e = hipSuccess;
    int bad = 0;
    for (int r = 0; r < (int)c->ranks.size() && e == hipSuccess; ++r) {
        Rank& R = c->ranks[r];
        bad = r;
        if ((e = hipSetDevice(R.device)) != hipSuccess) break;
        fresh[r].resize(R.layers.size());
        auto take = [&](void** p, uint64_t bytes) { if (e == hipSuccess && bytes) e = hipMalloc(p, bytes); };
        for (size_t l = 0; l < R.layers.size() && e == hipSuccess; ++l) {
            const Layer& L = R.layers[l];
            MoeLayerAlloc& a = fresh[r][l];
            take(&a.w13, (uint64_t)E * L.w13.alloc_bytes());
            take(&a.s13, (uint64_t)E * L.w13.s_bytes());
            take(&a.w2, (uint64_t)E * L.w2.alloc_bytes());
            take(&a.s2, (uint64_t)E * L.w2.s_bytes());
            take(&a.gate, (uint64_t)E * c->d.hidden_dim * 2);
            if (e == hipSuccess && L.w2.Kp != L.w2.K) e = hipMemset(a.w2, 0, (uint64_t)E * L.w2.alloc_bytes());
        }
        take(&ws[r], moe_ffn_workspace_bytes(R.cap_T, E, k, c->d.hidden_dim, c->inter));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (auto& per_rank : fresh)
            for (MoeLayerAlloc& a : per_rank)
                for (void* p : {a.w13, a.s13, a.w2, a.s2, a.gate}) if (p) (void)hipFree(p);
        for (void* p : ws) if (p) (void)hipFree(p);
        return fail(c, bad, e == hipErrorOutOfMemory ? PPLHIP_OUT_OF_MEMORY : PPLHIP_DEVICE_RUNTIME_ERROR, std::string("pplhip_moe: ") + hipGetErrorString(e));
    }
    for (int r = 0; r < (int)c->ranks.size(); ++r) {
        Rank& R = c->ranks[r];
        (void)hipSetDevice(R.device);
        for (size_t l = 0; l < R.layers.size(); ++l) {
            Layer& L = R.layers[l];
            const MoeLayerAlloc& a = fresh[r][l];
            for (void* p : {L.w13.w, (void*)L.w13.scale, L.w2.w, (void*)L.w2.scale}) release_alloc(R, p);
            L.w13.w = a.w13; L.w13.scale = (uint16_t*)a.s13; L.w2.w = a.w2; L.w2.scale = (uint16_t*)a.s2; L.moe_gate = (uint16_t*)a.gate;
            for (void* p : {a.w13, a.s13, a.w2, a.s2, a.gate}) if (p) R.allocs.push_back(p);
        }
        R.moe_ws = ws[r];
        R.allocs.push_back(ws[r]);
        R.moe_counts_clean = false;
    }
    // one workspace per rank: a step's chunks never run side by side (the two-lane decode schedule is for link time, and there is none)
    c->dual_mode = 0;
    c->dual_auto = false;
    c->moe_E = E;
    c->moe_k = k;
    return 0;
}

// "feed_forward.gate.weight", "feed_forward.experts.J.w13|w2.weight|scale" of layer L -> the device range; *lin: the expert's view
bool moe_find_tensor(pplhip_ctx* c, Rank& R, Layer& L, const char* rest, void** ptr, uint64_t* bytes, Linear** lin) {
    if (!strcmp(rest, "feed_forward.gate.weight")) { *ptr = L.moe_gate; *bytes = (uint64_t)c->moe_E * c->d.hidden_dim * 2; return true; }
    int j = -1;
    char tail[32];
    if (sscanf(rest, "feed_forward.experts.%d.%31s", &j, tail) != 2 || j < 0 || j >= c->moe_E) return false;
    const Linear* base = !strncmp(tail, "w13.", 4) ? &L.w13 : (!strncmp(tail, "w2.", 3) ? &L.w2 : nullptr);
    if (!base) return false;
    const char* kind = strchr(tail, '.') + 1;
    R.moe_view = *base;
    R.moe_view.w = (char*)base->w + (uint64_t)j * base->alloc_bytes();
    R.moe_view.scale = base->scale ? base->scale + (uint64_t)j * base->N : nullptr;
    if (!strcmp(kind, "weight")) { *ptr = R.moe_view.w; *bytes = base->w_bytes(); if (lin) *lin = &R.moe_view; return true; }
    if (!strcmp(kind, "scale") && base->qbit) { *ptr = R.moe_view.scale; *bytes = base->s_bytes(); return true; }
    return false;
}

// the feed-forward block of a chunk's tn rows (normed rows xn) -> part2 rows, written in full: no deferred split-K slabs
int moe_ffn_part(pplhip_ctx* c, int rank, Lane& lane, const Layer& L, const uint16_t* xn, int64_t tn, uint16_t* out) {
    Rank& R = c->ranks[rank];
    const int hd = c->d.hidden_dim;
    HIPCK(c, rank, launch_moe_ffn(lane.stream, xn, L.moe_gate, L.w13.w, L.w13.scale, L.w2.w, L.w2.scale, L.w13.qbit, tn, c->moe_E, c->moe_k, hd,
                                  c->inter, R.moe_ws, R.moe_counts_clean, out, hd));
    R.moe_counts_clean = true;   // (the bucket kernel leaves the counts zeroed for the next launch)
    return 0;
}
