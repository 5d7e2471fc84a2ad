// QKV bias and per-head QK-norm (Qwen2 / Qwen3; pplhip_qkv_prologue; kernel: k_rope_prologue.hip, operator: rt_ops.cc).  Opt-in: a context that never calls
// pplhip_qkv_prologue allocates and launches what it always did.  With it on, every Layer::pro names the layer's bias and / or norm weights and
// layer_attention_part (pplhip.cc) launches launch_rope_kv_prologue with it in place of launch_rope_kv_write.
#include "rt_internal.h"

int pplhip_qkv_prologue(pplhip_ctx* c, int32_t qkv_bias, int32_t qk_norm, float eps) {
    if (!c || (!qkv_bias && !qk_norm)) return PPLHIP_INVALID_VALUE;
    if (c->qkv_prologue) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_qkv_prologue: already called");
    if (c->weights_touched) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_qkv_prologue: call it before any weight is loaded");
    const int D = c->D;
    if (qk_norm && (D < 32 || (D & (D - 1)) || !(eps >= 0.f)))
        return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_qkv_prologue: the head norm needs a head_dim that is a power of two >= 32 (got " +
                                                     std::to_string(D) + ") and eps >= 0");
    const uint64_t bias_bytes = (uint64_t)(c->H + 2 * c->Hkv) * D * 2;
    const std::vector<uint16_t> ones((size_t)D, 0x3c00u);
    for (int r = 0; r < (int)c->ranks.size(); ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        for (Layer& L : R.layers) {
            // (a failure leaves Layer::pro partly filled and the switch off: nothing reads it, pplhip_destroy frees what dev_alloc took)
            if (qkv_bias) {
                if (int rc = dev_alloc(c, r, (void**)&L.pro.bias, bias_bytes)) return rc;
                HIPCK(c, r, hipMemset((void*)L.pro.bias, 0, bias_bytes));
            }
            if (qk_norm) {
                for (const uint16_t** w : {&L.pro.q_norm, &L.pro.k_norm}) {
                    if (int rc = dev_alloc(c, r, (void**)w, (uint64_t)D * 2)) return rc;
                    HIPCK(c, r, hipMemcpy((void*)*w, ones.data(), (size_t)D * 2, hipMemcpyHostToDevice));
                }
                L.pro.eps = eps;
            }
        }
    }
    c->qkv_prologue = true;
    return 0;
}

bool qkv_prologue_find_tensor(const pplhip_ctx* c, const Layer& L, const char* rest, void** ptr, uint64_t* bytes) {
    const struct { const char* n; const uint16_t* p; uint64_t bytes; } tab[] = {
        {"attention.wqkv.bias", L.pro.bias, (uint64_t)(c->H + 2 * c->Hkv) * c->D * 2},
        {"attention.q_norm.weight", L.pro.q_norm, (uint64_t)c->D * 2},
        {"attention.k_norm.weight", L.pro.k_norm, (uint64_t)c->D * 2}};
    for (const auto& t : tab)
        if (t.p && !strcmp(rest, t.n)) { *ptr = (void*)t.p; *bytes = t.bytes; return true; }
    return false;
}
