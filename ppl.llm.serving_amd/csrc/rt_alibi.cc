// ALiBi attention, host side (k_attn_alibi.hip has the kernels): the standard slopes -- a pure function, no HIP call --, the operator that
// launches both parts, and the runtime's use of them.  Opt-in: a context that never calls pplhip_alibi allocates, uploads and launches what it
// always did.
#include "rt_internal.h"

namespace pplhip {

// what the ALiBi kernels do not serve; "" when the geometry is supported
static std::string alibi_refusal(int quant_bit, int quant_group, int H, int Hkv, int D) {
    if (D != 128) return "head_dim " + std::to_string(D) + " is not supported under ALiBi (128 only)";
    if (H != Hkv) return "grouped-query attention (" + std::to_string(H) + " heads over " + std::to_string(Hkv) + " KV heads) is not supported under ALiBi";
    const int fmt = kv_format(quant_bit, quant_group, D);
    if (fmt == KV_FP8) return "an fp8 KV cache is not supported under ALiBi (fp16 and int8 group 8 only)";
    if (fmt == KV_I4G32) return "an int4 KV cache is not supported under ALiBi (fp16 and int8 group 8 only)";
    if (!attn_alibi_supported(fmt, H, Hkv, D)) return "this KV cache format is not supported under ALiBi (fp16 and int8 group 8 only)";
    return "";
}

}  // namespace pplhip

static int op_rc(hipError_t e) { return e == hipSuccess ? 0 : (e == hipErrorInvalidValue ? PPLHIP_INVALID_VALUE : PPLHIP_DEVICE_RUNTIME_ERROR); }

// Press et al., as HF builds them: n = the largest power of two <= H; head i < n gets 2^(-8 (i + 1) / n), the remaining H - n heads the odd
// steps of the 2 n series, 2^(-4 (2 t + 1) / n)
int pplhip_op_alibi_slopes(int32_t num_heads, float* host_out) {
    if (num_heads <= 0 || !host_out) return PPLHIP_INVALID_VALUE;
    int n = 1;
    while (2 * n <= num_heads) n *= 2;
    for (int i = 0; i < n; ++i) host_out[i] = (float)exp2(-8.0 * (i + 1) / n);
    for (int t = 0; n + t < num_heads; ++t) host_out[n + t] = (float)exp2(-4.0 * (2 * t + 1) / n);
    return 0;
}

int pplhip_op_attention_alibi(void* stream, const void* qkv, const pplhip_kv_view* kv, const int64_t* seq_starts, const int64_t* start_pos,
                              const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t T, int64_t decoding_batches,
                              int64_t max_seq_len, int64_t max_kv_len, int32_t num_heads, int32_t split_k, void* workspace,
                              uint64_t workspace_bytes, void* out, const float* slopes_device) {
    if (!slopes_device)
        return pplhip_op_attention(stream, qkv, kv, seq_starts, start_pos, cache_indices, max_pages, B, T, decoding_batches, max_seq_len, max_kv_len,
                                   num_heads, split_k, workspace, workspace_bytes, out);
    if (!kv) return PPLHIP_INVALID_VALUE;
    const std::string why = alibi_refusal(kv->quant_bit, kv->quant_group, num_heads, kv->kv_heads, kv->head_dim);   // before any HIP call
    if (!why.empty()) return fail(nullptr, -1, PPLHIP_UNSUPPORTED, "pplhip_op_attention_alibi: " + why);
    const int fmt = kv_format(kv->quant_bit, kv->quant_group, kv->head_dim);
    const int H = num_heads, D = kv->head_dim;
    if (B < 0 || (kv->mode == 1 && (kv->page_size <= 0 || max_pages <= 0))) return PPLHIP_INVALID_VALUE;
    // pplhip_op_attention's routing: the first decoding_batches rows are decode rows, the others prefill or cache-prefill requests
    const int64_t nb = std::min<int64_t>(std::max<int64_t>(decoding_batches, 0), B);
    const int split = split_k < 1 ? 1 : split_k;
    if (split > 1 && nb > 0 && (!workspace || attn_decode_workspace_bytes(nb, H, D, split) > workspace_bytes)) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    const KvAddr a = view_kv_addr(kv);
    hipError_t e = hipSuccess;
    if (nb > 0)
        e = launch_attn_decode_alibi(s, (const uint16_t*)qkv, a, fmt, seq_starts, start_pos, cache_indices, max_pages, nb, H, H, D, split, 256,
                                     (float*)workspace, slopes_device, (uint16_t*)out);
    if (e == hipSuccess && B > nb)
        e = launch_attn_prefill_alibi(s, (const uint16_t*)qkv, a, fmt, seq_starts, start_pos, cache_indices, max_pages, nb, B, H, H, D, max_seq_len,
                                      slopes_device, (uint16_t*)out);
    return op_rc(e);
}

// ---- the runtime's use of it ----------------------------------------------------------------------------------------------------------

int pplhip_alibi(pplhip_ctx* c, const float* slopes_host) {
    if (!c) return PPLHIP_INVALID_VALUE;
    const std::string why = alibi_refusal(c->d.cache_quant_bit, c->d.cache_quant_group, c->d.num_heads, c->d.num_kv_heads, c->D);
    if (!why.empty()) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_alibi: " + why);
    if (c->tp > 1) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_alibi: tensor parallelism (world_size " + std::to_string(c->tp) + ") is not supported under ALiBi");
    if (c->window > 0) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_alibi: a sliding window is set in this context");
    for (const Rank& R : c->ranks)
        if (R.sp_min_rows > 0) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_alibi: shared-prefix detection is on in this context");
    const int H = c->H;
    std::vector<float> slopes((size_t)H);
    if (slopes_host) slopes.assign(slopes_host, slopes_host + H);
    else pplhip_op_alibi_slopes(H, slopes.data());
    for (float v : slopes)
        if (!(v >= 0.f) || std::isinf(v)) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_alibi: a slope is negative or not finite");
    // no rotation: the RoPE/KV-write kernels stay as they are and read a table of cos = 1, sin = 0 -- x 1 - y 0 and y 1 + x 0 are x and y
    // (a zero's sign can change; nothing else does)
    std::vector<float> ident((size_t)c->d.max_position * c->D);
    for (int64_t p = 0; p < c->d.max_position; ++p)
        for (int i = 0; i < c->D; ++i) ident[(size_t)(p * c->D + i)] = i < c->D / 2 ? 1.0f : 0.0f;
    for (int r = 0; r < (int)c->ranks.size(); ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        HIPCK(c, r, hipStreamSynchronize(R.stream));   // (a second call between steps: no launch still reads the old slopes)
        if (!R.alibi_slopes)
            if (int rc = dev_alloc(c, r, (void**)&R.alibi_slopes, (uint64_t)H * sizeof(float))) return rc;
        HIPCK(c, r, hipMemcpy(R.alibi_slopes, slopes.data(), (size_t)H * sizeof(float), hipMemcpyHostToDevice));
        HIPCK(c, r, hipMemcpy(R.rope, ident.data(), ident.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    c->alibi = true;
    return 0;
}

int alibi_attention_decode(pplhip_ctx* c, int rank, Lane& lane, const KvAddr& kv, const pplhip_chunk& k, int split, int threads) {
    Rank& R = c->ranks[rank];
    const int64_t ci_stride = c->d.cache_mode == 1 ? R.max_pages : 1;
    HIPCK(c, rank, launch_attn_decode_alibi(lane.stream, R.qkv, kv, c->kv_fmt, R.d_seq + k.b0, R.d_sp + k.b0, R.d_ci + k.b0 * ci_stride, R.max_pages,
                                            k.nd, c->H, c->Hkv, c->D, split, threads, lane.attn_ws, R.alibi_slopes,
                                            R.att + k.b0 * (int64_t)c->H * c->D));
    return 0;
}

int alibi_attention_prefill(pplhip_ctx* c, int rank, Lane& lane, const KvAddr& kv, const pplhip_chunk& k) {
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, launch_attn_prefill_alibi(lane.stream, R.qkv, kv, c->kv_fmt, R.d_seq, R.d_sp, R.d_ci, R.max_pages, k.b0 + k.nd, k.b0 + k.bn, c->H,
                                             c->Hkv, c->D, R.max_seq_len, R.alibi_slopes, R.att));
    return 0;
}
