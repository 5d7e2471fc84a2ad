// Sliding-window attention, host side (k_attn_window.hip has the kernels): the shifted positions, slots / page table and skips of the decode
// rows -- a pure function on host arrays, no HIP call, no context --, the operator that launches both parts, and the runtime's use of them.
#include "rt_internal.h"

namespace pplhip {

int64_t window_shift(const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t nb, int cache_mode, int page_size,
                     int64_t window, int64_t* pos_out, int64_t* table_out, int32_t* skip_out, int64_t* max_kv_len_out) {
    const int64_t ps = cache_mode == 1 ? page_size : 1;
    int64_t width = 1, max_kv = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t f = std::max<int64_t>(start_pos[b] - window + 1, 0);   // the row's first key
        const int64_t base = f / ps * ps;                                    // where its shifted table can start
        pos_out[b] = start_pos[b] - base;
        skip_out[b] = (int32_t)(f - base);
        max_kv = std::max(max_kv, pos_out[b] + 1);
        if (cache_mode == 1) width = std::max(width, pos_out[b] / ps + 1);
    }
    if (max_kv_len_out) *max_kv_len_out = max_kv;
    if (!table_out) return width;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t first = (start_pos[b] - pos_out[b]) / ps;   // pages (slots) in front of the shifted table
        if (cache_mode != 1) {
            table_out[b] = cache_indices[b] + first;
            continue;
        }
        for (int64_t j = 0; j < width; ++j) table_out[b * width + j] = first + j < max_pages ? cache_indices[b * max_pages + first + j] : 0;
    }
    return width;
}

// device image of the shifted decode arrays: positions | table [nb, width] | skips
struct WindowBlock : Packed {
    int64_t *pos, *table;
    int32_t* skip;
    WindowBlock(void* base, int64_t nb, int64_t width) : Packed(base) {
        pos = col<int64_t>(nb);
        table = col<int64_t>(nb * width);
        skip = col<int32_t>(nb);
    }
};

// what neither the band kernel nor the WIN decode kernels serve; "" when the geometry is supported
static std::string window_refusal(int quant_bit, int quant_group, int head_dim) {
    if (head_dim != 128) return "head_dim " + std::to_string(head_dim) + " is not supported under a sliding window (128 only)";
    const int fmt = kv_format(quant_bit, quant_group, head_dim);
    if (fmt == KV_FP8) return "an fp8 KV cache is not supported under a sliding window (fp16 and int8 group 8 only)";
    if (fmt == KV_I4G32) return "an int4 KV cache is not supported under a sliding window (fp16 and int8 group 8 only)";
    if (!attn_window_supported(fmt, head_dim)) return "this KV cache format is not supported under a sliding window (fp16 and int8 group 8 only)";
    return "";
}

// decode rows [0, nb) through the shifted arrays of `d`: the ordinary launch on a contiguous cache, the WIN kernels on a paged one
static hipError_t window_decode(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int fmt, const int64_t* seq_starts, const WindowBlock& d,
                                int64_t width, int64_t nb, int H, int Hkv, int D, int64_t max_kv, int split, int threads, float* ws, uint16_t* out,
                                hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    if (kv.mode != 1) return launch_attn_decode(s, qkv, kv, fmt, seq_starts, d.pos, d.table, 1, nb, H, Hkv, D, max_kv, split, threads, ws, out, t0, t1);
    return launch_attn_decode_window(s, qkv, kv, fmt, seq_starts, d.pos, d.table, width, d.skip, nb, H, Hkv, D, split, threads, ws, out);
}

}  // namespace pplhip

static uint64_t up256(uint64_t v) { return (v + 255) / 256 * 256; }
static int op_rc(hipError_t e) { return e == hipSuccess ? 0 : (e == hipErrorInvalidValue ? PPLHIP_INVALID_VALUE : PPLHIP_DEVICE_RUNTIME_ERROR); }

int pplhip_op_window_shift(const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t decoding_batches,
                           int32_t cache_mode, int32_t page_size, int32_t window, int64_t* pos_out, int64_t* table_out, int64_t* table_width,
                           int32_t* skip_out, int64_t* max_kv_len_out) {
    if (!start_pos || !cache_indices || !pos_out || !table_out || !table_width || !skip_out || decoding_batches < 0 || window < 1 ||
        (cache_mode != 0 && cache_mode != 1) || (cache_mode == 1 && (page_size <= 0 || max_pages <= 0)))
        return PPLHIP_INVALID_VALUE;
    for (int64_t b = 0; b < decoding_batches; ++b)
        if (start_pos[b] < 0 || (cache_mode == 1 && start_pos[b] / page_size >= max_pages)) return PPLHIP_INVALID_VALUE;
    *table_width = window_shift(start_pos, cache_indices, max_pages, decoding_batches, cache_mode, page_size, window, pos_out, table_out, skip_out,
                                max_kv_len_out);
    return 0;
}

int pplhip_op_attention_window(void* stream, const void* qkv, const pplhip_kv_view* kv, const int64_t* seq_starts, const int64_t* start_pos,
                               const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t T, int64_t decoding_batches,
                               int64_t max_seq_len, int64_t max_kv_len, int32_t num_heads, int32_t split_k, void* workspace,
                               uint64_t workspace_bytes, void* out, int32_t window) {
    if (window <= 0)
        return pplhip_op_attention(stream, qkv, kv, seq_starts, start_pos, cache_indices, max_pages, B, T, decoding_batches, max_seq_len, max_kv_len,
                                   num_heads, split_k, workspace, workspace_bytes, out);
    if (!kv) return PPLHIP_INVALID_VALUE;
    const std::string why = window_refusal(kv->quant_bit, kv->quant_group, kv->head_dim);   // before any HIP call
    if (!why.empty()) return fail(nullptr, -1, PPLHIP_UNSUPPORTED, "pplhip_op_attention_window: " + why);
    if (window >= max_kv_len)   // the window never binds: the same launches, so the same bits
        return pplhip_op_attention(stream, qkv, kv, seq_starts, start_pos, cache_indices, max_pages, B, T, decoding_batches, max_seq_len, max_kv_len,
                                   num_heads, split_k, workspace, workspace_bytes, out);
    const int fmt = kv_format(kv->quant_bit, kv->quant_group, kv->head_dim);
    const int H = num_heads, Hkv = kv->kv_heads, D = kv->head_dim;
    if (B < 0 || H <= 0 || Hkv <= 0 || H % Hkv || (kv->mode == 1 && (kv->page_size <= 0 || max_pages <= 0))) return PPLHIP_INVALID_VALUE;
    const int64_t nb = std::min<int64_t>(std::max<int64_t>(decoding_batches, 0), B);
    const int split = split_k < 1 ? 1 : split_k;
    const int64_t mp = kv->mode == 1 ? max_pages : 1;
    const uint64_t part = up256(attn_decode_workspace_bytes(nb, H, D, split));
    // (decode rows alone need the workspace: the band kernel takes none, and a pure-prefill call may pass NULL like pplhip_op_attention)
    if (nb > 0 && (!workspace || part + 256 + WindowBlock(nullptr, nb, mp).bytes > workspace_bytes)) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    const KvAddr a = view_kv_addr(kv);
    hipError_t e = hipSuccess;
    if (nb > 0) {
        // the decode rows' positions and slots / page table come to the host, are shifted, and go back behind the split partials
        std::vector<int64_t> pos((size_t)nb), tab((size_t)(nb * mp)), img((size_t)(WindowBlock(nullptr, nb, mp).bytes + 7) / 8);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return op_rc(e);
        if ((e = hipMemcpy(pos.data(), start_pos, (size_t)nb * 8, hipMemcpyDeviceToHost)) != hipSuccess) return op_rc(e);
        if ((e = hipMemcpy(tab.data(), cache_indices, (size_t)(nb * mp) * 8, hipMemcpyDeviceToHost)) != hipSuccess) return op_rc(e);
        for (int64_t b = 0; b < nb; ++b)
            if (pos[(size_t)b] < 0 || (kv->mode == 1 && pos[(size_t)b] / kv->page_size >= max_pages)) return PPLHIP_INVALID_VALUE;
        std::vector<int64_t> spos((size_t)nb);
        std::vector<int32_t> skip((size_t)nb);
        int64_t max_kv = 0;
        const int64_t width = window_shift(pos.data(), tab.data(), max_pages, nb, kv->mode, kv->page_size, window, spos.data(), nullptr, skip.data(), &max_kv);
        const WindowBlock h(img.data(), nb, width);
        window_shift(pos.data(), tab.data(), max_pages, nb, kv->mode, kv->page_size, window, h.pos, h.table, h.skip, nullptr);
        char* base = (char*)workspace + part;
        base += (256 - ((uintptr_t)base & 255)) & 255;
        const WindowBlock d(base, nb, width);
        // (a pageable source: the copy has left the host buffer when the call returns)
        if ((e = hipMemcpyAsync(base, img.data(), (size_t)h.bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return op_rc(e);
        e = window_decode(s, (const uint16_t*)qkv, a, fmt, seq_starts, d, width, nb, H, Hkv, D, max_kv, split, 256, (float*)workspace, (uint16_t*)out);
    }
    if (e == hipSuccess && B > nb)
        e = launch_attn_prefill_window(s, (const uint16_t*)qkv, a, fmt, seq_starts, start_pos, cache_indices, max_pages, nb, B, H, Hkv, D, max_seq_len,
                                       window, (uint16_t*)out);
    return op_rc(e);
}

// ---- the runtime's use of it ----------------------------------------------------------------------------------------------------------

int pplhip_sliding_window(pplhip_ctx* c, int32_t window) {
    if (!c || window < 0) return PPLHIP_INVALID_VALUE;
    if (window > 0) {
        const std::string why = window_refusal(c->d.cache_quant_bit, c->d.cache_quant_group, c->D);
        if (!why.empty()) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_sliding_window: " + why);
        if (c->alibi) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_sliding_window: this context runs under ALiBi");
        for (const Rank& R : c->ranks)
            if (R.sp_min_rows > 0) return fail(c, -1, PPLHIP_UNSUPPORTED, "pplhip_sliding_window: shared-prefix detection is on in this context");
    }
    c->window = window;
    return 0;
}

bool window_active(const pplhip_ctx* c, const Rank& R) { return c->window > 0 && c->window < R.max_kv_len; }

void window_release(Rank& R) {
    for (Stage& st : R.st_win) st.release();
    if (R.win_dev) (void)hipFree(R.win_dev);
    R.win_dev = nullptr;
    R.win_cap = 0;
}

void window_stage(const pplhip_ctx* c, Rank& R, const pplhip_step* st) {
    const int64_t nd = std::min<int64_t>(std::max<int64_t>(st->decoding_batches, 0), st->batch);
    R.win_start_pos.assign(st->start_pos, st->start_pos + nd);
    if (c->d.cache_mode == 0) R.win_slots.assign(st->cache_indices, st->cache_indices + nd);
}

int64_t window_split_kv_len(const pplhip_ctx* c, const Rank& R) {
    if (!window_active(c, R)) return R.max_kv_len;
    const int64_t ps = c->d.cache_mode == 1 ? std::max(c->d.page_size, 1) : 1;
    return std::min<int64_t>(R.max_kv_len, (int64_t)c->window + ps - 1);
}

int window_plan(pplhip_ctx* c, int rank) {
    Rank& R = c->ranks[rank];
    R.win_nd = 0;
    if (!window_active(c, R)) return 0;
    const int64_t nd = std::min<int64_t>(std::max<int64_t>(R.decoding_batches, 0), R.B);
    if (nd == 0 || (int64_t)R.win_start_pos.size() != nd) return 0;
    const bool paged = c->d.cache_mode == 1;
    if (paged && (!R.pages_host || R.max_pages <= 0)) return 0;
    const int64_t* table = paged ? R.pages_host : R.win_slots.data();
    const int64_t mp = paged ? R.max_pages : 1;
    const uint64_t need = WindowBlock(nullptr, nd, mp).bytes;
    if (need > R.win_cap) {   // (rare: a larger batch or a wider page table; hipFree waits for the launches that read the old block)
        window_release(R);
        HIPCK(c, rank, hipSetDevice(R.device));
        HIPCK(c, rank, hipMalloc((void**)&R.win_dev, need * 2));
        for (Stage& st : R.st_win) HIPCK(c, rank, st.allocate((size_t)need * 2));
        R.win_cap = need * 2;
    }
    Stage& stage = R.st_win[R.st_win_cur];
    R.st_win_cur ^= 1;
    char* img;
    HIPCK(c, rank, stage.begin(&img));
    // (the width first: the image's columns depend on it; positions and skips land in the image's own columns on the second pass)
    std::vector<int64_t> pos((size_t)nd);
    std::vector<int32_t> skip((size_t)nd);
    R.win_width = window_shift(R.win_start_pos.data(), table, mp, nd, c->d.cache_mode, c->d.page_size, c->window, pos.data(), nullptr, skip.data(),
                               &R.win_max_kv);
    const WindowBlock h(img, nd, R.win_width);
    window_shift(R.win_start_pos.data(), table, mp, nd, c->d.cache_mode, c->d.page_size, c->window, h.pos, h.table, h.skip, nullptr);
    HIPCK(c, rank, stage.upload(R.win_dev, (size_t)h.bytes, R.stream));
    R.win_nd = nd;
    return 0;
}

int window_attention_decode(pplhip_ctx* c, int rank, Lane& lane, const KvAddr& kv, const pplhip_chunk& k, int split, int threads) {
    Rank& R = c->ranks[rank];
    const int H = c->H, Hkv = c->Hkv, D = c->D;
    if (R.win_nd < k.b0 + k.nd) return fail(c, rank, PPLHIP_OTHER_ERROR, "sliding window: the step's decode rows were not staged");
    WindowBlock d(R.win_dev, R.win_nd, R.win_width);   // the chunk's rows of the step's block
    d.pos += k.b0; d.table += k.b0 * R.win_width; d.skip += k.b0;
    HIPCK(c, rank, window_decode(lane.stream, R.qkv, kv, c->kv_fmt, R.d_seq + k.b0, d, R.win_width, k.nd, H, Hkv, D, R.win_max_kv, split, threads,
                                 lane.attn_ws, R.att + k.b0 * (int64_t)H * D));
    return 0;
}

int window_attention_prefill(pplhip_ctx* c, int rank, Lane& lane, const KvAddr& kv, const pplhip_chunk& k) {
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, launch_attn_prefill_window(lane.stream, R.qkv, kv, c->kv_fmt, R.d_seq, R.d_sp, R.d_ci, R.max_pages, k.b0 + k.nd, k.b0 + k.bn, c->H,
                                              c->Hkv, c->D, R.max_seq_len, c->window, R.att));
    return 0;
}
