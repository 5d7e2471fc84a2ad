// pplhip_op_*: single kernels and the runtime's pure functions on caller-owned memory, for the tests.  None takes a context; what they
// share with the runtime (plan_step, the row and tile lists, the KV addressing) is declared in rt_internal.h.
#include "rt_internal.h"

static int op_rc(hipError_t e) { return e == hipSuccess ? 0 : (e == hipErrorInvalidValue ? PPLHIP_INVALID_VALUE : PPLHIP_DEVICE_RUNTIME_ERROR); }

int pplhip_op_embedding(void* stream, const int64_t* token_ids, const void* table, int64_t T, int32_t hidden, void* out) {
    return op_rc(launch_embedding((hipStream_t)stream, token_ids, (const uint16_t*)table, T, hidden, (uint16_t*)out));
}

int pplhip_op_rmsnorm(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t T, int32_t hidden,
                      void* out, void* residual_out) {
    return op_rc(launch_rmsnorm((hipStream_t)stream, (const uint16_t*)x, (const uint16_t*)skip, (const uint16_t*)w, eps, T,
                                hidden, nullptr, (uint16_t*)out, (uint16_t*)residual_out));
}

// split-K scratch of the stand-alone operators (the runtime owns its own per rank); one per device, never freed
static float* op_linear_ws(size_t* bytes) {
    static float* ws[16] = {nullptr};
    static const size_t ws_bytes = (size_t)64 << 20;
    int dev = 0;
    *bytes = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    if (!ws[dev] && hipMalloc((void**)&ws[dev], ws_bytes) != hipSuccess) ws[dev] = nullptr;
    if (ws[dev]) *bytes = ws_bytes;
    return ws[dev];
}

int pplhip_op_linear(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit, int32_t group, int64_t M,
                     int32_t N, int32_t K, void* y, int32_t out_fp32) {
    size_t ws_bytes = 0;
    float* ws = op_linear_ws(&ws_bytes);
    return op_rc(launch_linear((hipStream_t)stream, (const uint16_t*)x, w, (const uint16_t*)scale, wq_bit, group, M, N, K, y, N,
                               out_fp32 != 0, ws, ws_bytes));
}

// (the same scratch: without it 4 <= M <= 256 ran unsplit -- N / 128 blocks instead of a full chip)
int pplhip_op_linear_swiglu(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit, int32_t group, int64_t M,
                            int32_t N, int32_t K, void* y) {
    size_t ws_bytes = 0;
    float* ws = op_linear_ws(&ws_bytes);
    return op_rc(launch_linear((hipStream_t)stream, (const uint16_t*)x, w, (const uint16_t*)scale, wq_bit, group, M, N, K, y, N / 2,
                               false, ws, ws_bytes, true));
}

// launch_linear with the caller's row stride, workspace and pointers, and the route it takes (kernels.h LinearRoute); dry_run: the route and
// status only, no HIP call at all (works without a device)
int pplhip_op_linear_ex(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit, int32_t group, int64_t M, int32_t N,
                        int32_t K, void* y, int64_t ldy, int32_t epi, void* ws, uint64_t ws_bytes, int32_t dry_run, char* route, int32_t route_len) {
    LinearRoute r;
    r.buf = route_len > 0 ? route : nullptr;
    r.cap = route_len;
    r.dry = dry_run != 0;
    if (r.buf) r.buf[0] = 0;
    if (epi < 0 || epi > 2) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_linear((hipStream_t)stream, (const uint16_t*)x, w, (const uint16_t*)scale, wq_bit, group, M, N, K, y, ldy, epi == 1,
                               (float*)ws, (size_t)ws_bytes, epi == 2, nullptr, &r));
}

int pplhip_op_rmsnorm_quant(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t T, int32_t hidden,
                            void* residual_out, void* q, float* sx) {
    return op_rc(launch_rmsnorm((hipStream_t)stream, (const uint16_t*)x, (const uint16_t*)skip, (const uint16_t*)w, eps, T, hidden, nullptr,
                                nullptr, (uint16_t*)residual_out, (int8_t*)q, sx));
}

int pplhip_op_quant_act(void* stream, const void* x, int64_t M, int32_t K, void* q, float* sx) {
    return op_rc(launch_quant_act((hipStream_t)stream, (const uint16_t*)x, M, K, K, (int8_t*)q, K, sx));
}

int pplhip_op_quant_weight(void* stream, const void* w, int32_t N, int32_t K, void* q, void* scale) {
    return op_rc(launch_quant_weight((hipStream_t)stream, (const uint16_t*)w, N, K, (int8_t*)q, K, (uint16_t*)scale));
}

int pplhip_op_linear_i8(void* stream, const void* xq, const float* sx, const void* w, const void* scale, int64_t M, int32_t N, int32_t K,
                        void* y, int32_t out_fp32, int32_t swiglu) {
    return op_rc(launch_linear_i8((hipStream_t)stream, (const int8_t*)xq, sx, (const int8_t*)w, (const uint16_t*)scale, M, N, K, y,
                                  swiglu ? N / 2 : N, out_fp32 != 0, swiglu != 0));
}

int pplhip_op_rmsnorm_quant_f8(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t T, int32_t hidden,
                               void* residual_out, void* q, float* sx) {
    if (!q || !sx) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_rmsnorm((hipStream_t)stream, (const uint16_t*)x, (const uint16_t*)skip, (const uint16_t*)w, eps, T, hidden, nullptr,
                                nullptr, (uint16_t*)residual_out, (int8_t*)q, sx, nullptr, true));
}

int pplhip_op_quant_act_f8(void* stream, const void* x, int64_t M, int32_t K, void* q, float* sx) {
    return op_rc(launch_quant_act_f8((hipStream_t)stream, (const uint16_t*)x, M, K, K, (uint8_t*)q, K, sx));
}

int pplhip_op_quant_weight_f8(void* stream, const void* w, int32_t N, int32_t K, void* q, void* scale) {
    return op_rc(launch_quant_weight_f8((hipStream_t)stream, (const uint16_t*)w, N, K, (uint8_t*)q, K, (uint16_t*)scale));
}

int pplhip_op_linear_f8(void* stream, const void* xq, const float* sx, const void* w, const void* scale, int64_t M, int32_t N, int32_t K,
                        void* y, int32_t out_fp32, int32_t swiglu) {
    return op_rc(launch_linear_f8((hipStream_t)stream, (const uint8_t*)xq, sx, (const uint8_t*)w, (const uint16_t*)scale, M, N, K, y,
                                  swiglu ? N / 2 : N, out_fp32 != 0, swiglu != 0));
}

// launch_linear_i8 / _f8 with the caller's row stride and the route it takes (kernels.h LinearRoute); dry_run: the route and status only, no
// HIP call at all (works without a device)
int pplhip_op_linear_q8_ex(void* stream, const void* xq, const float* sx, const void* w, const void* scale, int32_t act_fmt, int64_t M,
                           int32_t N, int32_t K, void* y, int64_t ldy, int32_t epi, int32_t dry_run, char* route, int32_t route_len) {
    LinearRoute r;
    r.buf = route_len > 0 ? route : nullptr;
    r.cap = route_len;
    r.dry = dry_run != 0;
    if (r.buf) r.buf[0] = 0;
    if (epi < 0 || epi > 2) return PPLHIP_INVALID_VALUE;
    if (act_fmt == PPLHIP_ACT_QUANT_I8)
        return op_rc(launch_linear_i8((hipStream_t)stream, (const int8_t*)xq, sx, (const int8_t*)w, (const uint16_t*)scale, M, N, K, y, ldy,
                                      epi == 1, epi == 2, &r));
    if (act_fmt == PPLHIP_ACT_QUANT_FP8)
        return op_rc(launch_linear_f8((hipStream_t)stream, (const uint8_t*)xq, sx, (const uint8_t*)w, (const uint16_t*)scale, M, N, K, y, ldy,
                                      epi == 1, epi == 2, &r));
    return PPLHIP_INVALID_VALUE;
}

int pplhip_op_step_plan(const pplhip_plan_settings* settings, const pplhip_step_shape* shape, pplhip_step_plan* out) {
    if (!settings || !shape || !out || shape->batch < 0 || shape->num_tokens < 0) return PPLHIP_INVALID_VALUE;
    *out = plan_step(*settings, *shape);
    return 0;
}

int pplhip_op_lora(void* stream, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t T, int32_t N, int32_t K, const int32_t* row_slots,
                   int32_t n_slots, const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, void* ws,
                   uint64_t ws_bytes) {
    // everything the kernels trust is checked here, before any HIP call
    if (T < 0 || T > INT32_MAX || N <= 0 || K <= 0 || K % 32 || N % 16 || ldx < K || ldx % 8 || ldy < N) return PPLHIP_INVALID_VALUE;
    if (n_slots < 0 || n_slots > LORA_MAX_SLOTS || (T > 0 && !row_slots) || (n_slots > 0 && (!A || !B || !ranks || !scales))) return PPLHIP_INVALID_VALUE;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 1)) return PPLHIP_INVALID_VALUE;
    LoraSlot tab[LORA_MAX_SLOTS];
    for (int s = 0; s < LORA_MAX_SLOTS; ++s) tab[s] = LoraSlot{nullptr, nullptr, 0, 0.f};
    for (int s = 0; s < n_slots; ++s) {
        if (!A[s] && !B[s]) continue;
        if (!A[s] || !B[s] || ranks[s] < 1 || ranks[s] > LORA_MAX_RANK || ((uintptr_t)A[s] & 15) || ((uintptr_t)B[s] & 15)) return PPLHIP_INVALID_VALUE;
        tab[s] = LoraSlot{(const uint16_t*)A[s], (const uint16_t*)B[s], (ranks[s] + 15) / 16 * 16, scales[s]};
    }
    bool any = false;
    for (int64_t m = 0; m < T; ++m) {
        const int s = row_slots[m];
        if (s == -1) continue;
        if (s < 0 || s >= n_slots || !tab[s].a) return PPLHIP_INVALID_VALUE;   // out of range, or not loaded
        any = true;
    }
    if (!any) return 0;
    if (!x || !y || !ws) return PPLHIP_INVALID_VALUE;
    std::vector<LoraTile> tiles;
    lora_build_tiles(row_slots, T, tiles);
    // workspace: slot table | tile list | t, each on a 256-byte boundary
    const uint64_t tab_bytes = sizeof(tab), tile_bytes = (tiles.size() * sizeof(LoraTile) + 255) / 256 * 256;
    const uint64_t pre = (256 - ((uintptr_t)ws & 255)) & 255;
    const uint64_t need = pre + tab_bytes + tile_bytes + (uint64_t)tiles.size() * 16 * LORA_MAX_RANK * 2;
    if (ws_bytes < need) return PPLHIP_INVALID_VALUE;
    char* base = (char*)ws + pre;
    hipStream_t s = (hipStream_t)stream;
    // (pageable sources: each copy has left the host buffer when the call returns)
    hipError_t e = hipMemcpyAsync(base, tab, tab_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + tab_bytes, tiles.data(), tiles.size() * sizeof(LoraTile), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = launch_lora(s, (const LoraTile*)(base + tab_bytes), (int)tiles.size(), (const LoraSlot*)base, (const uint16_t*)x, ldx, (uint16_t*)y, ldy, N, K,
                        (uint16_t*)(base + tab_bytes + tile_bytes));
    return op_rc(e);
}

int pplhip_op_silu_mul(void* stream, const void* gate_up, int64_t T, int32_t inter, void* out) {
    return op_rc(launch_silu_mul((hipStream_t)stream, (const uint16_t*)gate_up, T, inter, (uint16_t*)out));
}

// K12 / K13 alone, on the caller's buffers (the tests preload and read back the count map and pick vocab, stride and alignment)
int pplhip_op_penalty(void* stream, float* logits, const float* temperatures, const float* rep, const float* presence,
                      const float* frequency, const int64_t* batch_slots, const int64_t* token_inputs, const int64_t* seq_starts,
                      const int64_t* start_pos, int32_t batch, int32_t vocab, int32_t stride, int32_t decoding_batches, uint16_t* count_map) {
    if (batch < 0 || vocab <= 0 || stride < vocab) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_penalty((hipStream_t)stream, logits, temperatures, rep, presence, frequency, batch_slots, token_inputs, seq_starts,
                                start_pos, batch, vocab, stride, decoding_batches, count_map));
}

int pplhip_op_sample(void* stream, const float* logits, const float* temperatures, const float* top_p, const float* rnd, int32_t batch,
                     int32_t vocab, int32_t stride, int32_t top_k, float default_top_p, int32_t* out_tok, float* out_logprob) {
    if (batch < 0 || vocab <= 0 || stride < vocab) return PPLHIP_INVALID_VALUE;
    if (top_k == 1)
        return op_rc(launch_sample_greedy((hipStream_t)stream, logits, temperatures, batch, vocab, stride, out_tok, out_logprob));
    if (!rnd && batch > 0) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_sample_topk_topp((hipStream_t)stream, logits, temperatures, top_p, rnd, batch, vocab, stride, top_k, default_top_p,
                                         nullptr, out_tok, out_logprob));
}

// the per-request sampler alone.  The row list is made here: top_k is read back, compacted on the host and sent up again into stream-ordered
// scratch (two synchronisations of `stream` in front of the launches) -- test support, the product entry point has the arrays on the host already
int pplhip_op_sample_rows(void* stream, const float* logits, const float* temperatures, const int32_t* top_k, const float* top_p,
                          const uint64_t* seeds, const uint64_t* draws, const float* rnd, int32_t batch, int32_t vocab, int32_t stride,
                          int32_t* out_tok, float* out_logprob) {
    return pplhip_op_sample_rows2(stream, logits, temperatures, top_k, top_p, nullptr, nullptr, seeds, draws, rnd, batch, vocab, stride, out_tok,
                                  out_logprob);
}

// ... with the two truncation arrays (either may be NULL), read back like top_k for the third kind of the row list
int pplhip_op_sample_rows2(void* stream, const float* logits, const float* temperatures, const int32_t* top_k, const float* top_p,
                           const float* min_p, const float* typical_p, const uint64_t* seeds, const uint64_t* draws, const float* rnd,
                           int32_t batch, int32_t vocab, int32_t stride, int32_t* out_tok, float* out_logprob) {
    if (batch < 0 || vocab <= 0 || stride < vocab) return PPLHIP_INVALID_VALUE;
    if (batch == 0) return 0;
    if (!logits || !top_k || !top_p || !out_tok || !out_logprob || (!rnd && (!seeds || !draws))) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> k(batch), rows(batch);
    std::vector<float> mp(min_p ? batch : 0), ty(typical_p ? batch : 0);
    hipError_t e = hipMemcpyAsync(k.data(), top_k, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && min_p) e = hipMemcpyAsync(mp.data(), min_p, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && typical_p) e = hipMemcpyAsync(ty.data(), typical_p, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    int nt = 0;
    const int ng = sample_row_list(k.data(), min_p ? mp.data() : nullptr, typical_p ? ty.data() : nullptr, batch, rows.data(), &nt);
    int32_t* d_rows = nullptr;
    if ((e = hipMallocAsync((void**)&d_rows, (size_t)batch * 4, s)) != hipSuccess) return op_rc(e);
    e = hipMemcpyAsync(d_rows, rows.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // `rows` is pageable and dies with this call; the stream was idle anyway
    if (e == hipSuccess)
        e = launch_sample_rows(s, logits, temperatures, top_k, top_p, seeds, draws, rnd, d_rows, ng, batch - ng - nt, vocab, stride, out_tok, out_logprob,
                               min_p, typical_p, nt);
    const hipError_t e2 = hipFreeAsync(d_rows, s);
    return op_rc(e != hipSuccess ? e : e2);
}

// top_logprobs_kernel alone.  The row list is made here from a read-back of num_logprobs, as pplhip_op_sample_rows makes its own
int pplhip_op_top_logprobs(void* stream, const float* logits, const float* temperatures, const int32_t* num_logprobs, int32_t batch,
                           int32_t vocab, int32_t stride, int32_t* out_tok, float* out_logprob) {
    if (batch < 0 || vocab <= 0 || stride < vocab) return PPLHIP_INVALID_VALUE;
    if (batch == 0) return 0;
    if (!logits || !num_logprobs || !out_tok || !out_logprob) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> n(batch), rows(batch);
    hipError_t e = hipMemcpyAsync(n.data(), num_logprobs, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    const int asked = top_logprobs_row_list(n.data(), batch, rows.data());
    if (asked < 0) return PPLHIP_INVALID_VALUE;
    if (asked == 0) return 0;
    int32_t* d_rows = nullptr;
    if ((e = hipMallocAsync((void**)&d_rows, (size_t)asked * 4, s)) != hipSuccess) return op_rc(e);
    e = hipMemcpyAsync(d_rows, rows.data(), (size_t)asked * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // `rows` is pageable and dies with this call
    if (e == hipSuccess) e = launch_top_logprobs(s, logits, temperatures, num_logprobs, d_rows, asked, vocab, stride, out_tok, out_logprob);
    const hipError_t e2 = hipFreeAsync(d_rows, s);
    return op_rc(e != hipSuccess ? e : e2);
}

// logit_edit_kernel alone on caller-owned memory; without `rows` the list is made here from a read-back of flags
int pplhip_op_logit_edit(void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const uint32_t* flags, const int32_t* slots,
                         const int32_t* head, const int32_t* bias_tokens, const float* bias_values, const int32_t* stop_tokens,
                         const uint32_t* mask, const int32_t* rows, int32_t n_rows) {
    if (batch < 0 || vocab <= 0 || stride < vocab || n_rows < 0 || n_rows > batch) return PPLHIP_INVALID_VALUE;
    if (batch == 0) return 0;
    if (!logits || !flags || !slots || !head || !bias_tokens || !bias_values || !stop_tokens || !mask) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    const LogitRuleTable tb{head, bias_tokens, bias_values, stop_tokens, mask, 4, LOGIT_BIAS_MAX, LOGIT_STOP_MAX, ((int64_t)vocab + 31) / 32};
    if (rows) return op_rc(launch_logit_edit(s, logits, stride, vocab, rows, n_rows, slots, flags, tb));
    std::vector<uint32_t> f(batch);
    std::vector<int32_t> list;
    hipError_t e = hipMemcpyAsync(f.data(), flags, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    for (int i = 0; i < batch; ++i)
        if (f[i]) list.push_back(i);
    if (list.empty()) return 0;
    int32_t* d_rows = nullptr;
    if ((e = hipMallocAsync((void**)&d_rows, list.size() * 4, s)) != hipSuccess) return op_rc(e);
    e = hipMemcpyAsync(d_rows, list.data(), list.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // `list` is pageable and dies with this call
    if (e == hipSuccess) e = launch_logit_edit(s, logits, stride, vocab, d_rows, (int)list.size(), slots, flags, tb);
    const hipError_t e2 = hipFreeAsync(d_rows, s);
    return op_rc(e != hipSuccess ? e : e2);
}

// prompt_logprobs_kernel alone.  rows and n_top are read back and checked here: the kernel indexes `targets` with the former
int pplhip_op_prompt_logprobs(void* stream, const float* logits, int32_t stride, int32_t vocab, const int32_t* rows, int32_t n_rows,
                              const int64_t* targets, int64_t n_targets, const int32_t* n_top, float* out_logprob, int32_t* out_rank,
                              int32_t* out_top_tok, float* out_top_logprob) {
    if (n_rows < 0 || vocab <= 0 || stride < vocab) return PPLHIP_INVALID_VALUE;
    if (n_rows == 0) return 0;
    if (!logits || !rows || !targets || !n_top || !out_logprob || !out_rank) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> hr(n_rows), hn(n_rows);
    hipError_t e = hipMemcpyAsync(hr.data(), rows, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hn.data(), n_top, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    bool top = false;
    for (int32_t j = 0; j < n_rows; ++j) {
        if (hn[j] < 0 || hn[j] > PPLHIP_TOP_LOGPROBS_MAX || hr[j] < -1 || (int64_t)hr[j] + 1 >= n_targets) return PPLHIP_INVALID_VALUE;
        top = top || hn[j] > 0;
    }
    if (top && (!out_top_tok || !out_top_logprob)) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_prompt_logprobs(s, logits, stride, vocab, rows, n_rows, targets, n_top, out_logprob, out_rank, out_top_tok, out_top_logprob));
}

// the two k_guide.hip kernels alone on caller-owned memory
int pplhip_op_guide_build(void* stream, const uint8_t* trans, const uint8_t* accept, int32_t n_states, const uint8_t* tok_bytes,
                          const int64_t* tok_off, int32_t n_tok, const int32_t* end_tokens, int32_t n_end, int32_t vocab, uint32_t* mask,
                          int64_t mask_stride, uint32_t* any) {
    if (n_states < 1 || n_states > GUIDE_MAX_STATES || vocab <= 0 || n_tok < 0 || n_tok > vocab || n_end < 0 || n_end > LOGIT_STOP_MAX ||
        mask_stride < ((int64_t)vocab + 31) / 32)
        return PPLHIP_INVALID_VALUE;
    if (!trans || !accept || !tok_bytes || !tok_off || !mask || !any || (n_end > 0 && !end_tokens)) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_guide_build((hipStream_t)stream, trans, accept, n_states, tok_bytes, tok_off, n_tok, end_tokens, n_end, vocab, mask,
                                    mask_stride, any));
}

int pplhip_op_guide_build16(void* stream, const uint16_t* trans, const uint8_t* accept, int32_t n_states, const uint8_t* tok_bytes,
                            const int64_t* tok_off, int32_t n_tok, const int32_t* end_tokens, int32_t n_end, int32_t vocab, uint32_t* mask,
                            int64_t mask_stride, uint32_t* any) {
    if (n_states < 1 || n_states > GUIDE16_MAX_STATES || vocab <= 0 || n_tok < 0 || n_tok > vocab || n_end < 0 || n_end > LOGIT_STOP_MAX ||
        mask_stride < ((int64_t)vocab + 31) / 32)
        return PPLHIP_INVALID_VALUE;
    if (!trans || !accept || !tok_bytes || !tok_off || !mask || !any || (n_end > 0 && !end_tokens)) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_guide_build16((hipStream_t)stream, trans, accept, n_states, tok_bytes, tok_off, n_tok, end_tokens, n_end, vocab, mask,
                                      mask_stride, any));
}

static int op_guide_mask(int max_states, void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const int32_t* guide_slots,
                         const int32_t* states, const uint32_t* masks, int32_t n_slots, int32_t n_states, int64_t mask_stride,
                         const int32_t* rows, int32_t n_rows) {
    if (batch < 0 || vocab <= 0 || stride < vocab || n_rows < 0 || n_rows > batch || n_slots < 1 || n_slots > GUIDE_MAX_SLOTS ||
        n_states < 1 || n_states > max_states || mask_stride < ((int64_t)vocab + 31) / 32)
        return PPLHIP_INVALID_VALUE;
    if (batch == 0) return 0;
    if (!logits || !guide_slots || !states || !masks) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    GuideTable tb;
    for (int i = 0; i < GUIDE_MAX_SLOTS; ++i) tb.mask[i] = i < n_slots ? masks + (int64_t)i * n_states * mask_stride : nullptr;
    tb.mask_stride = mask_stride;
    if (rows) return op_rc(launch_guide_mask(s, logits, stride, vocab, rows, n_rows, guide_slots, states, tb));
    std::vector<int32_t> gs(batch), st(batch), list;
    hipError_t e = hipMemcpyAsync(gs.data(), guide_slots, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(st.data(), states, (size_t)batch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return op_rc(e);
    for (int i = 0; i < batch; ++i) {
        if (gs[i] < 0) continue;
        if (gs[i] >= n_slots || st[i] < 0 || st[i] >= n_states) return PPLHIP_INVALID_VALUE;   // would read outside `masks`
        list.push_back(i);
    }
    if (list.empty()) return 0;
    int32_t* d_rows = nullptr;
    if ((e = hipMallocAsync((void**)&d_rows, list.size() * 4, s)) != hipSuccess) return op_rc(e);
    e = hipMemcpyAsync(d_rows, list.data(), list.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // `list` is pageable and dies with this call
    if (e == hipSuccess) e = launch_guide_mask(s, logits, stride, vocab, d_rows, (int)list.size(), guide_slots, states, tb);
    const hipError_t e2 = hipFreeAsync(d_rows, s);
    return op_rc(e != hipSuccess ? e : e2);
}

int pplhip_op_guide_mask(void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const int32_t* guide_slots,
                         const int32_t* states, const uint32_t* masks, int32_t n_slots, int32_t n_states, int64_t mask_stride,
                         const int32_t* rows, int32_t n_rows) {
    return op_guide_mask(GUIDE_MAX_STATES, stream, logits, stride, vocab, batch, guide_slots, states, masks, n_slots, n_states, mask_stride, rows,
                         n_rows);
}

int pplhip_op_guide_mask16(void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const int32_t* guide_slots,
                           const int32_t* states, const uint32_t* masks, int32_t n_slots, int32_t n_states, int64_t mask_stride,
                           const int32_t* rows, int32_t n_rows) {
    return op_guide_mask(GUIDE16_MAX_STATES, stream, logits, stride, vocab, batch, guide_slots, states, masks, n_slots, n_states, mask_stride,
                         rows, n_rows);
}

int pplhip_op_sample_uniform(void* stream, const uint64_t* seeds, const uint64_t* draws, int32_t batch, float* out_u) {
    if (batch < 0 || (batch > 0 && (!seeds || !draws || !out_u))) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_sample_uniform((hipStream_t)stream, seeds, draws, batch, out_u));
}

static KvAddr view_addr(const pplhip_kv_view* v) {
    pplhip_model_desc d;
    memset(&d, 0, sizeof(d));
    d.num_layers = v->num_layers;
    d.cache_quant_bit = v->quant_bit; d.cache_quant_group = v->quant_group;
    d.cache_layout = v->layout; d.cache_mode = v->mode; d.page_size = v->page_size;
    return make_kv_addr(d, v->kv_heads, v->head_dim, (uint64_t)v->max_tokens, v->cache, (uint16_t*)v->scale, v->layer);
}

int pplhip_op_rope_kv_write(void* stream, void* qkv, const float* cos_sin, const pplhip_kv_view* kv, const int64_t* seq_starts,
                            const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t T,
                            int32_t num_heads) {
    const int fmt = kv ? kv_format(kv->quant_bit, kv->quant_group, kv->head_dim) : -1;
    if (fmt < 0) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_rope_kv_write((hipStream_t)stream, (uint16_t*)qkv, cos_sin, view_addr(kv), fmt,
                                      seq_starts, start_pos, cache_indices, max_pages, B, 0, T, num_heads, kv->kv_heads, kv->head_dim));
}

// ---- the row kernels with everything their launchers take (for the tests: not part of the product boundary) ----
// slab description -> SplitSlabs of a [slab_M, N] launch; false: not a description a producer can leave
static bool op_slabs(const float* ws, int32_t splits, const void* scale, int64_t M, int N, SplitSlabs* sl) {
    *sl = SplitSlabs{};
    if (splits == 0) return true;
    if (splits < 0 || splits > 8 || !ws || M <= 0 || N <= 0 || N % 8 || ((uintptr_t)ws & 15) || ((uintptr_t)scale & 15)) return false;
    *sl = SplitSlabs{ws, splits, (const uint16_t*)scale, N, M};
    return true;
}

int pplhip_op_rmsnorm_form(int64_t rows, int32_t hidden, int32_t quant, int32_t wide_max_rows, char* buf, int32_t len) {
    if (buf && len > 0) buf[0] = 0;
    if (rows < 0 || quant < 0 || quant > 2) return PPLHIP_INVALID_VALUE;
    RmsnormForm f;
    const hipError_t e = rmsnorm_form(rows, hidden, wide_max_rows, &f);
    if (e == hipSuccess && f.nt && buf && len > 0)
        snprintf(buf, (size_t)len, "rmsnorm_kernel<%d,%d%s>", f.maxc, f.nt, quant == 2 ? ",f8" : (quant == 1 ? ",i8" : ""));
    return op_rc(e);
}

int pplhip_op_rmsnorm_ex(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t rows, int32_t hidden,
                         const int64_t* gather_seq_starts, void* out, void* residual_out, void* q, float* sx, int32_t q_fp8,
                         const float* slab_ws, int32_t slab_splits, const void* slab_scale, int64_t slab_M) {
    SplitSlabs sl;
    if (rows < 0 || !op_slabs(slab_ws, slab_splits, slab_scale, slab_M, hidden, &sl)) return PPLHIP_INVALID_VALUE;
    if (rows > 0 && (!x || !w || (q ? !sx : !out))) return PPLHIP_INVALID_VALUE;
    if (sl.splits && !gather_seq_starts && rows > slab_M) return PPLHIP_INVALID_VALUE;   // (gathered rows: the caller's seq_starts stay below slab_M)
    return op_rc(launch_rmsnorm((hipStream_t)stream, (const uint16_t*)x, (const uint16_t*)skip, (const uint16_t*)w, eps, rows, hidden,
                                gather_seq_starts, (uint16_t*)out, (uint16_t*)residual_out, (int8_t*)q, sx, &sl, q_fp8 != 0));
}

int pplhip_op_gather_last_rows(void* stream, const void* x, const int64_t* seq_starts, int64_t B, int32_t hidden, void* out) {
    if (B < 0 || (B > 0 && (!x || !seq_starts || !out))) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_gather_last_rows((hipStream_t)stream, (const uint16_t*)x, seq_starts, B, hidden, (uint16_t*)out));
}

int pplhip_op_rope_kv_write_ex(void* stream, void* qkv, const float* cos_sin, const pplhip_kv_view* kv, const int64_t* seq_starts,
                               const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t t0, int64_t T,
                               int32_t num_heads, const float* slab_ws, int32_t slab_splits, const void* slab_scale, int64_t slab_M) {
    const int fmt = kv ? kv_format(kv->quant_bit, kv->quant_group, kv->head_dim) : -1;
    if (fmt < 0 || t0 < 0 || T < 0 || B < 0) return PPLHIP_INVALID_VALUE;
    SplitSlabs sl;
    if (!op_slabs(slab_ws, slab_splits, slab_scale, slab_M, (num_heads + 2 * kv->kv_heads) * kv->head_dim, &sl)) return PPLHIP_INVALID_VALUE;
    return op_rc(launch_rope_kv_write((hipStream_t)stream, (uint16_t*)qkv, cos_sin, view_addr(kv), fmt, seq_starts, start_pos, cache_indices,
                                      max_pages, B, t0, T, num_heads, kv->kv_heads, kv->head_dim, &sl));
}

// launch_linear (fp16 epilogue) with a non-null `defer`, as layer_linear calls it for wqkv / wo / w2: a split-K route leaves its slabs in ws
int pplhip_op_linear_defer(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit, int32_t group, int64_t M, int32_t N,
                           int32_t K, void* y, int64_t ldy, void* ws, uint64_t ws_bytes, int32_t dry_run, int32_t* splits,
                           const void** slab_scale, char* route, int32_t route_len) {
    LinearRoute r;
    r.buf = route_len > 0 ? route : nullptr;
    r.cap = route_len;
    r.dry = dry_run != 0;
    if (r.buf) r.buf[0] = 0;
    SplitSlabs sl;
    const hipError_t e = launch_linear((hipStream_t)stream, (const uint16_t*)x, w, (const uint16_t*)scale, wq_bit, group, M, N, K, y, ldy, false,
                                       (float*)ws, (size_t)ws_bytes, false, &sl, &r);
    if (splits) *splits = sl.splits;
    if (slab_scale) *slab_scale = sl.scale;
    return op_rc(e);
}

int pplhip_op_attention(void* stream, const void* qkv, const pplhip_kv_view* kv, const int64_t* seq_starts,
                        const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t T,
                        int64_t decoding_batches, int64_t max_seq_len, int64_t max_kv_len, int32_t num_heads, int32_t split_k,
                        void* workspace, uint64_t workspace_bytes, void* out) {
    (void)T;
    const int fmt = kv ? kv_format(kv->quant_bit, kv->quant_group, kv->head_dim) : -1;
    if (fmt < 0) return PPLHIP_INVALID_VALUE;
    const int64_t nb = std::min<int64_t>(std::max<int64_t>(decoding_batches, 0), B);
    int split = split_k < 1 ? 1 : split_k;
    if (split > 1 && attn_decode_workspace_bytes(nb, num_heads, kv->head_dim, split) > workspace_bytes) return PPLHIP_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    const KvAddr a = view_addr(kv);
    hipError_t e = hipSuccess;
    if (nb > 0)
        e = launch_attn_decode(s, (const uint16_t*)qkv, a, fmt, seq_starts, start_pos, cache_indices, max_pages, nb,
                               num_heads, kv->kv_heads, kv->head_dim, max_kv_len, split, 256, (float*)workspace, (uint16_t*)out);
    if (e == hipSuccess && B > nb)
        e = launch_attn_prefill(s, (const uint16_t*)qkv, a, fmt, seq_starts, start_pos, cache_indices, max_pages, nb, B,
                                num_heads, kv->kv_heads, kv->head_dim, max_seq_len, (uint16_t*)out, max_kv_len, (float*)workspace,
                                (size_t)workspace_bytes, nb, T - nb);
    return op_rc(e);
}

