// What happens to a step's logits on local rank 0's stream: the samplers, the penalty, top-N logprobs, logit rules and guided decoding;
// and prompt logprobs, which pplhip_run itself scores (run_prompt_logprobs, called by pplhip.cc run_launches).
#include "rt_internal.h"

// What the row entry points check first: batch in [0, max_running_batch] and a row stride that covers the vocabulary; `who` != NULL: the
// vocabulary must also be the model's (the message names the entry point)
static int check_rows(pplhip_ctx* c, int batch, int vocab_size, int batch_stride, const char* who) {
    if (batch < 0 || batch > c->ranks[0].cap_B) return fail(c, 0, PPLHIP_INVALID_VALUE, "batch exceeds max_running_batch");
    if (who && vocab_size != c->d.vocab_size) return fail(c, 0, PPLHIP_INVALID_VALUE, std::string(who) + ": vocab_size is not the model's");
    if (vocab_size <= 0 || batch_stride < vocab_size) return fail(c, 0, PPLHIP_INVALID_VALUE, "row stride below vocab_size");
    return 0;
}

/* ------------------------------------------------------------------------------------------------ sampler */

int pplhip_sample(pplhip_ctx* c, const float* logits_device, const pplhip_sample_args* a, int32_t* output_host,
                  float* logprob_host) {
    if (!c || !a || !logits_device || !output_host || !logprob_host) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int B = a->batch;
    if (B < 0 || B > R.cap_B) return fail(c, 0, PPLHIP_INVALID_VALUE, "batch exceeds max_running_batch");
    HIPCK(c, 0, hipSetDevice(R.device));
    hipStream_t s = R.stream;
    // src/backends/cuda/post_processor.cc:126,154-177: temperatures are skipped when the penalty kernel already
    // applied them; device copies are refreshed only when the batch changed and (quirk Q3 of SURVEY.md, kept)
    // passed to the kernel only on those steps.
    const float* temps_host = a->enable_penalty ? nullptr : a->temperatures;
    const float* temp_opt = nullptr;
    const float* topp_opt = nullptr;
    if (a->req_list_changed) {
        if (temps_host) { HIPCK(c, 0, hipMemcpyAsync(R.d_temp, temps_host, B * 4, hipMemcpyHostToDevice, s)); temp_opt = R.d_temp; }
        if (a->top_p) { HIPCK(c, 0, hipMemcpyAsync(R.d_topp, a->top_p, B * 4, hipMemcpyHostToDevice, s)); topp_opt = R.d_topp; }
    }
    static const bool trace = getenv("PPLHIP_SAMPLE_TRACE") != nullptr;  // diagnosis: what every sampling call was handed
    if (trace) {
        fprintf(stderr, "[sample] B %d top_k0 %d top_p0 %g changed %d penalty %d temps", B, a->default_top_k, a->default_top_p, a->req_list_changed, a->enable_penalty);
        for (int i = 0; i < B && a->temperatures; ++i) fprintf(stderr, " %g", a->temperatures[i]);
        fprintf(stderr, " top_p");
        for (int i = 0; i < B && a->top_p; ++i) fprintf(stderr, " %g", a->top_p[i]);
        fprintf(stderr, " top_k");
        for (int i = 0; i < B && a->top_k; ++i) fprintf(stderr, " %d", a->top_k[i]);
        fprintf(stderr, "\n");
    }
    // post_processor.cc:179-183: unseeded rand() sequence (one default value, then one per row)
    const float default_rand = (float)rand() / (float)RAND_MAX;
    (void)default_rand;
    for (int i = 0; i < B; ++i) R.h_rand[i] = (float)rand() / (float)RAND_MAX;
    if (a->default_top_k == 1) {
        HIPCK(c, 0, launch_sample_greedy(s, logits_device, temp_opt, B, a->vocab_size, a->batch_stride, R.d_tokout, R.d_lp));
    } else {
        // top_k <= 0: top-p over the whole vocabulary; top_k > 1024 is clamped (k_sample.hip).  default_top_k is the FIRST
        // row's client-supplied value: it must never turn into a batch-wide Execute failure.
        HIPCK(c, 0, hipMemcpyAsync(R.d_rand, R.h_rand, B * 4, hipMemcpyHostToDevice, s));
        HIPCK(c, 0, launch_sample_topk_topp(s, logits_device, temp_opt, topp_opt, R.d_rand, B, a->vocab_size, a->batch_stride,
                                            a->default_top_k, a->default_top_p, nullptr, R.d_tokout, R.d_lp));
    }
    HIPCK(c, 0, hipMemcpyAsync(output_host, R.d_tokout, B * 4, hipMemcpyDeviceToHost, s));
    HIPCK(c, 0, hipMemcpyAsync(logprob_host, R.d_lp, B * 4, hipMemcpyDeviceToHost, s));
    HIPCK(c, 0, hipStreamSynchronize(s));  // the step's only host<->device synchronisation (post_processor.cc:212)
    if (trace) {
        std::vector<float> row(a->vocab_size);
        for (int i = 0; i < B; ++i) {
            (void)hipMemcpy(row.data(), logits_device + (size_t)i * a->batch_stride, (size_t)a->vocab_size * 4, hipMemcpyDeviceToHost);
            double sum = 0;
            int am = 0;
            for (int v = 0; v < a->vocab_size; ++v) { sum += row[v]; if (row[v] > row[am]) am = v; }
            fprintf(stderr, "[sample]   row %d -> token %d logprob %.6f | logits sum %.6f argmax %d (%.6f) rand %.8f\n", i, output_host[i], logprob_host[i], sum, am,
                    row[am], R.h_rand[i]);
        }
    }
    return p2p_check(c, 0);
}

// greedy rows (top_k == 1) first, then the sampling rows, then the truncating rows (min_p or typical_p on: kernels.h row_min_p /
// row_typical_p; either array may be NULL), each kind in batch order; returns the number of greedy rows, *n_trunc the truncating ones
int sample_row_list(const int32_t* top_k, const float* min_p, const float* typical_p, int B, int32_t* rows, int* n_trunc) {
    const auto trunc = [&](int i) {
        return (min_p && row_min_p(min_p[i]) > 0.f) || (typical_p && row_typical_p(typical_p[i]) > 0.f);
    };
    int ng = 0;
    for (int i = 0; i < B; ++i)
        if (top_k[i] == 1) rows[ng++] = i;
    int n = ng;
    for (int i = 0; i < B; ++i)
        if (top_k[i] != 1 && !trunc(i)) rows[n++] = i;
    *n_trunc = B - n;
    for (int i = 0; i < B; ++i)
        if (top_k[i] != 1 && trunc(i)) rows[n++] = i;
    return ng;
}

int pplhip_sample_rows(pplhip_ctx* c, const float* logits_device, const pplhip_sample_rows_args* a, int32_t* output_host,
                       float* logprob_host) {
    if (!a) return PPLHIP_INVALID_VALUE;
    const pplhip_sample_rows2_args a2{a->temperatures, a->top_k, a->top_p, a->seeds, a->draws, a->batch, a->vocab_size, a->batch_stride,
                                      nullptr, nullptr};
    return pplhip_sample_rows2(c, logits_device, &a2, output_host, logprob_host);
}

int pplhip_sample_rows2(pplhip_ctx* c, const float* logits_device, const pplhip_sample_rows2_args* a, int32_t* output_host,
                        float* logprob_host) {
    if (!c || !a || !logits_device || !output_host || !logprob_host) return PPLHIP_INVALID_VALUE;
    if (!a->top_k || !a->top_p || !a->seeds || !a->draws) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int B = a->batch;
    if (int rc = check_rows(c, B, a->vocab_size, a->batch_stride, nullptr)) return rc;
    if (B == 0) return 0;
    // every array, every call, one copy: the block keeps its capacity layout, so the copy is cap_B rows long only when B is.  (A plain
    // block: the synchronisation at the end of this call is what lets the next one write it, Rank::h_srows.)
    const SampleRowsBlock h(R.h_srows, R.cap_B), d(R.d_srows, R.cap_B);
    memcpy(h.seeds, a->seeds, (size_t)B * 8);
    memcpy(h.draws, a->draws, (size_t)B * 8);
    if (a->temperatures) memcpy(h.temperatures, a->temperatures, (size_t)B * 4);
    memcpy(h.top_p, a->top_p, (size_t)B * 4);
    memcpy(h.top_k, a->top_k, (size_t)B * 4);
    int nt = 0;
    const int ng = sample_row_list(a->top_k, a->min_p, a->typical_p, B, h.rows, &nt);
    // without a truncating row: the copy and the launches of a call that carries neither array
    if (nt > 0 && a->min_p) memcpy(h.min_p, a->min_p, (size_t)B * 4);
    if (nt > 0 && a->typical_p) memcpy(h.typical_p, a->typical_p, (size_t)B * 4);
    HIPCK(c, 0, hipSetDevice(R.device));
    hipStream_t s = R.stream;
    HIPCK(c, 0, hipMemcpyAsync(R.d_srows, R.h_srows, nt > 0 ? h.upto(h.typical_p + B) : h.upto(h.rows + B), hipMemcpyHostToDevice, s));
    HIPCK(c, 0, launch_sample_rows(s, logits_device, a->temperatures ? d.temperatures : nullptr, d.top_k, d.top_p, d.seeds, d.draws, nullptr,
                                   d.rows, ng, B - ng - nt, a->vocab_size, a->batch_stride, R.d_tokout, R.d_lp,
                                   a->min_p ? d.min_p : nullptr, a->typical_p ? d.typical_p : nullptr, nt));
    HIPCK(c, 0, hipMemcpyAsync(output_host, R.d_tokout, B * 4, hipMemcpyDeviceToHost, s));
    HIPCK(c, 0, hipMemcpyAsync(logprob_host, R.d_lp, B * 4, hipMemcpyDeviceToHost, s));
    HIPCK(c, 0, hipStreamSynchronize(s));  // the one synchronisation, as in pplhip_sample
    return p2p_check(c, 0);
}

// the rows with num_logprobs[b] in 1 .. 20, ascending; returns their number, or -1 for an entry outside [0, 20]
int top_logprobs_row_list(const int32_t* num_logprobs, int B, int32_t* rows) {
    int n = 0;
    for (int i = 0; i < B; ++i) {
        if (num_logprobs[i] < 0 || num_logprobs[i] > PPLHIP_TOP_LOGPROBS_MAX) return -1;
        if (num_logprobs[i] > 0) rows[n++] = i;
    }
    return n;
}

int pplhip_top_logprobs(pplhip_ctx* c, const float* logits_device, const pplhip_top_logprobs_args* a, const int32_t** tokens_out,
                        const float** logprobs_out, int32_t* rows_out) {
    if (!c || !a || !logits_device || !tokens_out || !logprobs_out || !rows_out || !a->num_logprobs) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int B = a->batch;
    if (int rc = check_rows(c, B, a->vocab_size, a->batch_stride, nullptr)) return rc;
    const TopLogprobsIn h(R.h_tlp_in, R.cap_B), d(R.d_tlp_in, R.cap_B);
    // (the list is built in place: a refused call has launched nothing, and nothing of an earlier call still reads this block once the
    // stream was synchronised, which the contract asks for between two calls -- a plain block, Rank::h_srows says why)
    const int asked = top_logprobs_row_list(a->num_logprobs, B, h.rows);
    if (asked < 0) return fail(c, 0, PPLHIP_INVALID_VALUE, "num_logprobs outside [0, PPLHIP_TOP_LOGPROBS_MAX]");
    const TopLogprobsOut h_out(R.h_tlp_out, asked), d_out(R.d_tlp_out, asked);
    *tokens_out = h_out.tokens;
    *logprobs_out = h_out.logprobs;
    *rows_out = asked;
    if (asked == 0) return 0;   // nobody asked: no HIP call
    if (a->temperatures) memcpy(h.temperatures, a->temperatures, (size_t)B * 4);
    memcpy(h.num_logprobs, a->num_logprobs, (size_t)B * 4);
    HIPCK(c, 0, hipSetDevice(R.device));
    hipStream_t s = R.stream;
    HIPCK(c, 0, hipMemcpyAsync(R.d_tlp_in, R.h_tlp_in, h.upto(h.rows + asked), hipMemcpyHostToDevice, s));
    HIPCK(c, 0, launch_top_logprobs(s, logits_device, a->temperatures ? d.temperatures : nullptr, d.num_logprobs, d.rows, asked, a->vocab_size,
                                    a->batch_stride, d_out.tokens, d_out.logprobs));
    // (the download block is single: two calls need a synchronisation of the stream between them, include/pplhip.h)
    HIPCK(c, 0, hipMemcpyAsync(R.h_tlp_out, R.d_tlp_out, (size_t)d_out.bytes, hipMemcpyDeviceToHost, s));
    return 0;   // asynchronous: the step's sampler call (or pplhip_sync) is the synchronisation
}

// the first rule of a context: the table, the staging ring and the edit's staging block
static int logit_rules_alloc(pplhip_ctx* c) {
    Rank& R = c->ranks[0];
    const int64_t words = ((int64_t)c->d.vocab_size + 31) / 32;
    const int64_t rec = LR_MASK + (words + 3) / 4 * 16;
    int rc;
    char *table = nullptr, *d_lre = nullptr;
    if ((rc = dev_alloc(c, 0, (void**)&table, (uint64_t)R.cap_B * rec))) return rc;
    if ((rc = dev_alloc(c, 0, (void**)&d_lre, block_bytes<RowEditBlock>(R.cap_B)))) return rc;
    for (Stage& st : R.st_rule) HIPCK(c, 0, st.allocate((size_t)rec));
    HIPCK(c, 0, R.st_lre.allocate(block_bytes<RowEditBlock>(R.cap_B)));
    R.lr_has.assign((size_t)R.cap_B, 0);
    R.d_lre = d_lre;
    R.lr_rec = rec;
    R.lr_table = table;   // last: the table counts as there only when everything is
    return 0;
}

int pplhip_logit_rule_set(pplhip_ctx* c, int32_t slot, const pplhip_logit_rule* r) {
    if (!c || !r) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int V = c->d.vocab_size;
    const int64_t words = ((int64_t)V + 31) / 32;
    if (slot < 0 || slot >= R.cap_B) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: slot outside [0, max_running_batch)");
    if (r->n_bias < 0 || r->n_bias > PPLHIP_LOGIT_BIAS_MAX) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: n_bias outside [0, PPLHIP_LOGIT_BIAS_MAX]");
    if (r->n_stop < 0 || r->n_stop > PPLHIP_LOGIT_STOP_MAX) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: n_stop outside [0, PPLHIP_LOGIT_STOP_MAX]");
    if ((r->n_bias > 0 && (!r->bias_tokens || !r->bias_values)) || (r->n_stop > 0 && !r->stop_tokens))
        return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: a count without its array");
    // dead[v]: the token cannot be produced; seen[v]: it has a bias entry
    std::vector<uint8_t> dead((size_t)V, 0), seen((size_t)V, 0);
    for (int i = 0; i < r->n_bias; ++i) {
        const int32_t t = r->bias_tokens[i];
        const float v = r->bias_values[i];
        if (t < 0 || t >= V) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: bias_tokens[" + std::to_string(i) + "] outside [0, vocab_size)");
        if (v != v || v == INFINITY) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: bias_values[" + std::to_string(i) + "] is NaN or +inf");
        if (seen[t]) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: bias_tokens[" + std::to_string(i) + "] has an entry already");
        seen[t] = 1;
        if (v == -INFINITY) dead[t] = 1;
    }
    for (int i = 0; i < r->n_stop; ++i) {
        const int32_t t = r->stop_tokens[i];
        if (t < 0 || t >= V) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: stop_tokens[" + std::to_string(i) + "] outside [0, vocab_size)");
        dead[t] = 1;
    }
    bool alive = false;
    for (int v = 0; v < V && !alive; ++v)
        alive = !dead[v] && (!r->allowed_bits || ((r->allowed_bits[v >> 5] >> (v & 31)) & 1u));
    if (!alive) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit rule: allowed_bits minus the banned and stop tokens leaves no token");
    HIPCK(c, 0, hipSetDevice(R.device));
    if (!R.lr_table)
        if (int rc = logit_rules_alloc(c)) return rc;
    Stage& record = R.st_rule[R.lr_next];
    char* h;
    HIPCK(c, 0, record.begin(&h));
    int32_t* head = (int32_t*)h;
    head[0] = r->n_bias; head[1] = r->n_stop; head[2] = r->allowed_bits ? 1 : 0; head[3] = 0;
    if (r->n_bias) {
        memcpy(h + LR_BIAS_TOK, r->bias_tokens, (size_t)r->n_bias * 4);
        memcpy(h + LR_BIAS_VAL, r->bias_values, (size_t)r->n_bias * 4);
    }
    if (r->n_stop) memcpy(h + LR_STOPS, r->stop_tokens, (size_t)r->n_stop * 4);
    if (r->allowed_bits) memcpy(h + LR_MASK, r->allowed_bits, (size_t)words * 4);
    // (the parts behind the counts, and the mask of a rule without one, go up as the ring holds them: the kernel reads none of it)
    HIPCK(c, 0, record.upload(R.lr_table + (int64_t)slot * R.lr_rec, (size_t)R.lr_rec, R.stream));
    R.lr_next = (R.lr_next + 1) % LR_RING;
    R.lr_has[slot] = 1;
    return 0;
}

int pplhip_logit_edit(pplhip_ctx* c, float* logits_device, const pplhip_logit_edit_args* a) {
    if (!c || !a || !logits_device || !a->batch_slots || !a->flags) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int B = a->batch;
    if (int rc = check_rows(c, B, a->vocab_size, a->batch_stride, "logit edit")) return rc;
    int asked = 0;
    for (int i = 0; i < B; ++i) {
        if (a->flags[i] > 3u) return fail(c, 0, PPLHIP_INVALID_VALUE, "logit edit: flags above 3");
        if (!a->flags[i]) continue;
        const int64_t slot = a->batch_slots[i];
        if (slot < 0 || slot >= R.cap_B || !R.lr_table || !R.lr_has[slot])
            return fail(c, 0, PPLHIP_INVALID_VALUE, "logit edit: row " + std::to_string(i) + " asks with a slot that holds no rule");
        ++asked;
    }
    if (asked == 0) return 0;   // nobody asks: no HIP call
    HIPCK(c, 0, hipSetDevice(R.device));
    char* hbuf;
    HIPCK(c, 0, R.st_lre.begin(&hbuf));
    const RowEditBlock h(hbuf, R.cap_B), d(R.d_lre, R.cap_B);
    int n = 0;
    for (int i = 0; i < B; ++i) {
        h.slots[i] = a->flags[i] ? (int32_t)a->batch_slots[i] : 0;
        h.arg[i] = (int32_t)a->flags[i];
        if (a->flags[i]) h.rows[n++] = i;
    }
    hipStream_t s = R.stream;
    HIPCK(c, 0, R.st_lre.upload(R.d_lre, h.upto(h.rows + asked), s));
    const int64_t rw = R.lr_rec / 4;
    const LogitRuleTable tb{(const int32_t*)R.lr_table, (const int32_t*)(R.lr_table + LR_BIAS_TOK), (const float*)(R.lr_table + LR_BIAS_VAL),
                            (const int32_t*)(R.lr_table + LR_STOPS), (const uint32_t*)(R.lr_table + LR_MASK), rw, rw, rw, rw};
    HIPCK(c, 0, launch_logit_edit(s, logits_device, a->batch_stride, a->vocab_size, d.rows, asked, d.slots, (const uint32_t*)d.arg, tb));
    return 0;   // asynchronous: in stream order in front of the step's penalty, top-N logprobs and sampler
}

// ---- guided decoding ----------------------------------------------------------------------------------------------------------------

int pplhip_guide_set_vocab(pplhip_ctx* c, const uint8_t* bytes, const int64_t* offsets, int32_t n_tok) {
    if (!c || !offsets) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    if (R.gd_n_tok >= 0) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide vocabulary: set already");
    if (n_tok < 1 || n_tok > c->d.vocab_size) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide vocabulary: n_tok outside [1, vocab_size]");
    if (offsets[0] != 0) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide vocabulary: offsets[0] is not 0");
    for (int i = 0; i < n_tok; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide vocabulary: offsets decrease at token " + std::to_string(i));
    const int64_t total = offsets[n_tok];
    if (total > 0 && !bytes) return PPLHIP_INVALID_VALUE;
    HIPCK(c, 0, hipSetDevice(R.device));
    uint8_t* d_bytes = nullptr;
    int64_t* d_off = nullptr;
    // (freed by pplhip_destroy even when a later step of this call fails: the fields are set as they come)
    HIPCK(c, 0, hipMalloc((void**)&d_bytes, (size_t)std::max<int64_t>(total, 1)));
    R.gd_bytes = d_bytes;
    HIPCK(c, 0, hipMalloc((void**)&d_off, (size_t)(n_tok + 1) * 8));
    R.gd_off = d_off;
    HIPCK(c, 0, R.st_gde.allocate(block_bytes<RowEditBlock>(R.cap_B)));
    if (!R.d_gde)
        if (int rc = dev_alloc(c, 0, (void**)&R.d_gde, block_bytes<RowEditBlock>(R.cap_B))) return rc;
    if (total > 0) HIPCK(c, 0, hipMemcpyAsync(d_bytes, bytes, (size_t)total, hipMemcpyHostToDevice, R.stream));
    HIPCK(c, 0, hipMemcpyAsync(d_off, offsets, (size_t)(n_tok + 1) * 8, hipMemcpyHostToDevice, R.stream));
    HIPCK(c, 0, hipStreamSynchronize(R.stream));   // the caller's arrays are pageable and free after this call
    R.gd_n_tok = n_tok;
    return 0;
}

// pplhip_guide_load and pplhip_guide_load16: T is the table's state type, `dead` its dead state, max_states / max_name the bound of n_states
template <typename T, typename Desc, typename Launch>
static int guide_load(pplhip_ctx* c, int32_t slot, const Desc* g, int dead, int max_states, const char* max_name, Launch launch) {
    if (!c || !g) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int V = c->d.vocab_size;
    if (R.gd_n_tok < 0) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: no vocabulary set (pplhip_guide_set_vocab)");
    if (slot < 0 || slot >= PPLHIP_GUIDE_MAX_SLOTS) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: slot outside [0, PPLHIP_GUIDE_MAX_SLOTS)");
    if (R.gd_mask[slot]) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: slot " + std::to_string(slot) + " is loaded");
    const int S = g->n_states;
    if (S < 1 || S > max_states) return fail(c, 0, PPLHIP_INVALID_VALUE, std::string("guide: n_states outside [1, ") + max_name + "]");
    if (g->n_end < 0 || g->n_end > PPLHIP_LOGIT_STOP_MAX) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: n_end outside [0, PPLHIP_LOGIT_STOP_MAX]");
    if (!g->trans || !g->accept || (g->n_end > 0 && !g->end_tokens)) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: a NULL array");
    for (int i = 0; i < g->n_end; ++i)
        if (g->end_tokens[i] < 0 || g->end_tokens[i] >= V)
            return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: end_tokens[" + std::to_string(i) + "] outside [0, vocab_size)");
    for (int s = 0; s < S; ++s) {
        bool live = g->accept[s] != 0;
        for (int b = 0; b < 256; ++b) {
            const int to = g->trans[s * 256 + b];
            if (to != dead && to >= S)
                return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: state " + std::to_string(s) + " byte " + std::to_string(b) + " leads to state " +
                                                            std::to_string(to) + " >= n_states");
            live = live || to != dead;
        }
        if (!live) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: state " + std::to_string(s) + " has neither a live byte nor acceptance");
    }
    HIPCK(c, 0, hipSetDevice(R.device));
    const int64_t words = ((int64_t)V + 31) / 32;
    // one scratch block: trans | accept (padded to 256) | any u32 (a multiple of 256 of them) | end tokens i32 [64]
    const size_t pad = ((size_t)S + 255) / 256 * 256;
    const size_t o_acc = (size_t)S * 256 * sizeof(T), o_any = o_acc + pad, o_end = o_any + pad * 4, scratch_bytes = o_end + 256;
    char* scratch = nullptr;
    uint32_t* mask = nullptr;
    std::vector<uint32_t> any((size_t)S, 0);
    hipError_t e = hipMalloc((void**)&scratch, scratch_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&mask, (size_t)S * words * 4);
    hipStream_t s = R.stream;
    if (e == hipSuccess) e = hipMemsetAsync(scratch + o_any, 0, pad * 4, s);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch, g->trans, (size_t)S * 256 * sizeof(T), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch + o_acc, g->accept, (size_t)S, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && g->n_end > 0) e = hipMemcpyAsync(scratch + o_end, g->end_tokens, (size_t)g->n_end * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = launch(s, (const T*)scratch, (const uint8_t*)(scratch + o_acc), S, R.gd_bytes, R.gd_off, R.gd_n_tok,
                   (const int32_t*)(scratch + o_end), g->n_end, V, mask, words, (uint32_t*)(scratch + o_any));
    if (e == hipSuccess) e = hipMemcpyAsync(any.data(), scratch + o_any, (size_t)S * 4, hipMemcpyDeviceToHost, s);
    const hipError_t e_sync = hipStreamSynchronize(s);   // synchronous by design: once per distinct pattern
    if (e == hipSuccess) e = e_sync;
    if (scratch) hipFree(scratch);
    if (e != hipSuccess) {
        if (mask) hipFree(mask);
        return fail(c, 0, e == hipErrorOutOfMemory ? PPLHIP_OUT_OF_MEMORY : PPLHIP_DEVICE_RUNTIME_ERROR, std::string("guide load: ") + hipGetErrorString(e));
    }
    for (int st = 0; st < S; ++st)
        if (!any[st]) {
            hipFree(mask);
            return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: state " + std::to_string(st) + " allows no token of the vocabulary");
        }
    R.gd_mask[slot] = mask;
    R.gd_states[slot] = S;
    return 0;
}

int pplhip_guide_load(pplhip_ctx* c, int32_t slot, const pplhip_guide_desc* g) {
    return guide_load<uint8_t>(c, slot, g, GUIDE_DEAD, PPLHIP_GUIDE_MAX_STATES, "PPLHIP_GUIDE_MAX_STATES", launch_guide_build);
}

int pplhip_guide_load16(pplhip_ctx* c, int32_t slot, const pplhip_guide_desc16* g) {
    return guide_load<uint16_t>(c, slot, g, GUIDE16_DEAD, PPLHIP_GUIDE16_MAX_STATES, "PPLHIP_GUIDE16_MAX_STATES", launch_guide_build16);
}

int32_t pplhip_guide16_state_chunk(void) { return GUIDE16_STATE_CHUNK; }

int pplhip_guide_unload(pplhip_ctx* c, int32_t slot) {
    if (!c) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    if (slot < 0 || slot >= PPLHIP_GUIDE_MAX_SLOTS || !R.gd_mask[slot]) return fail(c, 0, PPLHIP_INVALID_VALUE, "guide: slot is not loaded");
    HIPCK(c, 0, hipSetDevice(R.device));
    HIPCK(c, 0, hipStreamSynchronize(R.stream));   // a queued pplhip_guide_edit may still read the mask
    HIPCK(c, 0, hipFree(R.gd_mask[slot]));
    R.gd_mask[slot] = nullptr;
    R.gd_states[slot] = 0;
    return 0;
}

int pplhip_guide_edit(pplhip_ctx* c, float* logits_device, const pplhip_guide_edit_args* a) {
    if (!c || !a || !logits_device || !a->guide_slots || !a->states) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    const int B = a->batch;
    if (int rc = check_rows(c, B, a->vocab_size, a->batch_stride, "guide edit")) return rc;
    int asked = 0;
    for (int i = 0; i < B; ++i) {
        const int32_t slot = a->guide_slots[i];
        if (slot == -1) continue;
        if (slot < 0 || slot >= PPLHIP_GUIDE_MAX_SLOTS || !R.gd_mask[slot])
            return fail(c, 0, PPLHIP_INVALID_VALUE, "guide edit: row " + std::to_string(i) + " asks with a slot that holds no guide");
        if (a->states[i] < 0 || a->states[i] >= R.gd_states[slot])
            return fail(c, 0, PPLHIP_INVALID_VALUE, "guide edit: row " + std::to_string(i) + " is in a state outside its guide");
        ++asked;
    }
    if (asked == 0) return 0;   // nobody asks: no HIP call
    HIPCK(c, 0, hipSetDevice(R.device));
    char* hbuf;
    HIPCK(c, 0, R.st_gde.begin(&hbuf));
    const RowEditBlock h(hbuf, R.cap_B), d(R.d_gde, R.cap_B);
    int n = 0;
    for (int i = 0; i < B; ++i) {
        h.slots[i] = a->guide_slots[i];
        h.arg[i] = a->guide_slots[i] >= 0 ? a->states[i] : 0;
        if (a->guide_slots[i] >= 0) h.rows[n++] = i;
    }
    hipStream_t s = R.stream;
    HIPCK(c, 0, R.st_gde.upload(R.d_gde, h.upto(h.rows + asked), s));
    GuideTable tb;
    for (int i = 0; i < GUIDE_MAX_SLOTS; ++i) tb.mask[i] = R.gd_mask[i];
    tb.mask_stride = ((int64_t)a->vocab_size + 31) / 32;
    HIPCK(c, 0, launch_guide_mask(s, logits_device, a->batch_stride, a->vocab_size, d.rows, asked, d.slots, d.arg, tb));
    return 0;   // asynchronous: in stream order in front of the step's logit edit, penalty, top-N logprobs and sampler
}

int pplhip_penalty(pplhip_ctx* c, float* logits_device, const pplhip_penalty_args* a) {
    if (!c || !a || !logits_device) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[0];
    if (!R.count_map) return fail(c, 0, PPLHIP_INVALID_VALUE, "context was created without enable_penalty");
    const int B = a->batch;
    if (B < 0 || B > R.cap_B || B != R.B) return fail(c, 0, PPLHIP_INVALID_VALUE, "penalty batch does not match the step");
    HIPCK(c, 0, hipSetDevice(R.device));
    hipStream_t s = R.stream;
    if (a->req_list_changed) {  // post_processor.cc:231-263
        HIPCK(c, 0, hipMemcpyAsync(R.d_ptemp, a->temperatures, B * 4, hipMemcpyHostToDevice, s));
        HIPCK(c, 0, hipMemcpyAsync(R.d_slots, a->batch_slots, B * 8, hipMemcpyHostToDevice, s));
        HIPCK(c, 0, hipMemcpyAsync(R.d_rep, a->repetition_penalties, B * 4, hipMemcpyHostToDevice, s));
        if (a->presence_penalties) HIPCK(c, 0, hipMemcpyAsync(R.d_pres, a->presence_penalties, B * 4, hipMemcpyHostToDevice, s));
        if (a->frequency_penalties) HIPCK(c, 0, hipMemcpyAsync(R.d_freq, a->frequency_penalties, B * 4, hipMemcpyHostToDevice, s));
    }
    HIPCK(c, 0, launch_penalty(s, logits_device, R.d_ptemp, R.d_rep, a->presence_penalties ? R.d_pres : nullptr,
                               a->frequency_penalties ? R.d_freq : nullptr, R.d_slots, R.d_tok, R.d_seq, R.d_sp, B,
                               a->vocab_size, c->d.vocab_size, (int)R.decoding_batches, R.count_map));
    return 0;
}

// ---- prompt logprobs -------------------------------------------------------------------------------------------------------------------
// the first ask of a rank: the device blocks, the staging block and the pinned block of the download
static int prompt_logprobs_alloc(pplhip_ctx* c, int rank) {
    Rank& R = c->ranks[rank];
    const int64_t cap = R.cap_T;
    int rc;
    char *d_in = nullptr, *d_out = nullptr;
    if ((rc = dev_alloc(c, rank, (void**)&d_in, block_bytes<PromptLogprobsIn>(cap)))) return rc;
    if ((rc = dev_alloc(c, rank, (void**)&d_out, block_bytes<PromptLogprobsOut>(cap)))) return rc;
    HIPCK(c, rank, R.st_plp.allocate(block_bytes<PromptLogprobsIn>(cap)));
    if (!R.h_plp_out) HIPCK(c, rank, hipHostMalloc((void**)&R.h_plp_out, block_bytes<PromptLogprobsHost>(cap), hipHostMallocDefault));
    R.d_plp_out = d_out;
    R.d_plp_in = d_in;   // last: the blocks count as there only when all of them are
    return 0;
}

int pplhip_set_prompt_logprobs(pplhip_ctx* c, int rank, const int32_t* ask, int64_t batch) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    if (c->tp > 1 || c->tp_on)
        return fail(c, rank, PPLHIP_UNSUPPORTED, "prompt logprobs under tensor parallelism (world_size > 1) are not supported: the lm_head is vocabulary-sharded");
    if (!ask || batch != R.B) return fail(c, rank, PPLHIP_INVALID_VALUE, "pplhip_set_prompt_logprobs: one entry per request of the staged step");
    R.plp_n = 0;
    R.plp_top = false;
    int64_t P = 0;
    bool top = false;
    for (int64_t b = 0; b < batch; ++b) {
        if (ask[b] < -1 || ask[b] > PPLHIP_TOP_LOGPROBS_MAX)
            return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + ": prompt logprobs ask outside [-1, PPLHIP_TOP_LOGPROBS_MAX]");
        if (ask[b] < 0) continue;
        const int64_t len = R.h_seq[b + 1] - R.h_seq[b];   // (batch == R.B > 0: pplhip_set_inputs staged and validated seq_starts)
        if (len < 2) continue;
        P += len - 1;
        top = top || ask[b] > 0;
    }
    if (P == 0) return 0;   // exactly the step without the ask
    HIPCK(c, rank, hipSetDevice(R.device));
    if (!R.d_plp_in)
        if (int rc = prompt_logprobs_alloc(c, rank)) return rc;
    char* hbuf;
    HIPCK(c, rank, R.st_plp.begin(&hbuf));
    const PromptLogprobsIn h(hbuf, P);
    R.plp_rows.clear();
    h.gather[0] = 0;   // never read
    int64_t j = 0;
    for (int64_t b = 0; b < batch; ++b) {
        if (ask[b] < 0) continue;
        for (int64_t r = R.h_seq[b]; r + 1 < R.h_seq[b + 1]; ++r, ++j) {   // the request's last row predicts its first generated token
            h.gather[j + 1] = r + 1;
            h.rows[j] = (int32_t)r;
            R.plp_rows.push_back((int32_t)r);
            h.n_top[j] = ask[b];
        }
    }
    HIPCK(c, rank, R.st_plp.upload(R.d_plp_in, (size_t)h.bytes, R.stream));
    R.plp_n = P;
    R.plp_top = top;
    return 0;
}

int pplhip_prompt_logprobs(pplhip_ctx* c, int rank, pplhip_prompt_logprobs_out* out) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !out) return PPLHIP_INVALID_VALUE;
    const Rank& R = c->ranks[rank];
    memset(out, 0, sizeof(*out));
    const int64_t P = R.plp_done;
    if (P == 0) return 0;
    out->positions = P;
    const PromptLogprobsHost host(R.h_plp_out, R.cap_T);
    const PromptLogprobsOut h(host.out, P);
    out->rows = host.rows;
    out->logprobs = h.logprobs;
    out->ranks = h.ranks;
    out->top_tokens = h.top_tokens;
    out->top_logprobs = h.top_logprobs;
    return 0;
}

// The asked prompt rows of the staged step, in front of the step's own K11 and through its buffers: R.hn and R.logits are free until the
// step's own norm and lm_head write them, and a chunk of cap_B rows is the largest M they were sized for.  Per chunk: the final
// (Skip)RMSNorm of the chunk's rows, the lm_head, one workgroup per position; then one download for all chunks.
// The rows are selected with the norm's gathering form (row gather[j + 1] - 1).  Checked in rmsnorm_kernel (k_elem.hip): called without
// residual_out, as K11 calls it, the kernel folds the skip operand (part2 or its split-K slabs) into the row IN REGISTERS only -- R.h and
// the skip operand are read, never written -- so nothing is folded twice, neither between two chunks nor between these rows and the last
// rows the step's own K11 norm gathers afterwards (the two sets are disjoint anyway).
// When the last layer's w2 left its split-K slabs unreduced in the workspace (sl_part2), the step's own norm still has to read them: the
// lm_head here then runs without the workspace (no split-K) instead of overwriting them.
int run_prompt_logprobs(pplhip_ctx* c, int rank, hipStream_t s, const uint16_t* pending, const SplitSlabs& sl_part2) {
    Rank& R = c->ranks[rank];
    const pplhip_model_desc& d = c->d;
    const int hd = d.hidden_dim, V = d.vocab_size;
    const int64_t P = R.plp_n;
    const bool slabs = pending && sl_part2.splits > 0;
    const PromptLogprobsIn in(R.d_plp_in, P);
    const PromptLogprobsOut o(R.d_plp_out, P);
    for (int64_t c0 = 0; c0 < P; c0 += R.cap_B) {
        const int64_t cn = std::min<int64_t>(R.cap_B, P - c0);
        HIPCK(c, rank, launch_rmsnorm(s, R.h, pending, R.norm, d.norm_eps, cn, hd, in.gather + c0, R.hn, nullptr, nullptr, nullptr, pending ? &sl_part2 : nullptr));
        HIPCK(c, rank, launch_linear(s, R.hn, R.output.w, nullptr, 0, 0, cn, R.output.N, hd, R.logits, V, true, slabs ? nullptr : R.gemm_ws,
                                     slabs ? 0 : R.gemm_ws_bytes));
        HIPCK(c, rank, launch_prompt_logprobs(s, R.logits, V, V, in.rows + c0, (int)cn, R.d_tok, in.n_top + c0, o.logprobs + c0, o.ranks + c0,
                                              o.top_tokens + c0 * PPLHIP_TOP_LOGPROBS_MAX, o.top_logprobs + c0 * PPLHIP_TOP_LOGPROBS_MAX));
    }
    const PromptLogprobsHost host(R.h_plp_out, R.cap_T);
    memcpy(host.rows, R.plp_rows.data(), (size_t)P * 4);   // the rows, where the next step's staging leaves them alone
    HIPCK(c, rank, hipMemcpyAsync(host.out, R.d_plp_out, R.plp_top ? (size_t)o.bytes : o.upto(o.top_tokens), hipMemcpyDeviceToHost, s));
    R.plp_done = P;
    return 0;
}
