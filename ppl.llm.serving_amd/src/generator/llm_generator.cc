#include "llm_generator.h"

#include <random>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>

#include "../utils/utils.h"
#include "ppl/common/log.h"

using namespace ppl::common;

namespace ppl { namespace llm {

// scratch of one admission check (reference RequestCheckResult, llm_generator.cc:31-43)
struct LLMGenerator::Admission {
    int64_t cache_index = INT64_MAX;
    std::vector<int64_t> page_list;
    int64_t slot_index = INT64_MAX;
    int rest_iters = -1;
    int first_fill_len = 0;
    int total_tokens_per_step = 0;
    std::vector<uint64_t> hash_list;
    int64_t cache_hit_count = 0;
    int32_t running_batch = 0;
    int32_t prefill_batch = 0;
    std::string errmsg;
    RetCode errcode = RC_INVALID_VALUE;
    bool has_rule = false;  // the request carries a logit rule: `rule` is its validated, merged form
    LogitRule rule;
    int32_t guide_slot = -1;  // the request is guided: the slot it holds a reference on

    void ResetForRequest(int prompt_len) {
        errcode = RC_INVALID_VALUE;
        has_rule = false;
        guide_slot = -1;
        cache_index = INT64_MAX;
        page_list.clear();
        slot_index = INT64_MAX;
        rest_iters = -1;
        first_fill_len = prompt_len;
        hash_list.clear();
        cache_hit_count = 0;
        errmsg.clear();
    }
};

LLMGenerator::LLMGenerator(const Resource& resource, const GeneratorConfig& generator_config, const ModelConfig& model_config,
                           Connection* conn)
    : tokenizer_(resource.tokenizer)
    , adapters_(resource.adapters)
    , generator_config_(generator_config)
    , model_config_(model_config)
    , conn_(conn)
    , kv_cache_max_tokens_(resource.kv_cache_max_tokens)
    , llm_engine_(resource, model_config, generator_config.enable_penalty, generator_config.top_k, generator_config.top_p,
                  generator_config.per_request_sampling) {
    if (generator_config_.per_request_sampling && generator_config_.sampling_seed == 0) {
        std::random_device rd;
        generator_config_.sampling_seed = ((uint64_t)rd() << 32) | rd();
    }
    idx_mgr_.Init(kv_cache_max_tokens_);
    batch_slots_mgr_.Init(generator_config.max_running_batch);
    page_mgr_.Init(kv_cache_max_tokens_, model_config_.page_size);
    worker_profiler_ = std::make_shared<WorkerProfiler>();
}

LLMGenerator::~LLMGenerator() {
    if (generate_thread_active_.load(std::memory_order_relaxed)) {
        generate_thread_active_.store(false, std::memory_order_release);
        req_signal_.NotifyOne();
        pthread_join(generate_thread_, nullptr);
    }
    // the backend outlives the generator: its guide slots go back, so that the next generator finds them empty
    for (int32_t i = 0; i < PostProcessor::kGuideMaxSlots; ++i)
        if (!guides_[i].key.empty()) llm_engine_.UnloadGuide(i);
}

// reference CheckParameters, llm_generator.cc:114-144 (accepted combinations: SURVEY.md Q9)
RetCode LLMGenerator::CheckParameters() const {
    const ModelConfig& m = model_config_;
    if (!m.auto_causal) { LOG(ERROR) << "only support auto_causal == true"; return RC_INVALID_VALUE; }
    if (m.cache_mode != 0 && m.cache_mode != 1) { LOG(ERROR) << "unsupported cache_mode: " << m.cache_mode; return RC_INVALID_VALUE; }
    if (m.cache_layout < 0 || m.cache_layout > 3) { LOG(ERROR) << "only support cache_layout 0..3"; return RC_INVALID_VALUE; }
    const bool int8_kv = m.cache_quant_bit == 8 && m.cache_quant_group == 8;
    const bool fp16_kv = m.cache_quant_bit == 0 && m.cache_quant_group == 1;
    // this project's fp8 e4m3 KV cache: group = head_dim (one power-of-two scale per head row; the reference has no such pair)
    const int head_dim = m.num_heads > 0 ? m.hidden_dim / m.num_heads : 0;
    const bool fp8_kv = m.cache_quant_bit == 8 && m.cache_quant_group == head_dim && (head_dim == 32 || head_dim == 64 || head_dim == 128);
    // this project's int4 KV cache: one fp16 scale per 32 channels (the reference has no such pair either)
    const bool int4_kv = m.cache_quant_bit == 4 && m.cache_quant_group == 32 && (head_dim == 32 || head_dim == 64 || head_dim == 128);
    if (!int8_kv && !fp16_kv && !fp8_kv && !int4_kv) {
        LOG(ERROR) << "only support (cache_quant_bit == 8 and cache_quant_group == 8), (cache_quant_bit == 8 and cache_quant_group == "
                      "head_dim), (cache_quant_bit == 4 and cache_quant_group == 32, head_dim 32 / 64 / 128) or (cache_quant_bit == 0 and "
                      "cache_quant_group == 1)";
        return RC_INVALID_VALUE;
    }
    if (!m.dynamic_batching) { LOG(ERROR) << "only support dynamic_batching == true"; return RC_INVALID_VALUE; }
    if (m.cache_mode == 1 && m.page_size <= 0) { LOG(ERROR) << "cache_mode 1 needs page_size > 0"; return RC_INVALID_VALUE; }
    return RC_SUCCESS;
}

RetCode LLMGenerator::Init() {
    RetCode rc = CheckParameters();
    if (rc != RC_SUCCESS) { LOG(ERROR) << "CheckParameters failed."; return rc; }
    rc = llm_engine_.Init(&worker_profiler_->step_counter);
    if (rc != RC_SUCCESS) { LOG(ERROR) << "LLM Engine Init failed."; return rc; }
    // the rope table (and pplhip_set_inputs' range check) ends at max_position: a request may never grow past it, or one
    // long request would fail Execute for the whole running batch.  Clamp per request at admission instead.
    if (model_config_.max_position > 0 && generator_config_.max_total_tokens_per_request > model_config_.max_position) {
        LOG(WARNING) << "max_total_tokens_per_request [" << generator_config_.max_total_tokens_per_request
                     << "] > model max_position [" << model_config_.max_position << "]. use [" << model_config_.max_position << "]";
        generator_config_.max_total_tokens_per_request = model_config_.max_position;
    }
    rc = decoder_thread_pool_.Init(DECODER_THREAD_NUM);
    if (rc != RC_SUCCESS) { LOG(ERROR) << "Init decoder thread pool error"; return RC_OTHER_ERROR; }
    generate_thread_active_.store(true, std::memory_order_release);
    if (pthread_create(&generate_thread_, nullptr, GeneratorThreadFunc, this) != 0) {
        generate_thread_active_.store(false, std::memory_order_relaxed);
        LOG(ERROR) << "create generator thread failed.";
        return RC_OTHER_ERROR;
    }
    return RC_SUCCESS;
}

// reference Process, llm_generator.cc:788-814
void LLMGenerator::Process(const std::shared_ptr<Request>& req) {
    uint64_t encode_cost = 0;
    if (req->token_ids) req->is_token_in_out = true;
    {
        utils::TimingGuard timing(&encode_cost);
        if (!req->is_token_in_out) {
            if (!tokenizer_) {
                conn_->NotifyFailure(req->id, RC_UNSUPPORTED, "no tokenizer: only token-in/token-out requests are accepted");
                return;
            }
            req->token_ids = std::make_shared<std::vector<int>>();
            tokenizer_->Encode(req->prompt.data(), (uint32_t)req->prompt.size(), req->token_ids.get());
            req->stop_tokens = std::make_shared<std::unordered_set<int>>();
            req->stop_tokens->insert(tokenizer_->GetEosId());
            conn_->OnTokenize(req->id, *req->token_ids);
        }
    }
    worker_profiler_->step_counter.global.input_token_cnt += req->token_ids->size();
    ++worker_profiler_->req_counter.encode_cnt;
    worker_profiler_->req_counter.encode_cost += encode_cost;

    uint64_t lora_uid = 0;
    if (req->lora_slot != -1 && !(adapters_ && adapters_->Acquire(req->lora_slot, &lora_uid))) {
        conn_->NotifyFailure(req->id, RC_INVALID_VALUE, "adapter slot [" + std::to_string(req->lora_slot) + "] is not loaded");
        return;
    }
    auto* lreq = new LlmRequest();
    lreq->orig = req;
    lreq->lora_uid = lora_uid;
    lreq->enqueue_ts = std::chrono::high_resolution_clock::now();
    if (sched_.PushRequest(lreq)) req_signal_.NotifyOne();
}

// reference GeneratorThreadFunc, llm_generator.cc:342-366
void* LLMGenerator::GeneratorThreadFunc(void* arg) {
    auto* g = static_cast<LLMGenerator*>(arg);
    while (true) {
        while (true) {
            const auto key = g->req_signal_.PrepareWait();
            if (!g->generate_thread_active_.load(std::memory_order_acquire)) {
                g->req_signal_.CancelWait();
                return nullptr;
            }
            if (g->sched_.GetPendingSize() > 0) {
                g->generating_.store(true, std::memory_order_release);
                g->req_signal_.CancelWait();
                break;
            }
            LOG(INFO) << "waiting for request ...";
            g->req_signal_.CommitWait(key);
        }
        g->generating_.store(true, std::memory_order_release);
        g->Generate();
        g->generating_.store(false, std::memory_order_release);
    }
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ admission

// length clamps: reference CheckTotalLen, llm_generator.cc:441-478 (including that the total-length clamp is
// computed from the REQUESTED generation length and may exceed max_output_tokens_per_request)
static bool ClampLengths(const GeneratorConfig& cfg, const Request& r, int* first_fill_len, int* rest_iters, std::string* errmsg) {
    const std::string idstr = "id [" + std::to_string(r.id) + "]";
    if (*first_fill_len > cfg.max_input_tokens_per_request) {
        *errmsg = idstr + " invalid input token len: " + std::to_string(*first_fill_len) +
                  ", server allowed max input len: " + std::to_string(cfg.max_input_tokens_per_request);
        *first_fill_len = -1;
        return false;
    }
    *rest_iters = r.generation_length;
    if (r.generation_length > cfg.max_output_tokens_per_request) {
        const std::string msg = idstr + ": generation len in request is [" + std::to_string(r.generation_length) + "] > [" +
                                std::to_string(cfg.max_output_tokens_per_request) + "] from cmd. use [" +
                                std::to_string(cfg.max_output_tokens_per_request) + "]";
        LOG(WARNING) << msg;
        *rest_iters = cfg.max_output_tokens_per_request;
        if (*rest_iters <= 0) { *errmsg = msg; return false; }
    }
    if (*first_fill_len + r.generation_length > cfg.max_total_tokens_per_request) {
        const int clamped = cfg.max_total_tokens_per_request - *first_fill_len;
        const std::string msg = idstr + ": total len in request is [" + std::to_string(*first_fill_len + r.generation_length) +
                                "] > [" + std::to_string(cfg.max_total_tokens_per_request) + "] from cmd. use [" +
                                std::to_string(clamped) + "]";
        LOG(WARNING) << msg;
        *rest_iters = clamped;
        if (*rest_iters <= 0) { *errmsg = msg; return false; }
    }
    return true;
}

// KV reservation for the request's whole lifetime, total_len = prompt + rest_iters - 1 tokens, up front
// (reference CheckAndAllocGPUMemory, llm_generator.cc:480-572)
bool LLMGenerator::ReserveKv(const LlmRequest& req, Admission* adm, int32_t* cool_down, bool* is_prefix_cache_hit) {
    const uint64_t total_len = (uint64_t)adm->first_fill_len + adm->rest_iters - 1;
    if (model_config_.cache_mode == 0) {
        adm->cache_index = idx_mgr_.Alloc(total_len);
        if (adm->cache_index == INT64_MAX) {
            // wait until a few running requests finish before trying again (llm_generator.cc:488-492)
            const int running = (int)tid_list_.size();
            *cool_down = std::min(std::max(1, (int)floorf(running * 0.1f)), generator_config_.max_cooldown_request);
            return false;
        }
    } else if (generator_config_.enable_prefix_cache) {
        const std::vector<int>& tokens = *req.orig->token_ids;
        const int64_t P = model_config_.page_size;
        // 1. longest chain of cached full pages: h_i = HashCombine(h_{i-1}, page i tokens)
        // (the chain of a request on an adapter starts from the adapter's uid: its K/V are not the base model's, nor another adapter's)
        // A request that asks for prompt logprobs matches nothing: a cached prefix has no hidden states to score, so its prefill starts at
        // position 0 and every position is computed.  It still publishes its pages in step 3, up to the first one that is cached already
        // (an existing hash keeps its page, and a request's published pages are the leading ones of its list).
        const bool scores_prompt = req.orig->prompt_logprobs >= 0;
        uint64_t prev_hash = req.lora_uid, start = 0;
        for (; !scores_prompt && start + P <= tokens.size(); start += P) {
            const uint64_t h = utils::HashCombine(prev_hash, tokens.data() + start, (int32_t)P);
            const int64_t page_id = prefix_cache_mgr_.Find(h);
            if (page_id == -1) break;
            prev_hash = h;
            adm->page_list.push_back(page_id);
            adm->hash_list.push_back(h);
        }
        prefix_cache_mgr_.IncRefCount(adm->hash_list.data(), (int64_t)adm->hash_list.size());
        // 2. pages still needed; evict unreferenced cached pages if the pool is short
        const int64_t avail = page_mgr_.GetAvail();
        const int64_t need = ((int64_t)total_len - (int64_t)start + P - 1) / P;
        if (avail < need) {
            std::vector<int64_t> evicted;
            prefix_cache_mgr_.Evict(need - avail, &evicted);
            page_mgr_.Free(evicted.data(), (int64_t)evicted.size());
            if ((int64_t)evicted.size() < need - avail) {
                prefix_cache_mgr_.DecRefCount(adm->hash_list.data(), (int64_t)adm->hash_list.size());
                return false;
            }
        }
        adm->cache_hit_count = (int64_t)adm->hash_list.size() * P;
        worker_profiler_->step_counter.global.cache_hit_count += adm->cache_hit_count;
        if (adm->cache_hit_count != 0) {
            *is_prefix_cache_hit = true;
            LOG(INFO) << "Cache Hit [" << adm->cache_hit_count << "]/[" << tokens.size() << "] input tokens";
        }
        if (page_mgr_.Alloc(need, &adm->page_list) != RC_SUCCESS) {
            LOG(WARNING) << "page alloc failed after eviction";
            prefix_cache_mgr_.DecRefCount(adm->hash_list.data(), (int64_t)adm->hash_list.size());
            return false;
        }
        // 3. publish the remaining full prompt pages
        for (uint64_t pos = start; pos + P <= tokens.size(); pos += P) {
            const uint64_t h = utils::HashCombine(prev_hash, tokens.data() + pos, (int32_t)P);
            if (scores_prompt && prefix_cache_mgr_.Find(h) != -1) break;
            prefix_cache_mgr_.Insert(h, adm->page_list[pos / P]);
            prev_hash = h;
            adm->hash_list.push_back(h);
        }
    } else {
        const int64_t pages = ((int64_t)total_len + model_config_.page_size - 1) / model_config_.page_size;
        if (page_mgr_.Alloc(pages, &adm->page_list) != RC_SUCCESS) return false;
    }
    if (generator_config_.enable_penalty || adm->has_rule) {  // the count map row and the rule record live in the request's batch slot
        adm->slot_index = batch_slots_mgr_.Alloc(1);
        if (adm->slot_index == INT64_MAX) {
            LOG(ERROR) << "alloc batch slot error, available [" << batch_slots_mgr_.GetAvailableBlockNum() << "]";
            return false;
        }
    }
    return true;
}

static std::string GuideExclusion(const Request& r);

// the admission predicate handed to the request scheduler (reference check_func, llm_generator.cc:590-617).
// true  -> the request leaves the queue (either admitted, or invalid and failed by StartRequest)
// false -> it stays at the head (stash) and admission stops for this step
bool LLMGenerator::AdmitRequest(const LlmRequest& req, Admission* adm, int32_t* cool_down, bool* is_prefix_cache_hit) {
    adm->ResetForRequest((int)req.orig->token_ids->size());
    // the prompt length counts against the step budget BEFORE the check and even for prefix-cache hits
    adm->total_tokens_per_step += adm->first_fill_len;
    if (adm->total_tokens_per_step > generator_config_.max_tokens_per_step) return false;
    if (adm->first_fill_len == 0) {  // deviation: an empty prompt would reserve zero KV slots and feed no token
        adm->errmsg = "id [" + std::to_string(req.orig->id) + "] empty prompt";
        adm->first_fill_len = -1;
        return true;
    }
    if (!ClampLengths(generator_config_, *req.orig, &adm->first_fill_len, &adm->rest_iters, &adm->errmsg)) {
        LOG(ERROR) << adm->errmsg;
        return true;
    }
    if (adm->rest_iters <= 0) {  // deviation: the reference reserves KV here and leaks it when StartRequest rejects
        adm->errmsg = "id [" + std::to_string(req.orig->id) + "] generation length <= 0";
        return true;
    }
    if (!req.orig->guide_regex.empty()) {
        adm->errmsg = GuideExclusion(*req.orig);
        if (!adm->errmsg.empty()) {
            adm->errmsg = "id [" + std::to_string(req.orig->id) + "] " + adm->errmsg;
            LOG(ERROR) << adm->errmsg;
            adm->first_fill_len = -1;
            return true;
        }
    }
    if (req.orig->HasLogitRule()) {  // validated once, here; an invalid rule fails its request alone (StartRequest)
        const Request& r = *req.orig;
        bool ok = llm_engine_.HasLogitRules();
        if (!ok) {
            adm->errmsg = "logit rules: the backend's post processor has no EditLogits";
            adm->errcode = RC_UNSUPPORTED;
        } else {
            std::vector<int> stops(generator_config_.stop_tokens.begin(), generator_config_.stop_tokens.end());
            if (r.stop_tokens) stops.insert(stops.end(), r.stop_tokens->begin(), r.stop_tokens->end());
            ok = BuildLogitRule(r.logit_bias, r.allowed_tokens.get(), r.banned_tokens, r.min_new_tokens, stops, model_config_.vocab_size,
                                &adm->rule, &adm->errmsg);
        }
        if (!ok) {
            adm->errmsg = "id [" + std::to_string(r.id) + "] " + adm->errmsg;
            LOG(ERROR) << adm->errmsg;
            adm->first_fill_len = -1;
            return true;
        }
        adm->has_rule = true;
    }
    if (!req.orig->guide_regex.empty() && !AdmitGuide(*req.orig, adm)) {  // a refused guide fails its request alone (StartRequest)
        adm->errmsg = "id [" + std::to_string(req.orig->id) + "] " + adm->errmsg;
        LOG(ERROR) << adm->errmsg;
        adm->first_fill_len = -1;
        return true;
    }
    if (!ReserveKv(req, adm, cool_down, is_prefix_cache_hit)) {
        ReleaseGuide(adm->guide_slot);   // the request stays queued and asks again
        adm->guide_slot = -1;
        return false;
    }
    ++adm->running_batch;
    ++adm->prefill_batch;
    return true;
}

// ------------------------------------------------------------------------------------------------ guided decoding

// the end tokens of a request: allowed exactly where its pattern is matched in full
static std::vector<int32_t> GuideEndTokens(const Tokenizer* tokenizer, const GeneratorConfig& cfg, const Request& r) {
    std::vector<int32_t> ends(cfg.stop_tokens.begin(), cfg.stop_tokens.end());
    if (r.stop_tokens) ends.insert(ends.end(), r.stop_tokens->begin(), r.stop_tokens->end());
    if (tokenizer) ends.push_back(tokenizer->GetEosId());
    std::sort(ends.begin(), ends.end());
    ends.erase(std::unique(ends.begin(), ends.end()), ends.end());
    return ends;
}

// what a guided request may not carry: the exclusions keep "no token left alive" impossible by construction, as nothing else removes a
// token the automaton counts on.  Empty: the request is fine
static std::string GuideExclusion(const Request& r) {
    if (!r.early_stopping) return "guide_regex: needs early_stopping (the request ends on an end token)";
    if (r.allowed_tokens) return "guide_regex: cannot be combined with allowed_tokens";
    if (!r.banned_tokens.empty()) return "guide_regex: cannot be combined with banned_tokens";
    if (r.min_new_tokens > 0) return "guide_regex: cannot be combined with min_new_tokens";
    for (const auto& p : r.logit_bias)
        if (p.second == -INFINITY) return "guide_regex: cannot be combined with a -inf logit_bias";
    return "";
}

bool LLMGenerator::AdmitGuide(const Request& r, Admission* adm) {
    adm->errcode = RC_UNSUPPORTED;
    if (!llm_engine_.HasGuides()) { adm->errmsg = "guide_regex: the backend's post processor has no GuideEdit"; return false; }
    std::string bytes;
    if (!tokenizer_ || !tokenizer_->TokenBytes(0, &bytes)) {
        adm->errmsg = "guide_regex: needs a tokenizer that knows the bytes of its tokens (TokenBytes)";
        return false;
    }
    if (guide_vocab_ == 0) {  // the first guided request: the vocabulary goes to the backend, once
        const int32_t V = model_config_.vocab_size;
        std::string blob;
        std::vector<int64_t> offsets(1, 0);
        for (int32_t t = 0; t < V; ++t) {
            tokenizer_->TokenBytes(t, &bytes);
            blob += bytes;
            offsets.push_back((int64_t)blob.size());
        }
        const RetCode rc = llm_engine_.SetGuideVocab((const uint8_t*)blob.data(), offsets.data(), V);
        guide_vocab_ = rc == RC_SUCCESS ? 1 : -1;
        if (rc != RC_SUCCESS) LOG(ERROR) << "SetGuideVocab failed: " << GetRetCodeStr(rc);
    }
    if (guide_vocab_ < 0) {
        adm->errcode = RC_OTHER_ERROR;
        adm->errmsg = "guide_regex: the backend refused the vocabulary";
        return false;
    }
    adm->errcode = RC_INVALID_VALUE;
    const std::vector<int32_t> ends = GuideEndTokens(tokenizer_, generator_config_, r);
    if ((int32_t)ends.size() > PostProcessor::kLogitStopMax) {
        adm->errmsg = "guide_regex: more than " + std::to_string(PostProcessor::kLogitStopMax) + " end tokens";
        return false;
    }
    for (int32_t t : ends)
        if (t < 0 || t >= model_config_.vocab_size) {
            adm->errmsg = "guide_regex: end token [" + std::to_string(t) + "] outside the vocabulary";
            return false;
        }
    std::string key = r.guide_regex;
    key.push_back('\0');
    for (int32_t t : ends) key += std::to_string(t) + ",";
    GuideDfa dfa;
    bool cached = false;
    for (const GuideSlot& g : guides_) cached = cached || g.key == key;
    if (!cached && !CompileGuideRegex(r.guide_regex, &dfa, &adm->errmsg)) return false;
    adm->guide_slot = AcquireGuide(key, dfa, ends, &adm->errmsg, &adm->errcode);
    return adm->guide_slot >= 0;
}

int32_t LLMGenerator::AcquireGuide(const std::string& key, const GuideDfa& dfa, const std::vector<int32_t>& end_tokens, std::string* err,
                                   RetCode* errcode) {
    const int32_t n = PostProcessor::kGuideMaxSlots;
    int32_t pick = -1;
    for (int32_t i = 0; i < n; ++i)
        if (guides_[i].key == key) {
            ++guides_[i].refs;
            guides_[i].last_use = ++guide_clock_;
            return i;
        }
    for (int32_t i = 0; i < n && pick < 0; ++i)
        if (guides_[i].key.empty()) pick = i;
    if (pick < 0) {  // evict the idle slot that was used longest ago
        for (int32_t i = 0; i < n; ++i)
            if (guides_[i].refs == 0 && (pick < 0 || guides_[i].last_use < guides_[pick].last_use)) pick = i;
        if (pick < 0) {
            *errcode = RC_OTHER_ERROR;
            *err = "guide_regex: all " + std::to_string(n) + " guide slots are held by running requests";
            return -1;
        }
        const RetCode rc = llm_engine_.UnloadGuide(pick);
        if (rc != RC_SUCCESS) {
            *errcode = RC_OTHER_ERROR;
            *err = "guide_regex: UnloadGuide failed: " + std::string(GetRetCodeStr(rc));
            return -1;
        }
        guides_[pick] = GuideSlot();
    }
    const RetCode rc = llm_engine_.LoadGuide(pick, dfa, end_tokens);
    if (rc != RC_SUCCESS) {
        *errcode = rc == RC_INVALID_VALUE ? RC_INVALID_VALUE : RC_OTHER_ERROR;
        *err = rc == RC_INVALID_VALUE ? "guide_regex: some state of the pattern's automaton allows no token of the vocabulary"
                                      : "guide_regex: LoadGuide failed: " + std::string(GetRetCodeStr(rc));
        return -1;
    }
    guides_[pick].key = key;
    guides_[pick].dfa = dfa;
    guides_[pick].refs = 1;
    guides_[pick].last_use = ++guide_clock_;
    return pick;
}

void LLMGenerator::ReleaseGuide(int32_t slot) {
    if (slot < 0 || slot >= PostProcessor::kGuideMaxSlots) return;
    if (guides_[slot].refs > 0) --guides_[slot].refs;
}

// seed of a request that brings none: one step of the splitmix64 generator (Vigna) from state x
static uint64_t SplitMix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// reference ParseRequest, llm_generator.cc:193-261
bool LLMGenerator::StartRequest(const LlmRequest& req, const Admission& adm, ModelInput* in) {
    const Request& r = *req.orig;
    if (adm.rest_iters <= 0 || adm.first_fill_len == -1) {
        conn_->NotifyFailure(r.id, adm.errcode, adm.errmsg);
        if (adapters_) adapters_->Release(r.lora_slot);
        return true;
    }
    const int mode = model_config_.cache_mode;
    if ((mode == 0 && adm.cache_index == INT64_MAX) || (mode == 1 && adm.page_list.empty())) {
        LOG(ERROR) << "catch invalid cache_index or page list";
        if (adapters_) adapters_->Release(r.lora_slot);
        ReleaseGuide(adm.guide_slot);
        return false;
    }
    TidData& t = tid_data_map_.emplace(r.id, TidData()).first->second;
    t.tid = r.id;
    t.temperature = r.temperature;
    t.top_p = r.top_p;
    t.top_k = r.top_k;
    t.repetition_penalty = r.repetition_penalty;
    t.presence_penalty = r.presence_penalty;
    t.frequency_penalty = r.frequency_penalty;
    t.early_stopping = r.early_stopping;
    t.rest_iters = adm.rest_iters;
    t.total_len = adm.first_fill_len + adm.rest_iters;
    t.stop_tokens = r.stop_tokens;
    t.is_token_in_out = r.is_token_in_out;
    t.slot_index = adm.slot_index;
    t.lora_slot = r.lora_slot;
    t.seed = r.seed ? r.seed : SplitMix64(generator_config_.sampling_seed + ++unseeded_requests_);
    t.num_logprobs = std::min(std::max(r.num_logprobs, 0), PostProcessor::kTopLogprobsMax);
    t.prompt_logprobs = std::min(std::max(r.prompt_logprobs, -1), PostProcessor::kTopLogprobsMax);
    // the logit rule goes up once, now that the request has its slot and before its first step.  A slot's record is never cleared: it is
    // read only while its owner's flags are set, and the next owner with a rule overwrites it
    uint32_t logit_flags = 0;
    if (adm.has_rule) {
        t.min_new_tokens = r.min_new_tokens;
        const RetCode rule_rc = llm_engine_.SetLogitRule(t.slot_index, adm.rule);
        if (rule_rc != RC_SUCCESS) {
            LOG(ERROR) << "id [" << r.id << "] SetLogitRule failed: " << GetRetCodeStr(rule_rc);
            t.rule_failed = true;
        } else {
            if (!adm.rule.bias_tokens.empty() || adm.rule.has_mask) logit_flags |= 1u;
            if (!adm.rule.stop_tokens.empty()) logit_flags |= 2u;
        }
    }
    if (adm.guide_slot >= 0) {
        t.guide_slot = adm.guide_slot;
        t.guide_state = 0;
        // drawing an end token ends the request: the tokenizer's EOS counts as one of its stop tokens
        auto stops = std::make_shared<std::unordered_set<int>>();
        if (r.stop_tokens) *stops = *r.stop_tokens;
        stops->insert(tokenizer_->GetEosId());
        t.stop_tokens = stops;
    }
    if (mode == 0) {
        t.cache_index = (uint64_t)adm.cache_index;
    } else {
        t.page_list = adm.page_list;
        t.hash_list = adm.hash_list;
        t.cache_hit_count = adm.cache_hit_count;
    }
    // where the prefill starts: no hit -> 0; whole prompt cached -> recompute only its last token; else -> the hit
    const int64_t hit = adm.cache_hit_count;
    if (hit == 0) {
        t.next_tokens = r.token_ids;
        t.start_pos = 0;
    } else if ((size_t)hit == r.token_ids->size()) {
        t.next_tokens = std::make_shared<std::vector<int>>(1, r.token_ids->back());
        t.start_pos = hit - 1;
    } else {
        t.next_tokens = std::make_shared<std::vector<int>>(r.token_ids->begin() + hit, r.token_ids->end());
        t.start_pos = hit;
    }
    tid_list_.push_back(&t);
    in->start_pos.push_back(t.start_pos);
    in->temperatures.push_back(t.temperature);
    in->top_p_list.push_back(t.top_p);
    in->top_k_list.push_back(t.top_k);
    in->seed_list.push_back(t.seed);
    in->draw_list.push_back(0);
    in->repetition_penalty_list.push_back(t.repetition_penalty);
    in->presence_penalty_list.push_back(t.presence_penalty);
    in->frequency_penalty_list.push_back(t.frequency_penalty);
    in->batch_slots.push_back(t.slot_index);
    in->lora_slots.push_back(t.lora_slot);
    in->num_logprobs_list.push_back(t.num_logprobs);
    in->prompt_logprobs_list.push_back(t.prompt_logprobs);
    in->logit_flags.push_back(logit_flags);
    in->guide_slots.push_back(t.guide_slot);
    in->guide_states.push_back(t.guide_state);
    if (mode == 0) in->cache_indices.push_back(adm.cache_index);
    else in->max_pages = std::max<int64_t>((int64_t)t.page_list.size(), in->max_pages);
    return true;
}

// ------------------------------------------------------------------------------------------------ packing

// reference UpdateInput, llm_generator.cc:263-298
void LLMGenerator::PackStep(bool req_list_changed, ModelInput* in) const {
    const size_t n = tid_list_.size();
    in->max_seq_len = 0;
    in->max_kv_len = 0;
    in->token_inputs.clear();
    in->seq_starts.assign(1, 0);
    in->kv_starts.assign(1, 0);
    in->seq_starts.reserve(n + 1);
    in->kv_starts.reserve(n + 1);
    const bool repack_pages = req_list_changed && model_config_.cache_mode == 1;
    if (repack_pages) in->page_list.assign(n * in->max_pages, INT64_MAX);
    for (size_t i = 0; i < n; ++i) {
        const TidData* t = tid_list_[i];
        const int64_t seqlen = (int64_t)t->next_tokens->size();
        in->token_inputs.insert(in->token_inputs.end(), t->next_tokens->begin(), t->next_tokens->end());
        in->seq_starts.push_back(in->seq_starts[i] + seqlen);
        in->kv_starts.push_back(in->kv_starts[i] + t->start_pos + seqlen);
        in->max_seq_len = std::max(in->max_seq_len, seqlen);
        in->max_kv_len = std::max(in->max_kv_len, t->start_pos + seqlen);
        if (repack_pages) std::copy(t->page_list.begin(), t->page_list.end(), in->page_list.begin() + i * in->max_pages);
    }
}

// reference RemoveFinishedTask, llm_generator.cc:300-340: stable compaction of every per-row vector
void LLMGenerator::CompactBatch(ModelInput* in) {
    const int mode = model_config_.cache_mode;
    size_t keep = 0;
    if (mode == 1) in->max_pages = 0;
    for (size_t i = 0; i < tid_list_.size(); ++i) {
        if (!tid_list_[i]) continue;
        tid_list_[keep] = tid_list_[i];
        if (mode == 0) in->cache_indices[keep] = in->cache_indices[i];
        else in->max_pages = std::max<int64_t>(in->max_pages, (int64_t)tid_list_[i]->page_list.size());
        in->start_pos[keep] = in->start_pos[i];
        in->temperatures[keep] = in->temperatures[i];
        in->top_p_list[keep] = in->top_p_list[i];
        in->top_k_list[keep] = in->top_k_list[i];
        in->seed_list[keep] = in->seed_list[i];
        in->draw_list[keep] = in->draw_list[i];
        in->repetition_penalty_list[keep] = in->repetition_penalty_list[i];
        in->presence_penalty_list[keep] = in->presence_penalty_list[i];
        in->frequency_penalty_list[keep] = in->frequency_penalty_list[i];
        in->batch_slots[keep] = in->batch_slots[i];
        in->lora_slots[keep] = in->lora_slots[i];
        in->num_logprobs_list[keep] = in->num_logprobs_list[i];
        in->prompt_logprobs_list[keep] = in->prompt_logprobs_list[i];
        in->logit_flags[keep] = in->logit_flags[i];
        in->guide_slots[keep] = in->guide_slots[i];
        in->guide_states[keep] = in->guide_states[i];
        ++keep;
    }
    tid_list_.resize(keep);
    if (mode == 0) in->cache_indices.resize(keep);
    in->start_pos.resize(keep);
    in->temperatures.resize(keep);
    in->top_p_list.resize(keep);
    in->top_k_list.resize(keep);
    in->seed_list.resize(keep);
    in->draw_list.resize(keep);
    in->repetition_penalty_list.resize(keep);
    in->presence_penalty_list.resize(keep);
    in->frequency_penalty_list.resize(keep);
    in->batch_slots.resize(keep);
    in->lora_slots.resize(keep);
    in->num_logprobs_list.resize(keep);
    in->prompt_logprobs_list.resize(keep);
    in->logit_flags.resize(keep);
    in->guide_slots.resize(keep);
    in->guide_states.resize(keep);
    LOG(DEBUG) << "Rest tasks: " << keep;
}

// reference DeleteTasks, llm_generator.cc:387-439
void LLMGenerator::DeleteTasks(ModelInput* in) {
    FinishedTaskInfo info;
    while (finished_tasks_.Pop(&info)) {
        auto it = tid_data_map_.find(info.id);
        if (it == tid_data_map_.end()) continue;  // finished by the worker and cancelled by the connection at once
        TidData& t = it->second;
        --in->decoding_batches;
        size_t row = 0;
        while (row < tid_list_.size() && !(tid_list_[row] && tid_list_[row]->tid == info.id)) ++row;
        if (row == tid_list_.size()) continue;
        tid_list_[row] = nullptr;
        // the batch rows shift: the device page table, the penalty slots and the sampler's per-row parameters must be
        // re-uploaded by the next Execute even when nothing finished in the worker and nothing new was admitted (a
        // cancel from the connection on an otherwise quiet step; the reference leaves the flag untouched here)
        req_list_changed_ = true;
        if (model_config_.cache_mode == 0) {
            idx_mgr_.Free(t.cache_index, (uint64_t)t.total_len - 1);
        } else if (generator_config_.enable_prefix_cache) {
            // hashed prompt pages go back to the prefix cache (LRU once unreferenced); the rest to the page pool
            const int64_t hashed = (int64_t)t.hash_list.size();
            prefix_cache_mgr_.DecRefCount(t.hash_list.data(), hashed);
            page_mgr_.Free(t.page_list.data() + hashed, (int64_t)t.page_list.size() - hashed);
        } else {
            page_mgr_.Free(t.page_list.data(), (int64_t)t.page_list.size());
        }
        if (t.slot_index != INT64_MAX) batch_slots_mgr_.Free((uint64_t)t.slot_index, 1);
        if (adapters_) adapters_->Release(t.lora_slot);
        ReleaseGuide(t.guide_slot);
        // (the reference adds to a by-value pointer here and so counts nothing -- SURVEY.md Q2; counted properly)
        worker_profiler_->req_counter.output_tokens_per_req += (uint64_t)t.gen_tokens_cnt;
        tid_data_map_.erase(it);
        ++worker_profiler_->finished_task_cnt;
    }
    CompactBatch(in);
}

// reference ReleaseResource, llm_generator.cc:368-385 (after a failed Execute)
void LLMGenerator::ReleaseResource() {
    for (TidData* t : tid_list_) {
        if (model_config_.cache_mode == 0) idx_mgr_.Free(t->cache_index, (uint64_t)t->total_len - 1);
        else page_mgr_.Free(t->page_list.data(), (int64_t)t->page_list.size());
        if (t->slot_index != INT64_MAX) batch_slots_mgr_.Free((uint64_t)t->slot_index, 1);
        if (adapters_) adapters_->Release(t->lora_slot);
        ReleaseGuide(t->guide_slot);
    }
    prefix_cache_mgr_.Reset();
    tid_list_.clear();
    tid_data_map_.clear();
    req_list_changed_ = true;
    FinishedTaskInfo info;
    while (finished_tasks_.Pop(&info)) {}
}

// reference DecodeAndSendTask, llm_generator.cc:58-112: one Response per request per step; text requests buffer up
// to three tokens while the piece decodes to U+FFFD
void LLMGenerator::SendTokens(const std::vector<TidGenToken>& tokens) {
    static const char kReplacement[] = "\xef\xbf\xbd";
    std::vector<Response> rsp(tokens.size());
    for (size_t i = 0; i < tokens.size(); ++i) {
        const TidGenToken& g = tokens[i];
        Response& r = rsp[i];
        r.id = g.tid;
        r.token = g.token;
        r.finish_flag = g.finish_flag;
        r.logprob = g.logprob;
        r.is_special = g.is_special;
        r.top_tokens = g.top_tokens;
        r.top_logprobs = g.top_logprobs;
        r.prompt_logprobs = g.prompt_logprobs;
        r.prompt_ranks = g.prompt_ranks;
        r.prompt_top_tokens = g.prompt_top_tokens;
        r.prompt_top_logprobs = g.prompt_top_logprobs;
        if (!g.is_token_in_out && tokenizer_) {
            int tok = g.token;
            tokenizer_->Decode(&tok, 1, &r.generated);
            if (r.generated == kReplacement) {
                std::vector<int>& buf = decode_buffer_[g.tid];
                buf.push_back(g.token);
                r.generated.clear();
                if (buf.size() == 3) {
                    tokenizer_->Decode(buf.data(), 3, &r.generated);
                    buf.clear();
                }
            }
            if (g.finish_flag != FinishFlag::NOT_FINISHED) decode_buffer_.erase(g.tid);
        }
    }
    conn_->Send(rsp);
}

// ------------------------------------------------------------------------------------------------ the step loop

// reference Generate, llm_generator.cc:574-786
void LLMGenerator::Generate() {
    ModelInput in;
    ModelOutput out;
    Admission adm;
    int running_batch = 0, prefill_batch = 0;
    int32_t cool_down = 0;
    uint64_t loop_step = 0;
    bool is_prefix_cache_hit = false;
    std::string error_msg;
    auto& counters = worker_profiler_->step_counter;

    tid_list_.clear();
    tid_data_map_.clear();
    req_list_changed_ = true;
    { FinishedTaskInfo drop; while (finished_tasks_.Pop(&drop)) {} }

    const std::function<bool(const LlmRequest&)> admit = [&](const LlmRequest& req) {
        return AdmitRequest(req, &adm, &cool_down, &is_prefix_cache_hit);
    };

    while (true) {
        is_prefix_cache_hit = false;
        const auto step_begin = std::chrono::high_resolution_clock::now();
        adm.total_tokens_per_step = running_batch;  // every running request contributes one decode token
        adm.running_batch = running_batch;
        adm.prefill_batch = 0;
        {
            utils::TimingGuard timing(&counters.current.prepare_cost);
            while (adm.running_batch < generator_config_.max_running_batch &&
                   adm.prefill_batch < generator_config_.max_prefill_batch && cool_down <= 0) {
                std::unique_ptr<LlmRequest> req(sched_.TryPopRequest(admit));
                if (!req) break;
                ++worker_profiler_->req_counter.waiting_cnt;
                worker_profiler_->req_counter.waiting_cost += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                    std::chrono::high_resolution_clock::now() - req->enqueue_ts).count();
                if (!StartRequest(*req, adm, &in)) break;
                req_list_changed_ = true;
            }
            running_batch = (int)tid_list_.size();
            if (running_batch == 0) break;
            PackStep(req_list_changed_, &in);
            worker_profiler_->max_running_task = std::max<uint64_t>(running_batch, worker_profiler_->max_running_task);
            prefill_batch = adm.prefill_batch;
        }
        counters.global.prepare_cost += counters.current.prepare_cost;

        if (observer_) observer_(observer_arg_, loop_step, in, req_list_changed_, is_prefix_cache_hit);
        out.Clear();
        out.Resize(running_batch);
        error_msg.clear();
        const RetCode rc = llm_engine_.Execute(in, req_list_changed_, is_prefix_cache_hit, &out, &error_msg);
        if (rc != RC_SUCCESS) {
            LOG(ERROR) << "llm engine excute failed";
            for (TidData* t : tid_list_) conn_->NotifyFailure(t->tid, rc, error_msg);
            ReleaseResource();
            break;
        }
        req_list_changed_ = false;

        {
            utils::TimingGuard timing(&counters.current.post_process_cost);
            decoder_thread_pool_.Wait();  // the previous step's responses are out
            auto tokens = std::make_shared<std::vector<TidGenToken>>();
            tokens->reserve(running_batch);
            int32_t top_row = 0;  // the place of the next asking row in the compact top-N results
            size_t prompt_pos = 0;  // the place of the next asking request's first position in the step's prompt logprobs
            for (int row = 0; row < running_batch; ++row) {
                TidData* t = tid_list_[row];
                ++t->gen_tokens_cnt;
                ++in.draw_list[row];
                if (t->gen_tokens_cnt >= t->min_new_tokens) in.logit_flags[row] &= ~2u;  // the stops are free from the next step on
                const int tok = out.output_token[row];
                const int64_t fed = (int64_t)t->next_tokens->size();
                t->next_tokens = std::make_shared<std::vector<int>>(1, tok);
                if (t->steps == 0) {  // prefill row becomes a decode row
                    in.start_pos[row] += fed;
                    ++in.decoding_batches;
                } else {
                    ++in.start_pos[row];
                }
                t->start_pos += fed;
                ++t->steps;
                --t->rest_iters;
                FinishFlag flag = FinishFlag::NOT_FINISHED;
                const bool hit_stop = t->early_stopping &&
                    (generator_config_.stop_tokens.count(tok) || (t->stop_tokens && t->stop_tokens->count(tok)));
                // a request that asks for top-N logprobs on a backend without them fails alone: it leaves like a finished one, unanswered
                // the prompt logprobs of a request arrive with its first token: its fed - 1 positions are the next ones of the step's results
                const bool scores_prompt = in.prompt_logprobs_list[row] >= 0;
                const size_t prompt_n = scores_prompt && !out.prompt_unsupported ? (size_t)(fed - 1) : 0;
                in.prompt_logprobs_list[row] = -1;   // asked once: later steps carry nothing
                const bool no_prompt = scores_prompt && out.prompt_unsupported;
                // a guided request walks its automaton over the bytes of every token that does not end it.  The mask allowed only tokens
                // that keep the automaton alive, so the dead state here means kernel and host disagree: that request fails, alone
                bool guide_broken = false;
                if (t->guide_slot >= 0 && hit_stop) {
                    guide_broken = !guides_[t->guide_slot].dfa.Accepting(t->guide_state);   // an end token in front of a full match
                } else if (t->guide_slot >= 0) {
                    std::string bytes;
                    tokenizer_->TokenBytes(tok, &bytes);
                    const int32_t to = bytes.empty() ? GuideDfa::kDead : guides_[t->guide_slot].dfa.Step(t->guide_state, bytes);
                    if (to == GuideDfa::kDead) guide_broken = true;
                    else in.guide_states[row] = t->guide_state = to;
                }
                const bool no_top = (t->num_logprobs > 0 && out.top_unsupported) || t->rule_failed || no_prompt || guide_broken;
                if (t->rest_iters <= 0 || hit_stop || no_top) {
                    flag = t->rest_iters <= 0 ? FinishFlag::LENGTH : FinishFlag::EOS_TOKEN;
                    if (cool_down > 0) --cool_down;
                    finished_tasks_.Push(FinishedTaskInfo(t->tid, FinishedTaskInfo::FROM_WORKER));
                    req_list_changed_ = true;
                }
                if (no_top) {
                    // the step's results hold this row's entries all the same: both cursors pass them, or the rows behind read them
                    prompt_pos += prompt_n;
                    if (t->num_logprobs > 0 && top_row < out.top_rows) ++top_row;
                    if (guide_broken) conn_->NotifyFailure(t->tid, RC_OTHER_ERROR, "guide_regex: internal error: token [" + std::to_string(tok) + "] is not allowed in state [" + std::to_string(t->guide_state) + "] of the request's guide");
                    else if (t->rule_failed) conn_->NotifyFailure(t->tid, RC_OTHER_ERROR, "logit rules: the backend could not take the request's rule");
                    else if (no_prompt) conn_->NotifyFailure(t->tid, RC_UNSUPPORTED, "prompt_logprobs: the backend's runtime has no SetPromptLogprobs");
                    else conn_->NotifyFailure(t->tid, RC_UNSUPPORTED, "num_logprobs: the backend's post processor has no TopLogprobs");
                    continue;
                }
                tokens->push_back(TidGenToken{t->tid, tok, out.logprobs[row], flag, (uint64_t)t->steps, t->is_token_in_out,
                                              generator_config_.special_tokens.count(tok) > 0, {}, {}, {}, {}, {}, {}});
                if (prompt_n > 0 && prompt_pos + prompt_n <= out.prompt_logprobs.size()) {
                    TidGenToken& g = tokens->back();
                    const size_t n = (size_t)t->prompt_logprobs, W = (size_t)PostProcessor::kTopLogprobsMax;
                    g.prompt_logprobs.assign(out.prompt_logprobs.begin() + prompt_pos, out.prompt_logprobs.begin() + prompt_pos + prompt_n);
                    g.prompt_ranks.assign(out.prompt_ranks.begin() + prompt_pos, out.prompt_ranks.begin() + prompt_pos + prompt_n);
                    for (size_t i = prompt_pos; n > 0 && i < prompt_pos + prompt_n; ++i) {
                        g.prompt_top_tokens.insert(g.prompt_top_tokens.end(), out.prompt_top_tokens.begin() + i * W, out.prompt_top_tokens.begin() + i * W + n);
                        g.prompt_top_logprobs.insert(g.prompt_top_logprobs.end(), out.prompt_top_logprobs.begin() + i * W, out.prompt_top_logprobs.begin() + i * W + n);
                    }
                }
                prompt_pos += prompt_n;
                if (t->num_logprobs > 0 && top_row < out.top_rows) {
                    // the row's first n slots; the ones behind the vocabulary (token -1) are padding
                    const int32_t* tt = out.top_tokens.data() + (size_t)top_row * PostProcessor::kTopLogprobsMax;
                    const float* tl = out.top_logprobs.data() + (size_t)top_row * PostProcessor::kTopLogprobsMax;
                    int32_t n = 0;
                    while (n < t->num_logprobs && tt[n] >= 0) ++n;
                    tokens->back().top_tokens.assign(tt, tt + n);
                    tokens->back().top_logprobs.assign(tl, tl + n);
                    ++top_row;
                }
            }
            // detokenise + send overlaps the next step (llm_generator.cc:738-745)
            decoder_thread_pool_.RunAsync([this, tokens](uint32_t, uint32_t) { SendTokens(*tokens); });
            if (finished_tasks_.Size() > 0) DeleteTasks(&in);
        }
        counters.global.post_process_cost += counters.current.post_process_cost;

        counters.current.total_cost = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
            std::chrono::high_resolution_clock::now() - step_begin).count();
        counters.global.total_cost += counters.current.total_cost;
        worker_profiler_->pending_task_size = sched_.GetPendingSize();
        ++counters.global.step_cnt;
        ++loop_step;
        if (generator_config_.enable_profiling && (loop_step == 1 || loop_step % 100 == 0 || tid_list_.empty())) {
            worker_profiler_->running_task = running_batch;
            worker_profiler_->prefill_batch = prefill_batch;
            worker_profiler_->prefill_tokens = in.token_inputs.size() - (running_batch - prefill_batch);
            worker_profiler_->kv_max_blk = kv_cache_max_tokens_;
            worker_profiler_->kv_rest_blk = model_config_.cache_mode == 0
                ? (uint64_t)idx_mgr_.GetAvailableBlockNum()
                : (uint64_t)(page_mgr_.GetAvail() * model_config_.page_size);
            conn_->OnProfiling(worker_profiler_);
        }
    }
    decoder_thread_pool_.Wait();
}

}}  // namespace ppl::llm
