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
    bool rejected = false;  // the request is invalid: it leaves the queue and StartRequest fails it with errcode / errmsg
    std::string errmsg;
    RetCode errcode = RC_INVALID_VALUE;
    bool has_rule = false;  // the request carries a logit rule: `rule` is its validated, merged form
    LogitRule rule;
    int32_t guide_slot = -1;  // the request is guided: the slot it holds a reference on

    // an invalid request: true for the scheduler, so that it leaves the queue; `msg` may be errmsg itself
    bool Reject(const std::string& msg, RetCode code = RC_INVALID_VALUE) {
        rejected = true;
        errmsg = msg;
        errcode = code;
        LOG(ERROR) << errmsg;
        return true;
    }
    bool Reject(uint64_t id, const std::string& msg, RetCode code = RC_INVALID_VALUE) {
        return Reject("id [" + std::to_string(id) + "] " + msg, code);
    }

    void ResetForRequest(int prompt_len) {
        rejected = false;
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
                  generator_config.per_request_sampling)
    , guide_cache_(&llm_engine_, resource.tokenizer, model_config.vocab_size) {
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
// false: the request cannot run, *errmsg says why
static bool ClampLengths(const GeneratorConfig& cfg, const Request& r, int first_fill_len, int* rest_iters, std::string* errmsg) {
    const std::string idstr = "id [" + std::to_string(r.id) + "]";
    if (first_fill_len > cfg.max_input_tokens_per_request) {
        *errmsg = idstr + " invalid input token len: " + std::to_string(first_fill_len) +
                  ", server allowed max input len: " + std::to_string(cfg.max_input_tokens_per_request);
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
    if (first_fill_len + r.generation_length > cfg.max_total_tokens_per_request) {
        const int clamped = cfg.max_total_tokens_per_request - first_fill_len;
        const std::string msg = idstr + ": total len in request is [" + std::to_string(first_fill_len + r.generation_length) +
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

// the end tokens of a guided request: allowed exactly where its pattern is matched in full
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
    if (!r.guide_regex.empty() && !r.guide_json_schema.empty()) return "guide_json_schema: cannot be combined with guide_regex";
    const std::string field = r.guide_regex.empty() ? "guide_json_schema" : "guide_regex";
    if (!r.early_stopping) return field + ": needs early_stopping (the request ends on an end token)";
    if (r.allowed_tokens) return field + ": cannot be combined with allowed_tokens";
    if (!r.banned_tokens.empty()) return field + ": cannot be combined with banned_tokens";
    if (r.min_new_tokens > 0) return field + ": cannot be combined with min_new_tokens";
    for (const auto& p : r.logit_bias)
        if (p.second == -INFINITY) return field + ": cannot be combined with a -inf logit_bias";
    return "";
}

// the admission predicate handed to the request scheduler (reference check_func, llm_generator.cc:590-617).
// true  -> the request leaves the queue (either admitted, or invalid and failed by StartRequest)
// false -> it stays at the head (stash) and admission stops for this step
bool LLMGenerator::AdmitRequest(const LlmRequest& req, Admission* adm, int32_t* cool_down, bool* is_prefix_cache_hit) {
    adm->ResetForRequest((int)req.orig->token_ids->size());
    // the prompt length counts against the step budget BEFORE the check and even for prefix-cache hits
    adm->total_tokens_per_step += adm->first_fill_len;
    if (adm->total_tokens_per_step > generator_config_.max_tokens_per_step) return false;
    const Request& r = *req.orig;
    if (adm->first_fill_len == 0) return adm->Reject(r.id, "empty prompt");  // deviation: it would reserve zero KV slots and feed no token
    if (!ClampLengths(generator_config_, r, adm->first_fill_len, &adm->rest_iters, &adm->errmsg)) return adm->Reject(adm->errmsg);
    // deviation: the reference reserves KV here and leaks it when StartRequest rejects
    if (adm->rest_iters <= 0) return adm->Reject(r.id, "generation length <= 0");
    const bool guided = !r.guide_regex.empty() || !r.guide_json_schema.empty();
    const std::string excluded = guided ? GuideExclusion(r) : "";
    if (!excluded.empty()) return adm->Reject(r.id, excluded);
    if (r.AsksTruncation()) {  // min_p / typical_p: a request that cannot be served as it asks fails alone (StartRequest)
        if (!generator_config_.per_request_sampling)
            return adm->Reject(r.id, "min_p / typical_p: need per_request_sampling", RC_UNSUPPORTED);
        if (!llm_engine_.HasSampleRowsTrunc())
            return adm->Reject(r.id, "min_p / typical_p: the backend's post processor has no SampleRowsTrunc", RC_UNSUPPORTED);
    }
    if (r.HasLogitRule()) {  // validated once, here; an invalid rule fails its request alone (StartRequest)
        if (!llm_engine_.HasLogitRules())
            return adm->Reject(r.id, "logit rules: the backend's post processor has no EditLogits", RC_UNSUPPORTED);
        std::vector<int> stops(generator_config_.stop_tokens.begin(), generator_config_.stop_tokens.end());
        if (r.stop_tokens) stops.insert(stops.end(), r.stop_tokens->begin(), r.stop_tokens->end());
        if (!BuildLogitRule(r.logit_bias, r.allowed_tokens.get(), r.banned_tokens, r.min_new_tokens, stops, model_config_.vocab_size,
                            &adm->rule, &adm->errmsg))
            return adm->Reject(r.id, adm->errmsg);
        adm->has_rule = true;
    }
    if (guided) {  // a refused guide fails its request alone (StartRequest)
        const bool schema = r.guide_regex.empty();
        adm->guide_slot = guide_cache_.Acquire(schema ? GuideCache::Kind::kJsonSchema : GuideCache::Kind::kRegex,
                                               schema ? r.guide_json_schema : r.guide_regex,
                                               GuideEndTokens(tokenizer_, generator_config_, r), &adm->errmsg, &adm->errcode);
        if (adm->guide_slot < 0) return adm->Reject(r.id, adm->errmsg, adm->errcode);
    }
    if (!ReserveKv(req, adm, cool_down, is_prefix_cache_hit)) {
        guide_cache_.Release(adm->guide_slot);   // the request stays queued and asks again
        adm->guide_slot = -1;
        return false;
    }
    ++adm->running_batch;
    ++adm->prefill_batch;
    return true;
}

// seed of a request that brings none: one step of the splitmix64 generator (Vigna) from state x
static uint64_t SplitMix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// reference ParseRequest, llm_generator.cc:193-261
bool LLMGenerator::StartRequest(const LlmRequest& req, const Admission& adm) {
    const Request& r = *req.orig;
    if (adm.rejected) {
        conn_->NotifyFailure(r.id, adm.errcode, adm.errmsg);
        if (adapters_) adapters_->Release(r.lora_slot);
        return true;
    }
    const int mode = model_config_.cache_mode;
    if ((mode == 0 && adm.cache_index == INT64_MAX) || (mode == 1 && adm.page_list.empty())) {
        LOG(ERROR) << "catch invalid cache_index or page list";
        if (adapters_) adapters_->Release(r.lora_slot);
        guide_cache_.Release(adm.guide_slot);
        return false;
    }
    TidData& t = tid_data_map_.emplace(r.id, TidData()).first->second;
    t.tid = r.id;
    t.temperature = r.temperature;
    t.top_p = r.top_p;
    t.top_k = r.top_k;
    t.min_p = r.min_p;
    t.typical_p = r.typical_p;
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
    if (adm.has_rule) {
        t.min_new_tokens = r.min_new_tokens;
        const RetCode rule_rc = llm_engine_.SetLogitRule(t.slot_index, adm.rule);
        if (rule_rc != RC_SUCCESS) {
            LOG(ERROR) << "id [" << r.id << "] SetLogitRule failed: " << GetRetCodeStr(rule_rc);
            t.rule_failed = true;
        } else {
            if (!adm.rule.bias_tokens.empty() || adm.rule.has_mask) t.logit_flags |= 1u;
            if (!adm.rule.stop_tokens.empty()) t.logit_flags |= 2u;
        }
    }
    if (adm.guide_slot >= 0) {
        t.guide_slot = adm.guide_slot;
        t.guide_state = 0;
        t.guide_schema = r.guide_regex.empty();
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
    tid_list_.push_back(&t);  // its row of the step's lists: PackStep
    return true;
}

// ------------------------------------------------------------------------------------------------ packing

// reference UpdateInput, llm_generator.cc:263-298.  The one place that writes a per-row list of ModelInput: every list is rebuilt from the
// requests' records on every step, so a row carries its own request's values whatever joined or left in front of it.  Only the page
// table and its width wait for a change of the row set
void LLMGenerator::PackStep(bool req_list_changed, ModelInput* in) const {
    const size_t n = tid_list_.size();
    in->decoding_batches = 0;
    in->max_seq_len = 0;
    in->max_kv_len = 0;
    in->token_inputs.clear();
    in->seq_starts.assign(1, 0);
    in->kv_starts.assign(1, 0);
    in->seq_starts.reserve(n + 1);
    in->kv_starts.reserve(n + 1);
    in->start_pos.clear(); in->cache_indices.clear(); in->batch_slots.clear(); in->lora_slots.clear();
    in->temperatures.clear(); in->top_p_list.clear(); in->min_p_list.clear(); in->typical_p_list.clear(); in->top_k_list.clear(); in->seed_list.clear(); in->draw_list.clear();
    in->repetition_penalty_list.clear(); in->presence_penalty_list.clear(); in->frequency_penalty_list.clear();
    in->num_logprobs_list.clear(); in->prompt_logprobs_list.clear(); in->logit_flags.clear();
    in->guide_slots.clear(); in->guide_states.clear();
    const bool repack_pages = req_list_changed && model_config_.cache_mode == 1;
    if (repack_pages) {
        in->max_pages = 0;
        for (const TidData* t : tid_list_) in->max_pages = std::max<int64_t>(in->max_pages, (int64_t)t->page_list.size());
        in->page_list.assign(n * in->max_pages, INT64_MAX);
    }
    for (size_t i = 0; i < n; ++i) {
        const TidData* t = tid_list_[i];
        const int64_t seqlen = (int64_t)t->next_tokens->size();
        in->token_inputs.insert(in->token_inputs.end(), t->next_tokens->begin(), t->next_tokens->end());
        in->seq_starts.push_back(in->seq_starts[i] + seqlen);
        in->kv_starts.push_back(in->kv_starts[i] + t->start_pos + seqlen);
        in->max_seq_len = std::max(in->max_seq_len, seqlen);
        in->max_kv_len = std::max(in->max_kv_len, t->start_pos + seqlen);
        if (repack_pages) std::copy(t->page_list.begin(), t->page_list.end(), in->page_list.begin() + i * in->max_pages);
        if (t->steps > 0) ++in->decoding_batches;  // the decode rows are the first ones: a request joins at the end of the batch
        in->start_pos.push_back(t->start_pos);
        if (model_config_.cache_mode == 0) in->cache_indices.push_back((int64_t)t->cache_index);
        in->batch_slots.push_back(t->slot_index);
        in->lora_slots.push_back(t->lora_slot);
        in->temperatures.push_back(t->temperature);
        in->top_p_list.push_back(t->top_p);
        in->min_p_list.push_back(t->min_p);
        in->typical_p_list.push_back(t->typical_p);
        in->top_k_list.push_back(t->top_k);
        in->seed_list.push_back(t->seed);
        in->draw_list.push_back((uint64_t)t->gen_tokens_cnt);
        in->repetition_penalty_list.push_back(t->repetition_penalty);
        in->presence_penalty_list.push_back(t->presence_penalty);
        in->frequency_penalty_list.push_back(t->frequency_penalty);
        in->num_logprobs_list.push_back(t->num_logprobs);
        in->prompt_logprobs_list.push_back(t->steps == 0 ? t->prompt_logprobs : -1);  // asked once: later steps carry nothing
        in->logit_flags.push_back(t->logit_flags);
        in->guide_slots.push_back(t->guide_slot);
        in->guide_states.push_back(t->guide_state);
    }
}

// reference RemoveFinishedTask, llm_generator.cc:300-340: the rows that left are taken out, the others keep their order
void LLMGenerator::CompactBatch() {
    tid_list_.erase(std::remove(tid_list_.begin(), tid_list_.end(), nullptr), tid_list_.end());
    LOG(DEBUG) << "Rest tasks: " << tid_list_.size();
}

// a leaving request gives back its KV, its batch slot and its references on an adapter and a guide.  keep_cached_pages: its hashed prompt
// pages go back to the prefix cache (LRU once unreferenced) and only the rest to the page pool
void LLMGenerator::ReleaseRequest(const TidData& t, bool keep_cached_pages) {
    if (model_config_.cache_mode == 0) {
        idx_mgr_.Free(t.cache_index, (uint64_t)t.total_len - 1);
    } else {
        const int64_t hashed = keep_cached_pages ? (int64_t)t.hash_list.size() : 0;
        prefix_cache_mgr_.DecRefCount(t.hash_list.data(), hashed);
        page_mgr_.Free(t.page_list.data() + hashed, (int64_t)t.page_list.size() - hashed);
    }
    if (t.slot_index != INT64_MAX) batch_slots_mgr_.Free((uint64_t)t.slot_index, 1);
    if (adapters_) adapters_->Release(t.lora_slot);
    guide_cache_.Release(t.guide_slot);
}

// reference DeleteTasks, llm_generator.cc:387-439
void LLMGenerator::DeleteTasks() {
    FinishedTaskInfo info;
    while (finished_tasks_.Pop(&info)) {
        auto it = tid_data_map_.find(info.id);
        if (it == tid_data_map_.end()) continue;  // finished by the worker and cancelled by the connection at once
        TidData& t = it->second;
        const auto row = std::find(tid_list_.begin(), tid_list_.end(), &t);
        if (row == tid_list_.end()) continue;
        *row = nullptr;
        // the batch rows shift: the device page table, the penalty slots and the sampler's per-row parameters must be
        // re-uploaded by the next Execute even when nothing finished in the worker and nothing new was admitted (a
        // cancel from the connection on an otherwise quiet step; the reference leaves the flag untouched here)
        req_list_changed_ = true;
        ReleaseRequest(t, true);  // (only a request admitted through the prefix cache has hashed pages)
        // (the reference adds to a by-value pointer here and so counts nothing -- SURVEY.md Q2; counted properly)
        worker_profiler_->req_counter.output_tokens_per_req += (uint64_t)t.gen_tokens_cnt;
        tid_data_map_.erase(it);
        ++worker_profiler_->finished_task_cnt;
    }
    CompactBatch();
}

// reference ReleaseResource, llm_generator.cc:368-385 (after a failed Execute): every page goes to the pool, and the prefix cache is dropped
void LLMGenerator::ReleaseResource() {
    for (const TidData* t : tid_list_) ReleaseRequest(*t, false);
    prefix_cache_mgr_.Reset();
    tid_list_.clear();
    tid_data_map_.clear();
    req_list_changed_ = true;
    FinishedTaskInfo info;
    while (finished_tasks_.Pop(&info)) {}
}

// reference DecodeAndSendTask, llm_generator.cc:58-112: one Response per request per step; text requests buffer up
// to three tokens while the piece decodes to U+FFFD
void LLMGenerator::SendTokens(std::vector<TidGenToken>* tokens) {
    static const char kReplacement[] = "\xef\xbf\xbd";
    std::vector<Response> rsp;
    rsp.reserve(tokens->size());
    for (TidGenToken& g : *tokens) {
        rsp.push_back(std::move(g.rsp));
        Response& r = rsp.back();
        if (!g.is_token_in_out && tokenizer_) {
            int tok = r.token;
            tokenizer_->Decode(&tok, 1, &r.generated);
            if (r.generated == kReplacement) {
                std::vector<int>& buf = decode_buffer_[r.id];
                buf.push_back(r.token);
                r.generated.clear();
                if (buf.size() == 3) {
                    tokenizer_->Decode(buf.data(), 3, &r.generated);
                    buf.clear();
                }
            }
            if (r.finish_flag != FinishFlag::NOT_FINISHED) decode_buffer_.erase(r.id);
        }
    }
    conn_->Send(rsp);
}

// ------------------------------------------------------------------------------------------------ one row of a finished step

// The step's two compact result lists (ModelOutput's top-N rows and prompt positions), read front to back.  A row takes its entries of
// both in one call, before anything decides whether it is answered: what a failing row would leave behind, the row behind it would read
class StepResults final {
public:
    struct Slice {
        size_t prompt_pos = 0, prompt_n = 0;  // the row's positions of the step's prompt logprobs; prompt_n == 0: none
        int32_t top_row = -1;                 // its row of the step's top-N results; -1: none
    };
    explicit StepResults(const ModelOutput& out) : out_(out) {}
    // prompt_n: the prompt positions the step scored for the row; asks_top: the row asked for top-N logprobs
    Slice Take(size_t prompt_n, bool asks_top) {
        Slice s;
        if (prompt_pos_ + prompt_n <= out_.prompt_logprobs.size()) {
            s.prompt_pos = prompt_pos_;
            s.prompt_n = prompt_n;
        }
        prompt_pos_ += prompt_n;
        if (asks_top && top_row_ < out_.top_rows) s.top_row = top_row_++;
        return s;
    }

private:
    const ModelOutput& out_;
    size_t prompt_pos_ = 0;
    int32_t top_row_ = 0;
};

// advance: the row has produced `tok`, which is its next input.  Returns the number of tokens the step fed it
static int64_t AdvanceRow(TidData* t, int tok) {
    const int64_t fed = (int64_t)t->next_tokens->size();
    t->next_tokens = std::make_shared<std::vector<int>>(1, tok);
    t->start_pos += fed;
    ++t->gen_tokens_cnt;
    ++t->steps;  // a prefill row has become a decode row
    --t->rest_iters;
    if (t->gen_tokens_cnt >= t->min_new_tokens) t->logit_flags &= ~2u;  // the stops are free from the next step on
    return fed;
}

// walk: a guided request takes its automaton over the bytes of every token that does not end it.  The mask allowed only tokens that keep
// the automaton alive, so the dead state here means kernel and host disagree.  false: the guide is broken, and the state stays where it was
bool LLMGenerator::WalkGuide(TidData* t, int tok, bool hit_stop) const {
    if (t->guide_slot < 0) return true;
    if (hit_stop) return guide_cache_.Accepting(t->guide_slot, t->guide_state);  // an end token in front of a full match
    std::string bytes;
    tokenizer_->TokenBytes(tok, &bytes);
    const int32_t to = bytes.empty() ? -1 : guide_cache_.Step(t->guide_slot, t->guide_state, bytes);
    if (to < 0) return false;
    t->guide_state = to;
    return true;
}

// decide: does the request fail on this step, alone, and with which words.  The first reason that holds speaks
static bool RowFailure(const TidData& t, int tok, bool guide_broken, bool no_prompt, bool no_top, RetCode* code, std::string* msg) {
    *code = guide_broken || t.rule_failed ? RC_OTHER_ERROR : RC_UNSUPPORTED;
    if (guide_broken) {
        *msg = std::string(t.guide_schema ? "guide_json_schema" : "guide_regex") + ": internal error: token [" + std::to_string(tok) +
               "] is not allowed in state [" + std::to_string(t.guide_state) + "] of the request's guide";
    } else if (t.rule_failed) {
        *msg = "logit rules: the backend could not take the request's rule";
    } else if (no_prompt) {
        *msg = "prompt_logprobs: the backend's runtime has no SetPromptLogprobs";
    } else if (no_top) {
        *msg = "num_logprobs: the backend's post processor has no TopLogprobs";
    } else {
        return false;
    }
    return true;
}

// emit: the Response of the row's token, with the row's slice of the step's results
static TidGenToken EmitToken(const TidData& t, int tok, float logprob, FinishFlag flag, bool is_special, const ModelOutput& out,
                             const StepResults::Slice& mine) {
    TidGenToken g;
    g.is_token_in_out = t.is_token_in_out;
    Response& r = g.rsp;
    r.id = t.tid;
    r.token = tok;
    r.finish_flag = flag;
    r.logprob = logprob;
    r.is_special = is_special;
    if (mine.prompt_n > 0) {  // the prompt logprobs of a request go out with its first token
        const size_t from = mine.prompt_pos, to = from + mine.prompt_n, n = (size_t)t.prompt_logprobs, W = (size_t)PostProcessor::kTopLogprobsMax;
        r.prompt_logprobs.assign(out.prompt_logprobs.begin() + from, out.prompt_logprobs.begin() + to);
        r.prompt_ranks.assign(out.prompt_ranks.begin() + from, out.prompt_ranks.begin() + to);
        for (size_t i = from; n > 0 && i < to; ++i) {
            r.prompt_top_tokens.insert(r.prompt_top_tokens.end(), out.prompt_top_tokens.begin() + i * W, out.prompt_top_tokens.begin() + i * W + n);
            r.prompt_top_logprobs.insert(r.prompt_top_logprobs.end(), out.prompt_top_logprobs.begin() + i * W, out.prompt_top_logprobs.begin() + i * W + n);
        }
    }
    if (mine.top_row >= 0) {
        // the row's first n slots; the ones behind the vocabulary (token -1) are padding
        const int32_t* tt = out.top_tokens.data() + (size_t)mine.top_row * PostProcessor::kTopLogprobsMax;
        const float* tl = out.top_logprobs.data() + (size_t)mine.top_row * PostProcessor::kTopLogprobsMax;
        int32_t n = 0;
        while (n < t.num_logprobs && tt[n] >= 0) ++n;
        r.top_tokens.assign(tt, tt + n);
        r.top_logprobs.assign(tl, tl + n);
    }
    return g;
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
                if (!StartRequest(*req, adm)) break;
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
            StepResults results(out);
            for (int row = 0; row < running_batch; ++row) {
                TidData* t = tid_list_[row];
                const int tok = out.output_token[row];
                // the prompt logprobs of a request arrive with its first token: its fed - 1 positions are the next ones of the step's results
                const bool scores_prompt = t->steps == 0 && t->prompt_logprobs >= 0;
                const int64_t fed = AdvanceRow(t, tok);
                const StepResults::Slice mine = results.Take(scores_prompt && !out.prompt_unsupported ? (size_t)(fed - 1) : 0, t->num_logprobs > 0);
                const bool hit_stop = t->early_stopping &&
                    (generator_config_.stop_tokens.count(tok) || (t->stop_tokens && t->stop_tokens->count(tok)));
                const bool guide_broken = !WalkGuide(t, tok, hit_stop);
                // a request that asks for what the backend does not have, or whose rule or guide broke, fails alone: it leaves like a
                // finished one, unanswered
                RetCode fail_code;
                std::string fail_msg;
                const bool failed = RowFailure(*t, tok, guide_broken, scores_prompt && out.prompt_unsupported,
                                               t->num_logprobs > 0 && out.top_unsupported, &fail_code, &fail_msg);
                FinishFlag flag = FinishFlag::NOT_FINISHED;
                if (t->rest_iters <= 0 || hit_stop || failed) {
                    flag = t->rest_iters <= 0 ? FinishFlag::LENGTH : FinishFlag::EOS_TOKEN;
                    if (cool_down > 0) --cool_down;
                    finished_tasks_.Push(FinishedTaskInfo(t->tid, FinishedTaskInfo::FROM_WORKER));
                    req_list_changed_ = true;
                }
                if (failed) conn_->NotifyFailure(t->tid, fail_code, fail_msg);
                else tokens->push_back(EmitToken(*t, tok, out.logprobs[row], flag, generator_config_.special_tokens.count(tok) > 0, out, mine));
            }
            // detokenise + send overlaps the next step (llm_generator.cc:738-745)
            decoder_thread_pool_.RunAsync([this, tokens](uint32_t, uint32_t) { SendTokens(tokens.get()); });
            if (finished_tasks_.Size() > 0) DeleteTasks();
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
