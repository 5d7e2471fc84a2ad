// Request / Response / Connection / profiler counters: the data the tools and the generator exchange
// (reference src/common/request.h:29-46, response.h:26-41, connection.h:28-35, profiler.h:27-115).
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "ppl/common/retcode.h"

namespace ppl { namespace llm {

struct Request final {
    Request() {}
    Request(uint64_t _id, std::string _prompt, float _temperature, uint32_t _generation_length)
        : id(_id), prompt(std::move(_prompt)), temperature(_temperature), generation_length(_generation_length) {}
    uint64_t id = 0;
    std::string prompt;
    float temperature = 1.f;
    float top_p = 0.f;
    int32_t top_k = 1;
    float repetition_penalty = 1.f;
    float presence_penalty = 0.f;
    float frequency_penalty = 0.f;
    int32_t generation_length = 0;
    bool early_stopping = true;
    bool is_token_in_out = false;
    std::shared_ptr<std::vector<int>> token_ids;
    std::shared_ptr<std::unordered_set<int>> stop_tokens;
    int32_t lora_slot = -1;  // LoRA adapter slot of this request (HipResourceManager::LoadAdapter), -1 = the base model
    uint64_t seed = 0;       // sampling seed (GeneratorConfig::per_request_sampling), 0 = none: the generator gives the request one
    // logprob and rank of every prompt token but the first under the model's own distribution (Response::prompt_logprobs): -1 off, 0 the
    // token alone, 1 .. 20 also the first n entries of every position's ranking; above 20: 20, below -1: -1.  Such a request takes no
    // prefix-cache hit (a cached prefix has no hidden states to score): its prefill starts at position 0
    int32_t prompt_logprobs = -1;
    int32_t num_logprobs = 0;  // ranked alternatives per generated token (Response::top_tokens); above 20: 20, negative: 0
    // logit rules (DESIGN.md "numerics", logit rules row; validated when the request is admitted, logit_rule.h):
    std::vector<std::pair<int32_t, float>> logit_bias;   // (token, value added to its raw logit); -inf bans the token
    std::shared_ptr<std::vector<int32_t>> allowed_tokens;  // the only tokens the request may produce; null: all
    std::vector<int32_t> banned_tokens;                  // tokens it never produces (single-token bad words)
    int32_t min_new_tokens = 0;                          // its stop tokens cannot be produced before this many tokens are out
    bool HasLogitRule() const { return !logit_bias.empty() || allowed_tokens || !banned_tokens.empty() || min_new_tokens > 0; }
};

enum class FinishFlag { NOT_FINISHED, LENGTH, EOS_TOKEN, STOP_SEQUENCE };

struct Response final {
    uint64_t id = 0;
    std::string generated;
    int token = 0;
    FinishFlag finish_flag = FinishFlag::NOT_FINISHED;
    float logprob = 0.f;
    bool is_special = false;
    // the first Request::num_logprobs tokens of the step's ranking and their logprobs (DESIGN.md "numerics", top-N logprobs): empty when
    // the request did not ask, else min(num_logprobs, vocab_size) entries; entry 0 is the greedy token
    std::vector<int32_t> top_tokens;
    std::vector<float> top_logprobs;
    // Request::prompt_logprobs >= 0, on the response that carries the request's FIRST generated token only: for prompt position t = 1 ..
    // L-1, at [t - 1], log softmax(logits[t-1])[prompt[t]] over the raw logits and the token's rank (0: it is the greedy token); for n >= 1
    // also n entries per position, at [(t - 1) * n ..), best first, entries behind the vocabulary token -1 / -inf.  Empty otherwise
    // (a prompt of one token asks for nothing)
    std::vector<float> prompt_logprobs;
    std::vector<int32_t> prompt_ranks;
    std::vector<int32_t> prompt_top_tokens;
    std::vector<float> prompt_top_logprobs;
};

struct GeneratorReqCounter final {
    uint64_t encode_cnt = 0;
    uint64_t encode_cost = 0;  // microseconds
    uint64_t output_tokens_per_req = 0;
    char padding[40];  // keep the producer-side and consumer-side counters on different cache lines
    uint64_t waiting_cnt = 0;
    uint64_t waiting_cost = 0;
};

struct WorkerPerStepCounter {
    struct Counters {
        uint64_t step_cnt = 0;
        uint64_t prepare_cost = 0;
        uint64_t set_input_cost = 0;
        uint64_t model_forward_cost = 0;
        uint64_t choose_token_cost = 0;  // penalty + sampling
        uint64_t post_process_cost = 0;
        uint64_t total_cost = 0;
        uint64_t input_token_cnt = 0;
        uint64_t output_token_cnt = 0;
        uint64_t cache_hit_count = 0;
    } global, current;
};

struct WorkerProfiler {
    uint64_t finished_task_cnt = 0;
    uint64_t kv_rest_blk = 0;
    uint64_t kv_max_blk = 0;
    uint64_t running_task = 0;
    uint64_t prefill_batch = 0;
    uint64_t prefill_tokens = 0;
    uint64_t max_running_task = 0;
    uint64_t pending_task_size = 0;
    uint64_t dev_mem_total = 0;
    uint64_t dev_mem_free = 0;
    WorkerPerStepCounter step_counter;
    GeneratorReqCounter req_counter;
};

void PrintProfiler(const WorkerProfiler& worker_profiler);

class Connection {
public:
    virtual ~Connection() {}
    virtual void OnProfiling(const std::shared_ptr<WorkerProfiler>&) = 0;
    virtual void OnTokenize(uint64_t id, const std::vector<int>&) = 0;
    virtual void Send(const std::vector<Response>&) = 0;
    virtual void NotifyFailure(uint64_t id, ppl::common::RetCode, const std::string& errmsg) = 0;
};

}}  // namespace ppl::llm
