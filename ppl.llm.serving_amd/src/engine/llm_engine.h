// The per-step operator API between the scheduler and a backend (reference src/engine/llm_engine.h:40-149):
// ModelInput (what the generator packs), ModelOutput (what sampling returns) and LLMEngine::Execute
// = upload step inputs on every tensor-parallel rank -> run the decoder on every rank -> penalty -> sampling on rank 0.
#pragma once
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "../common/config.h"
#include "../common/request.h"
#include "../common/resource.h"

namespace ppl { namespace llm {

struct ModelInput {
    int64_t decoding_batches = 0;
    int64_t max_seq_len = 0;
    int64_t max_kv_len = 0;
    int64_t max_pages = 0;

    std::vector<int64_t> token_inputs;
    std::vector<int64_t> seq_starts;
    std::vector<int64_t> start_pos;
    std::vector<int64_t> cache_indices;
    std::vector<int64_t> page_list;
    std::vector<int64_t> kv_starts;
    std::vector<float> temperatures;
    std::vector<float> top_p_list;
    std::vector<float> min_p_list;      // Request::min_p per request (<= 0 or NaN: off)
    std::vector<float> typical_p_list;  // Request::typical_p per request (<= 0, >= 1 or NaN: off)
    std::vector<int32_t> top_k_list;
    std::vector<uint64_t> seed_list;  // sampling seed per request (per_request_sampling)
    std::vector<uint64_t> draw_list;  // tokens the request has produced so far: 0 on the step that ends its prefill

    std::vector<float> repetition_penalty_list;
    std::vector<float> presence_penalty_list;
    std::vector<float> frequency_penalty_list;
    std::vector<int64_t> batch_slots;
    std::vector<int32_t> lora_slots;  // adapter slot per request (Request::lora_slot), -1 = none
    std::vector<int32_t> prompt_logprobs_list;  // prompt logprobs per request (Request::prompt_logprobs, clamped to -1 .. 20; -1 again after the request's first step)
    std::vector<int32_t> num_logprobs_list;  // top-N logprobs per request (Request::num_logprobs, clamped to 0 .. 20)
    // logit rules per request: 0 = the request has none; bit 0 = apply the mask and bias of the rule in its batch slot, bit 1 = suppress
    // the rule's stop tokens (set while the request has produced fewer than min_new_tokens tokens)
    std::vector<uint32_t> logit_flags;
    // guided decoding per request: the guide slot its pattern is loaded in (-1 = the request has no guide) and the state of the
    // automaton after the bytes it has generated so far
    std::vector<int32_t> guide_slots;
    std::vector<int32_t> guide_states;
};

struct ModelOutput {
    std::vector<int32_t> output_token;
    std::vector<float> logprobs;
    // top-N logprobs, compact: [top_rows, PostProcessor::kTopLogprobsMax] each, row j = the j-th batch row with num_logprobs_list > 0
    std::vector<int32_t> top_tokens;
    std::vector<float> top_logprobs;
    int32_t top_rows = 0;
    bool top_unsupported = false;  // a row asked and the backend has no TopLogprobs: the generator fails those requests
    // prompt logprobs of the step, ascending packed row: position i scores row prompt_rows[i]; the top arrays are
    // [positions, PostProcessor::kTopLogprobsMax]
    std::vector<int32_t> prompt_rows, prompt_ranks, prompt_top_tokens;
    std::vector<float> prompt_logprobs, prompt_top_logprobs;
    bool prompt_unsupported = false;  // a request asked and the backend has no SetPromptLogprobs: the generator fails those requests
    void Clear() {
        output_token.clear();
        logprobs.clear();
        top_tokens.clear();
        top_logprobs.clear();
        top_rows = 0;
        top_unsupported = false;
        prompt_rows.clear();
        prompt_ranks.clear();
        prompt_top_tokens.clear();
        prompt_logprobs.clear();
        prompt_top_logprobs.clear();
        prompt_unsupported = false;
    }
    void Resize(int32_t n) {
        output_token.resize(n);
        logprobs.resize(n);
    }
};

class LLMEngine final {
public:
    LLMEngine(const Resource& resource, const ModelConfig& model_config, bool enable_penalty, int32_t top_k, float top_p,
              bool per_request_sampling = false);

    ppl::common::RetCode Init(WorkerPerStepCounter* step_counter);
    ppl::common::RetCode Execute(const ModelInput& model_input, bool req_list_changed, bool is_prefix_cache_hit,
                                 ModelOutput* model_output, std::string* error_msg);
    // logit rules: whether the backend's post processor has them (PostProcessor::EditLogits with batch 0), and the upload of one slot's rule
    bool HasLogitRules() const {
        return post_processor_ && post_processor_->EditLogits(nullptr, nullptr, nullptr, 0, model_config_.vocab_size,
                                                              model_config_.vocab_size) == ppl::common::RC_SUCCESS;
    }
    ppl::common::RetCode SetLogitRule(int64_t slot, const LogitRule& rule) { auto lock = DeviceLock(); return post_processor_->SetLogitRule(slot, rule); }

    // min_p / typical_p: whether the backend's post processor has the truncating sampler (PostProcessor::SampleRowsTrunc with batch 0)
    bool HasSampleRowsTrunc() const {
        return post_processor_ && post_processor_->SampleRowsTrunc(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                                                   model_config_.vocab_size, model_config_.vocab_size, nullptr,
                                                                   nullptr) == ppl::common::RC_SUCCESS;
    }

    // guided decoding: whether the backend's post processor has it (PostProcessor::GuideEdit with batch 0), and its three set-up calls
    bool HasGuides() const {
        return post_processor_ && post_processor_->GuideEdit(nullptr, nullptr, nullptr, 0, model_config_.vocab_size,
                                                             model_config_.vocab_size) == ppl::common::RC_SUCCESS;
    }
    ppl::common::RetCode SetGuideVocab(const uint8_t* bytes, const int64_t* offsets, int32_t n_tok) {
        auto lock = DeviceLock(); return post_processor_->SetGuideVocab(bytes, offsets, n_tok);
    }
    ppl::common::RetCode LoadGuide(int32_t slot, const GuideDfa& dfa, const std::vector<int32_t>& end_tokens) {
        auto lock = DeviceLock(); return post_processor_->LoadGuide(slot, dfa, end_tokens);
    }
    ppl::common::RetCode LoadGuide16(int32_t slot, const GuideDfa16& dfa, const std::vector<int32_t>& end_tokens) {
        auto lock = DeviceLock(); return post_processor_->LoadGuide16(slot, dfa, end_tokens);
    }
    ppl::common::RetCode UnloadGuide(int32_t slot) { auto lock = DeviceLock(); return post_processor_->UnloadGuide(slot); }

private:
    // a backend with adapters loads and unloads them on the same device as the step and its set-up calls: one or the other at a time
    std::unique_lock<std::mutex> DeviceLock() const {
        return adapters_ ? std::unique_lock<std::mutex>(adapters_->DeviceMutex()) : std::unique_lock<std::mutex>();
    }

    uint32_t tensor_parallel_size_;
    ppl::common::StaticThreadPool* device_worker_pool_;
    std::vector<Runtime*> runtimes_;
    uint64_t kv_cache_max_tokens_;
    PostProcessor* post_processor_;
    AdapterRegistry* adapters_;
    ModelConfig model_config_;
    bool enable_penalty_;
    int32_t top_k_;
    float top_p_;
    bool per_request_sampling_;
    WorkerPerStepCounter* step_counter_ = nullptr;
};

}}  // namespace ppl::llm
