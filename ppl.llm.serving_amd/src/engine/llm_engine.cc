#include "llm_engine.h"

#include <algorithm>
#include <mutex>

#include "../utils/utils.h"
#include "ppl/common/log.h"

using namespace ppl::common;

namespace ppl { namespace llm {

LLMEngine::LLMEngine(const Resource& resource, const ModelConfig& model_config, bool enable_penalty, int32_t top_k, float top_p,
                     bool per_request_sampling)
    : tensor_parallel_size_(resource.tensor_parallel_size)
    , device_worker_pool_(resource.device_worker_pool_)
    , kv_cache_max_tokens_(resource.kv_cache_max_tokens)
    , post_processor_(resource.post_processor)
    , adapters_(resource.adapters)
    , model_config_(model_config)
    , enable_penalty_(enable_penalty)
    , top_k_(top_k)
    , top_p_(top_p)
    , per_request_sampling_(per_request_sampling) {
    for (uint32_t i = 0; i < tensor_parallel_size_; ++i) runtimes_.push_back(resource.items[i].runtime);
}

// The reference's Init reshapes the kv_cache / kv_scale tensors per cache_layout (src/engine/llm_engine.cc:118-169).
// In this build the slab shape is a property of the backend (it derives the four layouts' strides itself), so Init
// only validates what the reference validates there.
RetCode LLMEngine::Init(WorkerPerStepCounter* step_counter) {
    step_counter_ = step_counter;
    if (model_config_.cache_layout < 0 || model_config_.cache_layout > 3) {
        LOG(ERROR) << "impossible status: cache_layout = [" << model_config_.cache_layout << "]";
        return RC_INVALID_VALUE;
    }
    for (auto* rt : runtimes_) {
        if (!rt) {
            LOG(ERROR) << "resource item without runtime";
            return RC_INVALID_VALUE;
        }
    }
    if (per_request_sampling_ &&
        (!post_processor_ || post_processor_->SampleRows(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, model_config_.vocab_size,
                                                         model_config_.vocab_size, nullptr, nullptr) != RC_SUCCESS)) {
        LOG(ERROR) << "per_request_sampling is on, but the backend's post processor has no per-request sampler (SampleRows)";
        return RC_UNSUPPORTED;
    }
    return RC_SUCCESS;
}

static RetCode UploadInputs(uint32_t rank, const StepInputs& in, const std::vector<Runtime*>& runtimes) {
    const RetCode rc = runtimes[rank]->SetInputs(in);
    if (rc != RC_SUCCESS) LOG(ERROR) << "set inputs on rank [" << rank << "] failed: " << runtimes[rank]->GetLastError();
    return rc;
}

static RetCode RunDecoder(uint32_t rank, bool is_prefix_cache_hit, const std::vector<Runtime*>& runtimes) {
    const RetCode rc = runtimes[rank]->Run(is_prefix_cache_hit);
    if (rc != RC_SUCCESS) LOG(ERROR) << "run on rank [" << rank << "] failed: " << runtimes[rank]->GetLastError();
    return rc;
}

// a failed call of the step: `what` failed with `rc` (`detail`: the backend's own words behind it); the step fails with RC_OTHER_ERROR
static RetCode Fail(std::string* error_msg, const std::string& what, RetCode rc, const std::string& detail = "") {
    *error_msg = what + " failed: " + GetRetCodeStr(rc) + detail;
    LOG(ERROR) << *error_msg;
    return RC_OTHER_ERROR;
}

// does any row of the step ask: the stages of a step nobody asks for are not called at all
template <typename T, typename Pred>
static bool AnyRow(const std::vector<T>& list, Pred asks) {
    return std::any_of(list.begin(), list.end(), asks);
}

RetCode LLMEngine::Execute(const ModelInput& in, bool req_list_changed, bool is_prefix_cache_hit, ModelOutput* out,
                           std::string* error_msg) {
    const int32_t running_batch = (int32_t)in.start_pos.size();
    RetCode rc;

    StepInputs step;
    step.batch = running_batch;
    step.num_tokens = (int64_t)in.token_inputs.size();
    step.decoding_batches = in.decoding_batches;
    step.max_seq_len = in.max_seq_len;
    step.max_kv_len = in.max_kv_len;
    step.max_pages = in.max_pages;
    step.token_inputs = in.token_inputs.data();
    step.seq_starts = in.seq_starts.data();
    step.kv_starts = in.kv_starts.data();
    step.start_pos = in.start_pos.data();
    // cache_mode 0: cache_indices every step; cache_mode 1: the page table, consumed only when the batch changed
    // (src/engine/llm_engine.cc:63-71)
    step.cache_indices = model_config_.cache_mode == 0 ? in.cache_indices.data() : in.page_list.data();
    step.req_list_changed = req_list_changed;
    if (AnyRow(in.lora_slots, [](int32_t s) { return s >= 0; })) step.lora_slots = in.lora_slots.data();
    const auto device_lock = DeviceLock();

    {
        utils::TimingGuard timing(&step_counter_->current.set_input_cost);
        rc = utils::ParallelExecute(UploadInputs, device_worker_pool_, step, runtimes_);
        if (rc != RC_SUCCESS) return Fail(error_msg, "ParallelExecute(SetInputTask)", rc);
    }
    step_counter_->global.set_input_cost += step_counter_->current.set_input_cost;

    // prompt logprobs: the ask goes to rank 0 between its inputs and its run, only on steps in which a request asks (the generator asks
    // on a request's first step only); under tensor parallelism the backend refuses and the asking requests fail alone
    bool prompt_asks = AnyRow(in.prompt_logprobs_list, [](int32_t n) { return n >= 0; });
    if (prompt_asks) {
        rc = runtimes_[0]->SetPromptLogprobs(in.prompt_logprobs_list.data(), running_batch);
        if (rc == RC_UNSUPPORTED) {
            out->prompt_unsupported = true;
            prompt_asks = false;
        } else if (rc != RC_SUCCESS) {
            return Fail(error_msg, "SetPromptLogprobs", rc, std::string(": ") + runtimes_[0]->GetLastError());
        }
    }

    {
        utils::TimingGuard timing(&step_counter_->current.model_forward_cost);
        rc = utils::ParallelExecute(RunDecoder, device_worker_pool_, is_prefix_cache_hit, runtimes_);
        if (rc != RC_SUCCESS) return Fail(error_msg, "ParallelExecute(RunModelTask)", rc);
    }
    step_counter_->global.model_forward_cost += step_counter_->current.model_forward_cost;

    {
        utils::TimingGuard timing(&step_counter_->current.choose_token_cost);
        Runtime* rt0 = runtimes_[0];  // sampling happens on rank 0's logits only (src/engine/llm_engine.cc:200)
        int64_t stride = 0;
        float* logits = rt0->GetLogits(&stride);
        // guided decoding: the asking rows lose every token their automaton's state does not allow, in front of everything else that
        // reads or edits the logits; nothing on a step without an asking row
        if (AnyRow(in.guide_slots, [](int32_t g) { return g >= 0; })) {
            rc = post_processor_->GuideEdit(logits, in.guide_slots.data(), in.guide_states.data(), running_batch, model_config_.vocab_size,
                                            (int32_t)stride);
            if (rc != RC_SUCCESS) return Fail(error_msg, "GuideEdit", rc);
        }
        // logit rules: in place and first, so a bias is in raw-logit units and the penalty, the top-N logprobs and the sampler all see
        // the edited rows; nothing on a step without a flag
        if (AnyRow(in.logit_flags, [](uint32_t f) { return f != 0; })) {
            rc = post_processor_->EditLogits(logits, in.batch_slots.data(), in.logit_flags.data(), running_batch, model_config_.vocab_size,
                                             (int32_t)stride);
            if (rc != RC_SUCCESS) return Fail(error_msg, "EditLogits", rc);
        }
        if (enable_penalty_) {
            rc = post_processor_->ApplyPenalty(in.temperatures.data(), in.repetition_penalty_list.data(), nullptr, nullptr,
                                               in.batch_slots.data(), rt0->GetTokenInputsDevice(), rt0->GetSeqStartsDevice(),
                                               rt0->GetStartPosDevice(), running_batch, model_config_.vocab_size,
                                               req_list_changed, logits);
            if (rc != RC_SUCCESS) return Fail(error_msg, "Apply Penalty", rc);
        }
        // top-N logprobs: queued in front of the sampler, whose synchronisation makes the results readable; nothing on a step nobody asks in
        const int32_t* top_tok = nullptr;
        const float* top_lp = nullptr;
        int32_t top_rows = 0;
        if (AnyRow(in.num_logprobs_list, [](int32_t n) { return n > 0; })) {
            rc = post_processor_->TopLogprobs(logits, enable_penalty_ ? nullptr : in.temperatures.data(), in.num_logprobs_list.data(),
                                              running_batch, model_config_.vocab_size, (int32_t)stride, &top_tok, &top_lp, &top_rows);
            if (rc == RC_UNSUPPORTED) {
                out->top_unsupported = true;
                top_rows = 0;
            } else if (rc != RC_SUCCESS) {
                return Fail(error_msg, "TopLogprobs", rc);
            }
        }
        const char* sampler = per_request_sampling_ ? "SampleRows" : "SampleTopKTopP";
        // (a ModelInput packed without the two lists asks for nothing)
        const bool has_trunc_lists = in.min_p_list.size() == (size_t)running_batch && in.typical_p_list.size() == (size_t)running_batch;
        bool truncates = false;
        for (int32_t b = 0; b < running_batch && per_request_sampling_ && has_trunc_lists && !truncates; ++b)
            truncates = PostProcessor::RowTruncates(in.top_k_list[b], in.min_p_list[b], in.typical_p_list[b]);
        if (truncates) {
            // a row of the step cuts its tail by min_p or typical_p: the sampler that knows the two; every other step takes today's call
            sampler = "SampleRowsTrunc";
            rc = post_processor_->SampleRowsTrunc(logits, enable_penalty_ ? nullptr : in.temperatures.data(), in.top_k_list.data(),
                                                  in.top_p_list.data(), in.min_p_list.data(), in.typical_p_list.data(), in.seed_list.data(),
                                                  in.draw_list.data(), running_batch, model_config_.vocab_size, (int32_t)stride,
                                                  out->output_token.data(), out->logprobs.data());
        } else if (per_request_sampling_) {
            // every row its own parameters and random number (the penalty step has applied the temperatures already)
            rc = post_processor_->SampleRows(logits, enable_penalty_ ? nullptr : in.temperatures.data(), in.top_k_list.data(),
                                             in.top_p_list.data(), in.seed_list.data(), in.draw_list.data(), running_batch,
                                             model_config_.vocab_size, (int32_t)stride, out->output_token.data(), out->logprobs.data());
        } else {
            // only top_k_list[0] reaches the kernel (src/engine/llm_engine.cc:219)
            const int32_t default_top_k = in.top_k_list.empty() ? top_k_ : in.top_k_list[0];
            rc = post_processor_->SampleTopKTopP(logits, in.temperatures.data(), in.top_k_list.data(), in.top_p_list.data(),
                                                 running_batch, model_config_.vocab_size, (int32_t)stride, default_top_k, top_p_,
                                                 req_list_changed, out->output_token.data(), out->logprobs.data(),
                                                 enable_penalty_);
        }
        if (rc != RC_SUCCESS) return Fail(error_msg, sampler, rc);
        if (prompt_asks) {   // the sampler has synchronised: the step's prompt logprobs are readable
            PromptLogprobsView v;
            rc = rt0->GetPromptLogprobs(&v);
            if (rc != RC_SUCCESS) return Fail(error_msg, "GetPromptLogprobs", rc);
            const size_t P = (size_t)v.positions, cnt = P * PostProcessor::kTopLogprobsMax;
            if (P > 0) {
                out->prompt_rows.assign(v.rows, v.rows + P);
                out->prompt_logprobs.assign(v.logprobs, v.logprobs + P);
                out->prompt_ranks.assign(v.ranks, v.ranks + P);
                out->prompt_top_tokens.assign(v.top_tokens, v.top_tokens + cnt);
                out->prompt_top_logprobs.assign(v.top_logprobs, v.top_logprobs + cnt);
            }
        }
        if (top_rows > 0) {
            const size_t cnt = (size_t)top_rows * PostProcessor::kTopLogprobsMax;
            out->top_tokens.assign(top_tok, top_tok + cnt);
            out->top_logprobs.assign(top_lp, top_lp + cnt);
            out->top_rows = top_rows;
        }
    }
    step_counter_->global.choose_token_cost += step_counter_->current.choose_token_cost;
    step_counter_->current.output_token_cnt = running_batch;
    step_counter_->global.output_token_cnt += running_batch;
    return RC_SUCCESS;
}

}}  // namespace ppl::llm
