// What the generator/engine require of a backend (reference: PostProcessor src/common/post_processor.h:25-43,
// Resource/ResourceItem src/common/resource.h:33-49, and the ppl.nn Runtime/Tensor surface the engine drives,
// src/engine/llm_engine.h:124-147, llm_engine.cc:29-116).  The reference binds eleven ppl::nn::Tensor objects by
// index; here the same data crosses the boundary as ONE StepInputs record per rank (-> pplhip_step), because the
// HIP runtime stages it in pinned memory and issues a single H2D copy.
#pragma once
#include <stdint.h>

#include <vector>

#include "adapter_registry.h"
#include "guide.h"
#include "logit_rule.h"
#include "ppl/common/retcode.h"
#include "ppl/common/threadpool.h"

namespace ppl { namespace llm {

class PostProcessor {
public:
    virtual ~PostProcessor() {}
    virtual ppl::common::RetCode InitPostProcessorMem(int max_running_batch, int vocab_size, bool enable_penalty) = 0;
    // logits_device -> output_host / logprob_host; blocking (the step's one synchronisation)
    virtual ppl::common::RetCode SampleTopKTopP(const float* logits_device, const float* temperatures_host,
                                                const int32_t* top_k_host, const float* top_p_host, int32_t batch,
                                                int32_t vocab_size, int32_t batch_stride, int32_t default_top_k,
                                                float default_top_p, bool req_list_changed, int32_t* output_host,
                                                float* logprob_host, bool enable_penalty) = 0;
    virtual ppl::common::RetCode ApplyPenalty(const float* temperatures_host, const float* repetition_penalties_host,
                                              const float* presence_penalties_host, const float* frequency_penalties_host,
                                              const int64_t* batch_slots_host, const int64_t* token_inputs,
                                              const int64_t* seqstarts, const int64_t* start_pos, int32_t batch,
                                              int32_t vocab_size, bool req_list_changed, float* logits) = 0;
    // The per-request sampler (GeneratorConfig::per_request_sampling): row b is answered with ITS temperature, top_k, top_p and the random
    // number of (seeds[b], draws[b]); every array is consumed on every call (no req_list_changed).  temperatures_host NULL: the penalty
    // step already divided by them.  Blocking, like SampleTopKTopP.  batch == 0 touches nothing and only tells whether the backend can do
    // it (LLMEngine::Init asks so); a backend that cannot keeps this default.
    virtual ppl::common::RetCode SampleRows(const float* /*logits_device*/, const float* /*temperatures_host*/, const int32_t* /*top_k_host*/,
                                            const float* /*top_p_host*/, const uint64_t* /*seeds_host*/, const uint64_t* /*draws_host*/,
                                            int32_t /*batch*/, int32_t /*vocab_size*/, int32_t /*batch_stride*/, int32_t* /*output_host*/,
                                            float* /*logprob_host*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    // SampleRows with two more truncations per row (DESIGN.md "numerics", min_p / typical_p row): min_p_host[b] keeps the candidates whose
    // probability is at least min_p times the most probable one's (off when <= 0 or NaN), typical_p_host[b] is locally typical sampling
    // over what is left (off when <= 0, >= 1 or NaN).  The engine calls it only on steps in which a row has one of the two on
    // (RowTruncates), SampleRows on every other step.  batch == 0 touches nothing and only tells whether the backend can do it (the
    // generator asks so when a request that sets either is admitted); a backend that cannot keeps this default, and the requests that
    // ask are failed.
    virtual ppl::common::RetCode SampleRowsTrunc(const float* /*logits_device*/, const float* /*temperatures_host*/,
                                                 const int32_t* /*top_k_host*/, const float* /*top_p_host*/, const float* /*min_p_host*/,
                                                 const float* /*typical_p_host*/, const uint64_t* /*seeds_host*/,
                                                 const uint64_t* /*draws_host*/, int32_t /*batch*/, int32_t /*vocab_size*/,
                                                 int32_t /*batch_stride*/, int32_t* /*output_host*/, float* /*logprob_host*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    // whether a row with these parameters is a truncating row: not greedy, and min_p or typical_p on
    static bool RowTruncates(int32_t top_k, float min_p, float typical_p) {
        return top_k != 1 && (min_p > 0.f || (typical_p > 0.f && typical_p < 1.f));
    }
    // Top-N logprobs of the rows with num_logprobs_host[b] > 0 (0 .. kTopLogprobsMax), on the logits the step's sampler is about to see.
    // NOT blocking: *tokens / *logprobs point at backend-owned host memory, [*rows, kTopLogprobsMax] each, row j = the j-th asking batch
    // row, valid once the step's sampler call (SampleTopKTopP / SampleRows) has returned and until the next TopLogprobs.  Entries behind
    // a row's n are undefined; entries behind the vocabulary are token -1.  The engine calls it only on steps in which a row asks.  A
    // backend that cannot keeps this default, and the requests that ask are failed.
    static constexpr int32_t kTopLogprobsMax = 20;
    virtual ppl::common::RetCode TopLogprobs(const float* /*logits_device*/, const float* /*temperatures_host*/,
                                             const int32_t* /*num_logprobs_host*/, int32_t /*batch*/, int32_t /*vocab_size*/,
                                             int32_t /*batch_stride*/, const int32_t** /*tokens*/, const float** /*logprobs*/,
                                             int32_t* /*rows*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    // Logit rules (DESIGN.md "numerics", logit rules row).  SetLogitRule hands the backend the merged, validated rule of the request that
    // owns batch slot `slot` (logit_rule.h: BuildLogitRule), once, before the request's first step; NOT blocking, ordered in front of
    // every later EditLogits.  EditLogits edits the rows with flags_host[b] != 0 in place with the rule of batch_slots_host[b] (bit 0:
    // mask and bias, bit 1: suppress the rule's stops); NOT blocking; the engine calls it in front of ApplyPenalty and only on steps in
    // which a flag is set.  batch == 0 touches nothing and only tells whether the backend can do it (the generator asks so when a
    // request with a rule is admitted); a backend that cannot keeps these defaults, and the requests that ask are failed.
    static constexpr int32_t kLogitBiasMax = 512;
    static constexpr int32_t kLogitStopMax = 64;
    virtual ppl::common::RetCode SetLogitRule(int64_t /*slot*/, const LogitRule& /*rule*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    virtual ppl::common::RetCode EditLogits(float* /*logits_device*/, const int64_t* /*batch_slots_host*/, const uint32_t* /*flags_host*/,
                                            int32_t /*batch*/, int32_t /*vocab_size*/, int32_t /*batch_stride*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    // Guided decoding (DESIGN.md "numerics", guided decoding row).  SetGuideVocab hands the backend the bytes of every token, once:
    // token t < n_tok is bytes[offsets[t] .. offsets[t + 1]).  LoadGuide builds guide slot `slot` (0 .. kGuideMaxSlots - 1) from a DFA
    // (guide.h) and the end tokens, which are allowed exactly in accepting states; BLOCKING, once per distinct pattern; RC_INVALID_VALUE
    // when some state of the automaton allows no token of the vocabulary.  UnloadGuide frees a slot that no running request names.
    // GuideEdit sets to -inf, in row b, every token that state states_host[b] of slot guide_slots_host[b] does not allow (-1: the row
    // does not ask); NOT blocking; the engine calls it in front of EditLogits and only on steps with an asking row.  batch == 0 touches
    // nothing and only tells whether the backend can do it.  A backend that cannot keeps these defaults, and guided requests are failed.
    static constexpr int32_t kGuideMaxSlots = 16;
    static constexpr int32_t kGuideMaxStates = 255;
    virtual ppl::common::RetCode SetGuideVocab(const uint8_t* /*bytes*/, const int64_t* /*offsets*/, int32_t /*n_tok*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    virtual ppl::common::RetCode LoadGuide(int32_t /*slot*/, const GuideDfa& /*dfa*/, const std::vector<int32_t>& /*end_tokens*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    // the same for the wide automaton of a JSON schema (up to kGuide16MaxStates states); the slots are the same, a slot holds either
    // kind, and UnloadGuide / GuideEdit serve both.  A backend without it keeps this default: a request with a schema then fails alone
    static constexpr int32_t kGuide16MaxStates = 4096;
    virtual ppl::common::RetCode LoadGuide16(int32_t /*slot*/, const GuideDfa16& /*dfa*/, const std::vector<int32_t>& /*end_tokens*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
    virtual ppl::common::RetCode UnloadGuide(int32_t /*slot*/) { return ppl::common::RC_UNSUPPORTED; }
    virtual ppl::common::RetCode GuideEdit(float* /*logits_device*/, const int32_t* /*guide_slots_host*/, const int32_t* /*states_host*/,
                                           int32_t /*batch*/, int32_t /*vocab_size*/, int32_t /*batch_stride*/) {
        return ppl::common::RC_UNSUPPORTED;
    }
};

// one step of one rank: the 11-input contract of src/engine/llm_engine.h:124-138 (attn_mask is never written by the
// reference, llm_engine.cc:29-111, and is not carried)
struct StepInputs {
    int64_t batch = 0, num_tokens = 0;
    int64_t decoding_batches = 0, max_seq_len = 0, max_kv_len = 0, max_pages = 0;
    const int64_t* token_inputs = nullptr;
    const int64_t* seq_starts = nullptr;
    const int64_t* kv_starts = nullptr;
    const int64_t* start_pos = nullptr;
    const int64_t* cache_indices = nullptr;  // mode 0: [B]; mode 1: [B, max_pages], only read when req_list_changed
    bool req_list_changed = true;
    const int32_t* lora_slots = nullptr;     // [B] adapter slot per request, -1 = none; NULL when no request of the step has one
};

// Prompt logprobs of one step (DESIGN.md "numerics", prompt logprobs row): position i is packed row rows[i] of the step (ascending), scored
// against token_inputs[rows[i] + 1]; top_tokens / top_logprobs are [positions, PostProcessor::kTopLogprobsMax], the first n slots of a
// position whose request asked n >= 1 (entries behind the vocabulary: token -1).  Backend-owned host memory.
struct PromptLogprobsView {
    int64_t positions = 0;
    const int32_t* rows = nullptr;
    const float* logprobs = nullptr;
    const int32_t* ranks = nullptr;
    const int32_t* top_tokens = nullptr;
    const float* top_logprobs = nullptr;
};

// the runtime handle of one tensor-parallel rank (ppl::nn::Runtime + its bound tensors in the reference)
class Runtime {
public:
    virtual ~Runtime() {}
    // Prompt logprobs.  SetPromptLogprobs: ask_host [batch], -1 (off) .. 20 per request of the step SetInputs staged, between SetInputs
    // and Run; request b with ask >= 0 has its rows s .. e-2 scored against the tokens that follow them, under the model's own
    // distribution (raw logits).  The engine calls it only on steps in which a request asks.  GetPromptLogprobs: the results of the last
    // Run, valid once the step's sampler call has returned and until the next Run.  A backend that cannot keeps these defaults, and the
    // requests that ask are failed.
    virtual ppl::common::RetCode SetPromptLogprobs(const int32_t* /*ask_host*/, int64_t /*batch*/) { return ppl::common::RC_UNSUPPORTED; }
    virtual ppl::common::RetCode GetPromptLogprobs(PromptLogprobsView* /*out*/) { return ppl::common::RC_UNSUPPORTED; }
    virtual ppl::common::RetCode SetInputs(const StepInputs&) = 0;           // SetInputTask (async)
    virtual ppl::common::RetCode Run(bool is_prefix_cache_hit) = 0;          // RunModelTask (async)
    virtual float* GetLogits(int64_t* batch_stride) = 0;                     // logits tensor: device ptr + dim(1)
    // device-resident step arrays for ApplyPenalty (llm_engine.cc:207-211)
    virtual const int64_t* GetTokenInputsDevice() const { return nullptr; }
    virtual const int64_t* GetSeqStartsDevice() const { return nullptr; }
    virtual const int64_t* GetStartPosDevice() const { return nullptr; }
    virtual const char* GetLastError() const { return ""; }
};

struct ResourceItem final {
    void* kv_cache_mem = nullptr;
    void* kv_scale_mem = nullptr;
    Runtime* runtime = nullptr;
};

class Tokenizer;  // out of scope (token-in/token-out path only); kept so that Resource has the reference's shape

struct Resource final {
    uint32_t tensor_parallel_size = 0;
    uint64_t kv_cache_max_tokens = 0;
    std::vector<ResourceItem> items;
    PostProcessor* post_processor = nullptr;
    ppl::common::StaticThreadPool* device_worker_pool_ = nullptr;
    const Tokenizer* tokenizer = nullptr;
    AdapterRegistry* adapters = nullptr;     // LoRA adapter slots of the backend; NULL: the backend serves none
};

}}  // namespace ppl::llm
