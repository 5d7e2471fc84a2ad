// Continuous-batching scheduler of the hot path (reference src/generator/llm_generator.h:127-182,
// llm_generator.cc:574-786): request queue -> admission (token budget, length clamps, KV reservation, prefix-cache
// lookup) -> ModelInput packing -> LLMEngine::Execute -> finish detection -> asynchronous send -> KV release and
// batch compaction.  Public surface (Init / Process / ClearTask / GetPendingTaskNum) is the reference's.
#pragma once
#include <pthread.h>

#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <unordered_set>
#include <vector>

#include "../common/config.h"
#include "../common/request.h"
#include "../common/resource.h"
#include "../engine/llm_engine.h"
#include "../tokenizer/tokenizer.h"
#include "../utils/index_manager.h"
#include "../utils/mpsc_request_scheduler.h"
#include "../utils/prefix_cache_manager.h"
#include "guide_cache.h"
#include "ppl/common/allocators.h"
#include "ppl/common/mpsc_queue.h"
#include "ppl/common/threadpool.h"

namespace ppl { namespace llm {

// one generated token on its way to the connection: its Response, all but the text (SendTokens decodes that)
struct TidGenToken final {
    Response rsp;
    bool is_token_in_out;
};

struct FinishedTaskInfo final {
    enum { UNKNOWN, FROM_WORKER, FROM_CONN };
    FinishedTaskInfo(uint64_t fid = UINT64_MAX, uint32_t ftype = UNKNOWN) : id(fid), type(ftype) {}
    uint64_t id;
    uint32_t type;
};

// per running request (reference TidData, llm_generator.h:79-103).  Everything a request carries from step to step lives here and only
// here: PackStep builds every per-row list of ModelInput from these records, every step
struct TidData final {
    uint64_t tid = 0;
    float temperature = 1.f;
    float top_p = 0.f;
    float min_p = 0.f;
    float typical_p = 1.f;
    int32_t top_k = 1;
    float repetition_penalty = 1.f;
    float presence_penalty = 0.f;
    float frequency_penalty = 0.f;
    bool early_stopping = true;
    int32_t rest_iters = 0;
    bool is_token_in_out = false;
    int64_t total_len = 0;  // prompt + rest_iters at admission; KV reserved = total_len - 1
    std::shared_ptr<std::unordered_set<int>> stop_tokens;
    std::shared_ptr<std::vector<int>> next_tokens;
    int64_t start_pos = 0;
    uint64_t cache_index = 0;
    std::vector<int64_t> page_list;
    int64_t slot_index = 0;  // batch slot: the penalty count map row and the logit rule record; INT64_MAX: the request holds none
    int32_t steps = 0;
    int32_t gen_tokens_cnt = 0;
    std::vector<uint64_t> hash_list;  // hashes of this request's full prompt pages (cached + newly inserted)
    int64_t cache_hit_count = 0;
    int32_t lora_slot = -1;  // holds a reference in the adapter registry until the request leaves
    uint64_t seed = 0;       // sampling seed: the request's own, or the generator's next one
    int32_t prompt_logprobs = -1;  // Request::prompt_logprobs, clamped to -1 .. PostProcessor::kTopLogprobsMax
    int32_t num_logprobs = 0;  // Request::num_logprobs, clamped to 0 .. PostProcessor::kTopLogprobsMax
    uint32_t logit_flags = 0;    // ModelInput::logit_flags of its row: 0 without a rule, and when the backend refused the rule
    int32_t min_new_tokens = 0;  // Request::min_new_tokens: bit 1 of logit_flags until this many tokens are out
    bool rule_failed = false;    // the upload of its logit rule failed: the request is failed on its first step
    int32_t guide_slot = -1;     // guided decoding: the guide slot the request holds a reference on until it leaves; -1: none
    int32_t guide_state = 0;     // the state of its automaton after the bytes generated so far
    bool guide_schema = false;   // the guide is a JSON schema's (guide_json_schema), not a regular expression's
};

struct LlmRequest final : public ppl::common::MPSCQueue::Node {
    std::shared_ptr<Request> orig;
    std::chrono::time_point<std::chrono::high_resolution_clock> enqueue_ts;
    uint64_t lora_uid = 0;  // uid of the adapter in orig->lora_slot when the request was queued (0: none): seed of its page-hash chain
};

// test hook: receives every ModelInput right before Execute
typedef void (*StepObserver)(void* arg, uint64_t step, const ModelInput& input, bool req_list_changed, bool is_prefix_cache_hit);

class LLMGenerator final {
public:
    LLMGenerator(const Resource& resource, const GeneratorConfig& generator_config, const ModelConfig& model_config,
                 Connection* conn);
    ~LLMGenerator();

    ppl::common::RetCode Init();
    void Process(const std::shared_ptr<Request>&);
    void ClearTask(uint64_t tid) { finished_tasks_.Push(FinishedTaskInfo(tid, FinishedTaskInfo::FROM_CONN)); }
    uint32_t GetPendingTaskNum() const { return sched_.GetPendingSize(); }

    void SetStepObserver(StepObserver f, void* arg) { observer_ = f; observer_arg_ = arg; }
    const WorkerProfiler& GetProfiler() const { return *worker_profiler_; }
    // nothing queued and no batch running (tools use it to drain before shutdown)
    bool IsIdle() const { return sched_.GetPendingSize() == 0 && !generating_.load(std::memory_order_acquire); }

private:
    struct Admission;  // scratch of one admission check (RequestCheckResult in the reference)

    ppl::common::RetCode CheckParameters() const;
    void Generate();
    bool AdmitRequest(const LlmRequest& req, Admission* adm, int32_t* cool_down, bool* is_prefix_cache_hit);
    bool ReserveKv(const LlmRequest& req, Admission* adm, int32_t* cool_down, bool* is_prefix_cache_hit);
    bool StartRequest(const LlmRequest& req, const Admission& adm);
    void PackStep(bool req_list_changed, ModelInput* model_input) const;
    bool WalkGuide(TidData* t, int tok, bool hit_stop) const;
    void DeleteTasks();
    void CompactBatch();
    void ReleaseRequest(const TidData& t, bool keep_cached_pages);
    void ReleaseResource();
    void SendTokens(std::vector<TidGenToken>* tokens);
    static void* GeneratorThreadFunc(void*);

private:
    const Tokenizer* tokenizer_;
    AdapterRegistry* adapters_;
    GeneratorConfig generator_config_;
    ModelConfig model_config_;
    Connection* conn_;
    uint64_t kv_cache_max_tokens_ = 0;
    LLMEngine llm_engine_;
    GuideCache guide_cache_;  // behind the engine it unloads its slots through when it goes
    ppl::common::StaticThreadPool decoder_thread_pool_;

    // running batch: row order == ModelInput row order
    std::vector<TidData*> tid_list_;
    std::map<uint64_t, TidData> tid_data_map_;
    bool req_list_changed_ = true;
    uint64_t unseeded_requests_ = 0;  // requests parsed without a seed of their own so far (the n of splitmix64(sampling_seed + n))
    ppl::common::TypedMPSCQueue<FinishedTaskInfo> finished_tasks_;

    utils::IndexManager idx_mgr_;
    utils::IndexManager batch_slots_mgr_;
    ppl::common::PageManager page_mgr_;
    utils::PrefixCacheManager prefix_cache_mgr_;
    std::shared_ptr<WorkerProfiler> worker_profiler_;

    std::atomic<bool> generate_thread_active_{false};
    std::atomic<bool> generating_{false};
    pthread_t generate_thread_;
    ppl::common::EventCount req_signal_;
    utils::MPSCRequestScheduler<LlmRequest> sched_;

    // U+FFFD buffering of the text path (llm_generator.cc:84-99)
    std::map<uint64_t, std::vector<int>> decode_buffer_;

    StepObserver observer_ = nullptr;
    void* observer_arg_ = nullptr;
    static constexpr int DECODER_THREAD_NUM = 1;
};

}}  // namespace ppl::llm
