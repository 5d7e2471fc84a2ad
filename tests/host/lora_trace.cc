// Test driver for per-request LoRA adapters on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   lora_trace    runs LLMGenerator + LLMEngine against a fake Runtime with an AdapterRegistry driven the way
//                 HipResourceManager::LoadAdapter / UnloadAdapter drive it, and prints one JSON line per step (what the backend
//                 received) and per registry event.  tests/test_lora_host.py holds the expectations.
//
// The fake model repeats the last input token of every row, and every prompt of the batch-order phase ends in 500 + request id: the last
// token of a row names the request it belongs to at every step.
#include <condition_variable>
#include <iostream>
#include <mutex>
#include <sstream>
#include <thread>

#include "common/adapter_registry.h"
#include "common/config.h"
#include "common/request.h"
#include "common/resource.h"
#include "generator/llm_generator.h"

using namespace ppl::llm;
using namespace ppl::common;

namespace {

template <typename T>
std::string Arr(const std::vector<T>& v) {
    std::ostringstream ss;
    ss << "[";
    for (size_t i = 0; i < v.size(); ++i) ss << (i ? "," : "") << v[i];
    ss << "]";
    return ss.str();
}

class FakeRuntime final : public Runtime {
public:
    explicit FakeRuntime(int vocab) : vocab_(vocab) {}
    RetCode SetInputs(const StepInputs& in) override {
        B_ = in.batch;
        last_.clear();
        for (int64_t b = 0; b < in.batch; ++b) last_.push_back(in.token_inputs[in.seq_starts[b + 1] - 1]);
        has_slots_ = in.lora_slots != nullptr;
        slots_.clear();
        if (in.lora_slots) slots_.assign(in.lora_slots, in.lora_slots + in.batch);
        return RC_SUCCESS;
    }
    RetCode Run(bool) override {
        logits_.assign((size_t)B_ * vocab_, 0.f);
        for (int64_t b = 0; b < B_; ++b) logits_[(size_t)b * vocab_ + last_[b]] = 1.f;
        std::cout << "{\"backend\":1,\"has_slots\":" << (has_slots_ ? 1 : 0) << ",\"lora_slots\":" << Arr(slots_) << ",\"last_tokens\":" << Arr(last_)
                  << "}" << std::endl;
        return RC_SUCCESS;
    }
    float* GetLogits(int64_t* stride) override {
        *stride = vocab_;
        return logits_.data();
    }

private:
    int vocab_;
    int64_t B_ = 0;
    bool has_slots_ = false;
    std::vector<int64_t> last_;
    std::vector<int32_t> slots_;
    std::vector<float> logits_;
};

class FakePostProcessor final : public PostProcessor {
public:
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float*, const int32_t*, const float*, int32_t batch, int32_t vocab, int32_t stride,
                           int32_t, float, bool, int32_t* out, float* lp, bool) override {
        for (int b = 0; b < batch; ++b) {
            int best = 0;
            for (int v = 1; v < vocab; ++v)
                if (logits[(size_t)b * stride + v] > logits[(size_t)b * stride + best]) best = v;
            out[b] = best;
            lp[b] = 0.f;
        }
        return RC_SUCCESS;
    }
    RetCode ApplyPenalty(const float*, const float*, const float*, const float*, const int64_t*, const int64_t*, const int64_t*,
                         const int64_t*, int32_t, int32_t, bool, float*) override {
        return RC_SUCCESS;
    }
};

class CountingConnection final : public Connection {
public:
    void OnProfiling(const std::shared_ptr<WorkerProfiler>&) override {}
    void OnTokenize(uint64_t, const std::vector<int>&) override {}
    void Send(const std::vector<Response>& rsps) override {
        std::lock_guard<std::mutex> g(mu_);
        for (const auto& r : rsps)
            if (r.finish_flag != FinishFlag::NOT_FINISHED) ++done_;
        cv_.notify_all();
    }
    void NotifyFailure(uint64_t id, RetCode rc, const std::string& msg) override {
        std::lock_guard<std::mutex> g(mu_);
        std::cout << "{\"failed\":" << id << ",\"rc\":" << (int)rc << ",\"msg\":\"" << msg << "\"}" << std::endl;
        ++done_;
        cv_.notify_all();
    }
    void WaitDone(size_t wanted) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return done_ >= wanted; });
    }
    std::mutex mu_;
    std::condition_variable cv_;
    size_t done_ = 0;
};

struct TraceCtx {
    std::string phase;
    AdapterRegistry* reg = nullptr;
    int retire_slot = -1;   // tries to unload this slot from inside a step (a request on it is running)
};

void Observe(void* arg, uint64_t step, const ModelInput& in, bool, bool hit) {
    auto* t = static_cast<TraceCtx*>(arg);
    std::cout << "{\"phase\":\"" << t->phase << "\",\"step\":" << step << ",\"prefix_hit\":" << (hit ? 1 : 0) << ",\"start_pos\":" << Arr(in.start_pos)
              << ",\"num_tokens\":" << in.token_inputs.size() << ",\"lora_slots\":" << Arr(in.lora_slots) << "}" << std::endl;
    if (t->retire_slot >= 0 && step == 1)
        std::cout << "{\"event\":\"unload_while_running\",\"slot\":" << t->retire_slot << ",\"rc\":" << t->reg->Retire(t->retire_slot) << "}"
                  << std::endl;
}

std::shared_ptr<Request> MakeRequest(uint64_t id, const std::vector<int>& tokens, int gen, int slot) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = gen;
    r->early_stopping = false;
    r->token_ids = std::make_shared<std::vector<int>>(tokens);
    r->lora_slot = slot;
    return r;
}

void WaitIdle(LLMGenerator& gen) {
    while (!gen.IsIdle()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
}

}  // namespace

int main() {
    ModelConfig mc;
    mc.hidden_dim = 64; mc.intermediate_dim = 64; mc.num_layers = 1; mc.num_heads = 2; mc.num_kv_heads = 2;
    mc.vocab_size = 1000;
    mc.cache_quant_bit = 8; mc.cache_quant_group = 8; mc.cache_layout = 3; mc.cache_mode = 1; mc.page_size = 4;
    GeneratorConfig gc;
    gc.top_k = 1;
    gc.max_running_batch = 4;
    gc.max_input_tokens_per_request = 4096; gc.max_output_tokens_per_request = 4096; gc.max_total_tokens_per_request = 8192;
    gc.max_tokens_per_step = 8192;
    gc.max_cooldown_request = 2;

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt(mc.vocab_size);
    FakePostProcessor pp;
    AdapterRegistry reg;
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.post_processor = &pp;
    res.device_worker_pool_ = &pool;
    res.adapters = &reg;

    const uint64_t uid0 = reg.Publish(0), uid1 = reg.Publish(1);
    std::cout << "{\"event\":\"loaded\",\"uids_differ\":" << (uid0 != uid1 && uid0 && uid1 ? 1 : 0) << "}" << std::endl;
    std::vector<int> prompt;
    for (int i = 0; i < 13; ++i) prompt.push_back(100 + i);   // three full pages of four tokens and one token more

    CountingConnection conn;
    TraceCtx t;
    t.reg = &reg;
    size_t want = 0;
    {   // ---- the prefix cache under adapters: one request at a time over the same tokens
        gc.enable_prefix_cache = true;
        gc.max_prefill_batch = 1;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, &t);
        if (gen.Init() != RC_SUCCESS) return 2;
        auto one = [&](const char* phase, uint64_t id, int slot, int gen_len) {
            t.phase = phase;
            gen.Process(MakeRequest(id, prompt, gen_len, slot));
            conn.WaitDone(++want);
            WaitIdle(gen);
        };
        one("base_first", 1, -1, 2);
        one("adapter0_first", 2, 0, 2);        // same tokens, another model: no hit
        one("adapter0_again", 3, 0, 2);        // same adapter: hit
        one("adapter1_first", 4, 1, 2);        // another adapter: no hit
        one("base_again", 5, -1, 2);           // the base model's pages are still there: hit
        // the slot is reloaded: a new uid, the pages of what it held before never hit
        std::cout << "{\"event\":\"unload_idle\",\"slot\":0,\"rc\":" << reg.Retire(0) << "}" << std::endl;
        const uint64_t uid0b = reg.Publish(0);
        std::cout << "{\"event\":\"reloaded\",\"uid_is_new\":" << (uid0b != uid0 && uid0b != uid1 && uid0b ? 1 : 0) << "}" << std::endl;
        one("adapter0_reloaded", 6, 0, 2);
        // a running request holds its slot
        t.retire_slot = 1;
        one("adapter1_running", 7, 1, 6);
        t.retire_slot = -1;
        std::cout << "{\"event\":\"unload_after\",\"slot\":1,\"rc\":" << reg.Retire(1) << "}" << std::endl;
        std::cout << "{\"event\":\"unload_twice\",\"slot\":1,\"rc\":" << reg.Retire(1) << "}" << std::endl;
        one("adapter1_unloaded", 8, 1, 2);     // fails: nothing is loaded in slot 1
        one("slot_out_of_range", 9, 64, 2);
    }
    {   // ---- batch order: admission, finish and reuse of batch rows
        gc.enable_prefix_cache = false;
        gc.max_prefill_batch = 4;
        reg.Publish(1);
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, &t);
        t.phase = "batch_order";
        // queued before the generator thread starts: the admission order is deterministic.  Six requests on four batch rows; request id
        // has slot id % 3 - 1 and runs id + 1 steps, so rows free up one by one and later requests move into them
        for (uint64_t id = 1; id <= 6; ++id) {
            std::vector<int> p = {7, 8, (int)(500 + id)};
            gen.Process(MakeRequest(id, p, (int)id + 1, (int)(id % 3) - 1));
        }
        want += 6;
        if (gen.Init() != RC_SUCCESS) return 2;
        conn.WaitDone(want);
        WaitIdle(gen);
        // every request gave its reference back: both slots unload
        std::cout << "{\"event\":\"unload_end\",\"slot\":0,\"rc\":" << reg.Retire(0) << "}" << std::endl;
        std::cout << "{\"event\":\"unload_end\",\"slot\":1,\"rc\":" << reg.Retire(1) << "}" << std::endl;
    }
    return 0;
}
