// Test driver for the per-request sampler on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   sample_trace [sampling_seed]   runs LLMGenerator + LLMEngine against a fake Runtime and a fake PostProcessor and prints one JSON line
//                                  per step (what the generator packed) and per sampling call (what the backend received).
//                                  tests/test_sample_rows_host.py holds the expectations.
//
// The fake model repeats the last input token of every row, and every prompt ends in 500 + request id: the last token of a row names the
// request it belongs to at every step.
#include <stdlib.h>

#include <condition_variable>
#include <iostream>
#include <mutex>
#include <sstream>
#include <thread>

#include "common/config.h"
#include "common/request.h"
#include "common/resource.h"
#include "generator/llm_generator.h"

using namespace ppl::llm;
using namespace ppl::common;

namespace {

template <typename T>
std::string Arr(const T* v, size_t n) {
    std::ostringstream ss;
    ss << "[";
    for (size_t i = 0; i < n; ++i) ss << (i ? "," : "") << v[i];
    ss << "]";
    return ss.str();
}
template <typename T>
std::string Arr(const std::vector<T>& v) { return Arr(v.data(), v.size()); }

class FakeRuntime final : public Runtime {
public:
    explicit FakeRuntime(int vocab) : vocab_(vocab) {}
    RetCode SetInputs(const StepInputs& in) override {
        B_ = in.batch;
        last_.clear();
        for (int64_t b = 0; b < in.batch; ++b) last_.push_back(in.token_inputs[in.seq_starts[b + 1] - 1]);
        return RC_SUCCESS;
    }
    RetCode Run(bool) override {
        logits_.assign((size_t)B_ * vocab_, 0.f);
        for (int64_t b = 0; b < B_; ++b) logits_[(size_t)b * vocab_ + last_[b]] = 1.f;
        return RC_SUCCESS;
    }
    float* GetLogits(int64_t* stride) override {
        *stride = vocab_;
        return logits_.data();
    }
    const std::vector<int64_t>& last() const { return last_; }

private:
    int vocab_;
    int64_t B_ = 0;
    std::vector<int64_t> last_;
    std::vector<float> logits_;
};

void ArgMax(const float* logits, int32_t batch, int32_t vocab, int32_t stride, int32_t* out, float* lp) {
    for (int b = 0; b < batch; ++b) {
        int best = 0;
        for (int v = 1; v < vocab; ++v)
            if (logits[(size_t)b * stride + v] > logits[(size_t)b * stride + best]) best = v;
        out[b] = best;
        lp[b] = 0.f;
    }
}

// today's post processor: no SampleRows of its own (the base class answers RC_UNSUPPORTED)
class OldPostProcessor : public PostProcessor {
public:
    explicit OldPostProcessor(const FakeRuntime* rt) : rt_(rt) {}
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float* temps, const int32_t* top_k, const float* top_p, int32_t batch, int32_t vocab,
                           int32_t stride, int32_t default_top_k, float default_top_p, bool changed, int32_t* out, float* lp,
                           bool enable_penalty) override {
        std::cout << "{\"call\":\"SampleTopKTopP\",\"batch\":" << batch << ",\"vocab\":" << vocab << ",\"stride\":" << stride
                  << ",\"default_top_k\":" << default_top_k << ",\"default_top_p\":" << default_top_p << ",\"req_list_changed\":" << (changed ? 1 : 0)
                  << ",\"enable_penalty\":" << (enable_penalty ? 1 : 0) << ",\"temperatures\":" << Arr(temps, batch) << ",\"top_k\":" << Arr(top_k, batch)
                  << ",\"top_p\":" << Arr(top_p, batch) << ",\"last_tokens\":" << Arr(rt_->last()) << "}" << std::endl;
        ArgMax(logits, batch, vocab, stride, out, lp);
        return RC_SUCCESS;
    }
    RetCode ApplyPenalty(const float*, const float*, const float*, const float*, const int64_t*, const int64_t*, const int64_t*,
                         const int64_t*, int32_t, int32_t, bool, float*) override {
        return RC_SUCCESS;
    }

protected:
    const FakeRuntime* rt_;
};

class RowsPostProcessor final : public OldPostProcessor {
public:
    using OldPostProcessor::OldPostProcessor;
    RetCode SampleRows(const float* logits, const float* temps, const int32_t* top_k, const float* top_p, const uint64_t* seeds,
                       const uint64_t* draws, int32_t batch, int32_t vocab, int32_t stride, int32_t* out, float* lp) override {
        if (batch == 0) return RC_SUCCESS;
        std::cout << "{\"call\":\"SampleRows\",\"batch\":" << batch << ",\"vocab\":" << vocab << ",\"stride\":" << stride << ",\"temps_null\":"
                  << (temps ? 0 : 1) << ",\"temperatures\":" << (temps ? Arr(temps, batch) : "[]") << ",\"top_k\":" << Arr(top_k, batch)
                  << ",\"top_p\":" << Arr(top_p, batch) << ",\"seeds\":" << Arr(seeds, batch) << ",\"draws\":" << Arr(draws, batch)
                  << ",\"last_tokens\":" << Arr(rt_->last()) << "}" << std::endl;
        ArgMax(logits, batch, vocab, stride, out, lp);
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

std::string g_phase;

void Observe(void*, uint64_t step, const ModelInput& in, bool changed, bool hit) {
    std::cout << "{\"phase\":\"" << g_phase << "\",\"step\":" << step << ",\"req_list_changed\":" << (changed ? 1 : 0) << ",\"prefix_hit\":" << (hit ? 1 : 0)
              << ",\"start_pos\":" << Arr(in.start_pos) << ",\"top_k_list\":" << Arr(in.top_k_list) << ",\"seed_list\":" << Arr(in.seed_list)
              << ",\"draw_list\":" << Arr(in.draw_list) << "}" << std::endl;
}

std::shared_ptr<Request> MakeRequest(uint64_t id, const std::vector<int>& tokens, int gen, uint64_t seed, int top_k) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = gen;
    r->early_stopping = false;
    r->token_ids = std::make_shared<std::vector<int>>(tokens);
    r->seed = seed;
    r->top_k = top_k;
    r->top_p = 0.5f + 0.01f * (float)id;
    r->temperature = 1.f + 0.25f * (float)id;
    return r;
}

void WaitIdle(LLMGenerator& gen) {
    while (!gen.IsIdle()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
}

}  // namespace

int main(int argc, char** argv) {
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
    gc.sampling_seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 42;

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt(mc.vocab_size);
    RowsPostProcessor rows_pp(&rt);
    OldPostProcessor old_pp(&rt);
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.post_processor = &rows_pp;
    res.device_worker_pool_ = &pool;

    CountingConnection conn;
    size_t want = 0;
    // six requests on four batch rows, queued before the generator thread starts (the admission order is deterministic): request id runs
    // id + 1 steps, so rows free up one by one and later requests move into them; the even ids bring seed 1000 + id, the odd ones none;
    // top_k is 1 for ids 2 and 5
    auto batch_phase = [&](const char* phase, bool per_request) {
        gc.per_request_sampling = per_request;
        gc.enable_prefix_cache = false;
        gc.max_prefill_batch = 4;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = phase;
        for (uint64_t id = 1; id <= 6; ++id) {
            std::vector<int> p = {7, 8, (int)(500 + id)};
            gen.Process(MakeRequest(id, p, (int)id + 1, id % 2 ? 0 : 1000 + id, id == 2 || id == 5 ? 1 : (int)(10 * id)));
        }
        want += 6;
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    if (!batch_phase("rows_batch_order", true)) return 2;
    {   // ---- a request admitted on a prefix-cache hit starts its draws at 0 like any other
        gc.per_request_sampling = true;
        gc.enable_prefix_cache = true;
        gc.max_prefill_batch = 1;
        std::vector<int> prompt;
        for (int i = 0; i < 12; ++i) prompt.push_back(100 + i);   // three full pages of four tokens ...
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        if (gen.Init() != RC_SUCCESS) return 2;
        for (uint64_t id = 11; id <= 12; ++id) {
            g_phase = id == 11 ? "rows_prefix_cold" : "rows_prefix_hit";
            std::vector<int> p = prompt;
            p.push_back((int)(500 + id));                         // ... and the token that names the request
            gen.Process(MakeRequest(id, p, 3, id == 11 ? 77 : 0, 40));
            conn.WaitDone(++want);
            WaitIdle(gen);
        }
    }
    // ---- the switch off: today's call with today's arguments, SampleRows never
    if (!batch_phase("uniform_batch_order", false)) return 2;
    {   // ---- the switch on over a backend without SampleRows: Init fails
        gc.per_request_sampling = true;
        res.post_processor = &old_pp;
        LLMGenerator gen(res, gc, mc, &conn);
        const RetCode rc = gen.Init();
        std::cout << "{\"event\":\"init_without_sample_rows\",\"ok\":" << (rc == RC_SUCCESS ? 1 : 0) << ",\"unsupported\":" << (rc == RC_UNSUPPORTED ? 1 : 0)
                  << "}" << std::endl;
        gc.per_request_sampling = false;
        LLMGenerator gen2(res, gc, mc, &conn);
        std::cout << "{\"event\":\"init_switch_off\",\"ok\":" << (gen2.Init() == RC_SUCCESS ? 1 : 0) << "}" << std::endl;
    }
    return 0;
}
