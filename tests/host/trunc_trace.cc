// Test driver for min_p / typical_p on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   trunc_trace   runs LLMGenerator + LLMEngine against a fake Runtime and fake PostProcessors and prints one JSON line per step (what the
//                 generator packed), per sampling call (what the backend received), per finished and per failed request, and one at
//                 the beginning of each phase.
//                 tests/test_sample_trunc_host.py holds the expectations.
//
// The fake model repeats the last input token of every row, and every prompt ends in 500 + request id: the last token of a row names the
// request it belongs to at every step.  Request id runs id + 1 steps; ids 2 and 4 set min_p = id / 100, ids 3 and 4 typical_p = 0.5 + id / 20;
// id 5 is greedy (top_k 1), the others have top_k 10 * id.
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

// one line of the trace, written whole: the responses come from another thread than the steps
struct Line {
    std::ostringstream ss;
    template <typename T>
    Line& operator<<(const T& v) { ss << v; return *this; }
};
void Emit(Line& l) {
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    std::cout << l.ss.str() << std::endl;
}

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

// a backend with the per-request sampler and nothing more: SampleRowsTrunc is the base class's RC_UNSUPPORTED
class RowsPostProcessor : public PostProcessor {
public:
    explicit RowsPostProcessor(const FakeRuntime* rt) : rt_(rt) {}
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float*, const int32_t*, const float*, int32_t batch, int32_t vocab, int32_t stride, int32_t,
                           float, bool, int32_t* out, float* lp, bool) override {
        Emit(Line() << "{\"call\":\"SampleTopKTopP\",\"batch\":" << batch << ",\"last_tokens\":" << Arr(rt_->last()) << "}");
        ArgMax(logits, batch, vocab, stride, out, lp);
        return RC_SUCCESS;
    }
    RetCode ApplyPenalty(const float*, const float*, const float*, const float*, const int64_t*, const int64_t*, const int64_t*,
                         const int64_t*, int32_t, int32_t, bool, float*) override {
        return RC_SUCCESS;
    }
    RetCode SampleRows(const float* logits, const float*, const int32_t* top_k, const float*, const uint64_t*, const uint64_t*, int32_t batch,
                       int32_t vocab, int32_t stride, int32_t* out, float* lp) override {
        if (batch == 0) return RC_SUCCESS;
        Emit(Line() << "{\"call\":\"SampleRows\",\"batch\":" << batch << ",\"top_k\":" << Arr(top_k, batch) << ",\"last_tokens\":" << Arr(rt_->last())
                  << "}");
        ArgMax(logits, batch, vocab, stride, out, lp);
        return RC_SUCCESS;
    }

protected:
    const FakeRuntime* rt_;
};

class TruncPostProcessor final : public RowsPostProcessor {
public:
    using RowsPostProcessor::RowsPostProcessor;
    RetCode SampleRowsTrunc(const float* logits, const float* temps, const int32_t* top_k, const float* top_p, const float* min_p,
                            const float* typical_p, const uint64_t* seeds, const uint64_t* draws, int32_t batch, int32_t vocab, int32_t stride,
                            int32_t* out, float* lp) override {
        if (batch == 0) return RC_SUCCESS;
        Emit(Line() << "{\"call\":\"SampleRowsTrunc\",\"batch\":" << batch << ",\"vocab\":" << vocab << ",\"stride\":" << stride << ",\"temps_null\":"
                  << (temps ? 0 : 1) << ",\"top_k\":" << Arr(top_k, batch) << ",\"top_p\":" << Arr(top_p, batch) << ",\"min_p\":" << Arr(min_p, batch)
                  << ",\"typical_p\":" << Arr(typical_p, batch) << ",\"seeds\":" << Arr(seeds, batch) << ",\"draws\":" << Arr(draws, batch)
                  << ",\"last_tokens\":" << Arr(rt_->last()) << "}");
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
            if (r.finish_flag != FinishFlag::NOT_FINISHED) {
                Emit(Line() << "{\"finished\":" << r.id << "}");
                ++done_;
            }
        cv_.notify_all();
    }
    void NotifyFailure(uint64_t id, RetCode rc, const std::string& msg) override {
        std::lock_guard<std::mutex> g(mu_);
        Emit(Line() << "{\"failed\":" << id << ",\"unsupported\":" << (rc == RC_UNSUPPORTED ? 1 : 0) << ",\"msg\":\"" << msg << "\"}");
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

void Observe(void*, uint64_t step, const ModelInput& in, bool changed, bool) {
    Emit(Line() << "{\"phase\":\"" << g_phase << "\",\"step\":" << step << ",\"req_list_changed\":" << (changed ? 1 : 0) << ",\"top_k_list\":"
              << Arr(in.top_k_list) << ",\"min_p_list\":" << Arr(in.min_p_list) << ",\"typical_p_list\":" << Arr(in.typical_p_list) << "}");
}

std::shared_ptr<Request> MakeRequest(uint64_t id) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = (int)id + 1;
    r->early_stopping = false;
    r->token_ids = std::make_shared<std::vector<int>>(std::vector<int>{7, 8, (int)(500 + id)});
    r->seed = 1000 + id;
    r->top_k = id == 5 ? 1 : (int)(10 * id);
    r->top_p = 0.5f + 0.01f * (float)id;
    if (id == 2 || id == 4) r->min_p = 0.01f * (float)id;
    if (id == 3 || id == 4) r->typical_p = 0.5f + 0.05f * (float)id;
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
    gc.sampling_seed = 42;
    gc.enable_prefix_cache = false;
    gc.max_prefill_batch = 4;

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt(mc.vocab_size);
    TruncPostProcessor trunc_pp(&rt);
    RowsPostProcessor rows_pp(&rt);
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.device_worker_pool_ = &pool;

    CountingConnection conn;
    size_t want = 0;
    // six requests on four batch rows, queued before the generator thread starts (the admission order is deterministic): rows free up one
    // by one and later requests move into them
    auto phase = [&](const char* name, bool per_request, PostProcessor* pp) {
        gc.per_request_sampling = per_request;
        res.post_processor = pp;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = name;
        Emit(Line() << "{\"begin\":\"" << name << "\"}");   // (a request can fail at admission, in front of the phase's first step)
        for (uint64_t id = 1; id <= 6; ++id) gen.Process(MakeRequest(id));
        want += 6;
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    if (!phase("trunc", true, &trunc_pp)) return 2;
    if (!phase("switch_off", false, &trunc_pp)) return 2;
    if (!phase("no_backend", true, &rows_pp)) return 2;
    return 0;
}
