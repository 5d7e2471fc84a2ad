// Test driver for top-N logprobs on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   logprobs_trace   runs LLMGenerator + LLMEngine against a fake Runtime and fake PostProcessors and prints one JSON line per step (what
//                    the generator packed), per post-processor call (what the backend received), per Response and per failure.
//                    tests/test_top_logprobs_host.py holds the expectations.
//
// The fake model repeats the last input token of every row, and every prompt ends in 500 + request id: the last token of a row names the
// request it belongs to at every step.  The fake TopLogprobs answers row j with tokens last, last + 1, ... and logprobs 0, -1, ...; it
// knows 18 entries per row (the rest is token -1, as behind a vocabulary of 18) and leaves -7 in the slots behind a row's n.
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

std::mutex g_out;
void Line(const std::string& s) {
    std::lock_guard<std::mutex> g(g_out);
    std::cout << s << std::endl;
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

// a backend from before top-N logprobs: both samplers, no TopLogprobs of its own (the base class answers RC_UNSUPPORTED)
class OldPostProcessor : public PostProcessor {
public:
    explicit OldPostProcessor(const FakeRuntime* rt) : rt_(rt) {}
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float*, const int32_t*, const float*, int32_t batch, int32_t vocab, int32_t stride, int32_t,
                           float, bool, int32_t* out, float* lp, bool) override {
        Line("{\"call\":\"SampleTopKTopP\",\"batch\":" + std::to_string(batch) + ",\"last_tokens\":" + Arr(rt_->last()) + "}");
        ArgMax(logits, batch, vocab, stride, out, lp);
        return RC_SUCCESS;
    }
    RetCode ApplyPenalty(const float*, const float*, const float*, const float*, const int64_t*, const int64_t*, const int64_t*,
                         const int64_t*, int32_t, int32_t, bool, float*) override {
        return RC_SUCCESS;
    }
    RetCode SampleRows(const float* logits, const float*, const int32_t*, const float*, const uint64_t*, const uint64_t*, int32_t batch,
                       int32_t vocab, int32_t stride, int32_t* out, float* lp) override {
        if (batch == 0) return RC_SUCCESS;
        Line("{\"call\":\"SampleRows\",\"batch\":" + std::to_string(batch) + ",\"last_tokens\":" + Arr(rt_->last()) + "}");
        ArgMax(logits, batch, vocab, stride, out, lp);
        return RC_SUCCESS;
    }

protected:
    const FakeRuntime* rt_;
};

class TopPostProcessor final : public OldPostProcessor {
public:
    using OldPostProcessor::OldPostProcessor;
    RetCode TopLogprobs(const float*, const float* temps, const int32_t* nlp, int32_t batch, int32_t vocab, int32_t stride, const int32_t** tokens,
                        const float** logprobs, int32_t* rows) override {
        Line("{\"call\":\"TopLogprobs\",\"batch\":" + std::to_string(batch) + ",\"vocab\":" + std::to_string(vocab) + ",\"stride\":" +
             std::to_string(stride) + ",\"temps_null\":" + (temps ? "0" : "1") + ",\"num_logprobs\":" + Arr(nlp, batch) + ",\"last_tokens\":" +
             Arr(rt_->last()) + "}");
        tok_.clear();
        lp_.clear();
        int32_t asked = 0;
        for (int b = 0; b < batch; ++b) {
            if (nlp[b] <= 0) continue;
            for (int e = 0; e < kTopLogprobsMax; ++e) {
                tok_.push_back(e >= nlp[b] ? -7 : (e < 18 ? (int32_t)rt_->last()[b] + e : -1));
                lp_.push_back(e >= nlp[b] ? 7.f : -(float)e);
            }
            ++asked;
        }
        *tokens = tok_.data();
        *logprobs = lp_.data();
        *rows = asked;
        return RC_SUCCESS;
    }

private:
    std::vector<int32_t> tok_;
    std::vector<float> lp_;
};

class PrintingConnection final : public Connection {
public:
    void OnProfiling(const std::shared_ptr<WorkerProfiler>&) override {}
    void OnTokenize(uint64_t, const std::vector<int>&) override {}
    void Send(const std::vector<Response>& rsps) override {
        std::lock_guard<std::mutex> g(mu_);
        for (const auto& r : rsps) {
            Line("{\"rsp\":" + std::to_string(r.id) + ",\"token\":" + std::to_string(r.token) + ",\"finished\":" +
                 (r.finish_flag != FinishFlag::NOT_FINISHED ? "1" : "0") + ",\"top_tokens\":" + Arr(r.top_tokens) + ",\"top_logprobs\":" +
                 Arr(r.top_logprobs) + "}");
            if (r.finish_flag != FinishFlag::NOT_FINISHED) ++done_;
        }
        cv_.notify_all();
    }
    void NotifyFailure(uint64_t id, RetCode rc, const std::string& msg) override {
        std::lock_guard<std::mutex> g(mu_);
        Line("{\"failed\":" + std::to_string(id) + ",\"unsupported\":" + (rc == RC_UNSUPPORTED ? "1" : "0") + ",\"msg\":\"" + msg + "\"}");
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
    Line("{\"phase\":\"" + g_phase + "\",\"step\":" + std::to_string(step) + ",\"req_list_changed\":" + (changed ? "1" : "0") + ",\"prefix_hit\":" +
         (hit ? "1" : "0") + ",\"start_pos\":" + Arr(in.start_pos) + ",\"num_logprobs_list\":" + Arr(in.num_logprobs_list) + "}");
}

std::shared_ptr<Request> MakeRequest(uint64_t id, const std::vector<int>& tokens, int gen, int num_logprobs) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = gen;
    r->early_stopping = false;
    r->token_ids = std::make_shared<std::vector<int>>(tokens);
    r->num_logprobs = num_logprobs;
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

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt(mc.vocab_size);
    TopPostProcessor top_pp(&rt);
    OldPostProcessor old_pp(&rt);
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.device_worker_pool_ = &pool;

    PrintingConnection conn;
    size_t want = 0;
    // six requests on four batch rows, queued before the generator thread starts (the admission order is deterministic): request id runs
    // id + 1 steps, so rows free up one by one and later requests move into them; num_logprobs[id] as given (25: clamped to 20, -2: to 0)
    auto batch_phase = [&](const char* phase, PostProcessor* pp, bool per_request, const int* nlp) {
        res.post_processor = pp;
        gc.per_request_sampling = per_request;
        gc.enable_prefix_cache = false;
        gc.max_prefill_batch = 4;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = phase;
        for (uint64_t id = 1; id <= 6; ++id) {
            std::vector<int> p = {7, 8, (int)(500 + id)};
            gen.Process(MakeRequest(id, p, (int)id + 1, nlp[id - 1]));
        }
        want += 6;
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    const int mixed[6] = {0, 3, 25, -2, 1, 5}, nobody[6] = {0, 0, 0, 0, 0, 0}, one[6] = {0, 2, 0, 0, 0, 0};
    if (!batch_phase("rows_mixed", &top_pp, true, mixed)) return 2;
    if (!batch_phase("uniform_mixed", &top_pp, false, mixed)) return 2;
    {   // ---- a request admitted on a prefix-cache hit keeps its own count
        res.post_processor = &top_pp;
        gc.per_request_sampling = true;
        gc.enable_prefix_cache = true;
        gc.max_prefill_batch = 1;
        std::vector<int> prompt;
        for (int i = 0; i < 12; ++i) prompt.push_back(100 + i);   // three full pages of four tokens ...
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        if (gen.Init() != RC_SUCCESS) return 2;
        for (uint64_t id = 11; id <= 12; ++id) {
            g_phase = id == 11 ? "prefix_cold" : "prefix_hit";
            std::vector<int> p = prompt;
            p.push_back((int)(500 + id));                         // ... and the token that names the request
            gen.Process(MakeRequest(id, p, 3, id == 11 ? 2 : 4));
            conn.WaitDone(++want);
            WaitIdle(gen);
        }
    }
    // ---- nobody asks: TopLogprobs is never called
    if (!batch_phase("nobody", &top_pp, true, nobody)) return 2;
    // ---- a backend without TopLogprobs: the asking request fails alone, under either sampler
    if (!batch_phase("old_backend_rows", &old_pp, true, one)) return 2;
    if (!batch_phase("old_backend_uniform", &old_pp, false, one)) return 2;
    // ... and serves a workload in which nobody asks as before
    if (!batch_phase("old_backend_nobody", &old_pp, false, nobody)) return 2;
    return 0;
}
