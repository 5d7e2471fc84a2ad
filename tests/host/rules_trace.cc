// Test driver for logit rules on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   rules_trace   runs LLMGenerator + LLMEngine against a fake Runtime and fake PostProcessors and prints one JSON line per step (what the
//                 generator packed), per post-processor call (what the backend received), per Response and per failure.
//                 tests/test_logit_rules_host.py holds the expectations.
//
// The fake model repeats the last input token of every row, and every prompt ends in 500 + request id: the last token of a row names the
// request it belongs to at every step.  The fake backend records the rules and the edits it is handed and changes no logit, so every
// request keeps answering 500 + id.
#include <math.h>
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

// bias values as JSON: -inf goes out as the string "-inf"
std::string Values(const std::vector<float>& v) {
    std::ostringstream ss;
    ss << "[";
    for (size_t i = 0; i < v.size(); ++i) {
        ss << (i ? "," : "");
        if (v[i] == -INFINITY) ss << "\"-inf\"";
        else ss << v[i];
    }
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

// a backend from before logit rules: the sampler and the penalty, no SetLogitRule / EditLogits of its own (RC_UNSUPPORTED)
class OldPostProcessor : public PostProcessor {
public:
    explicit OldPostProcessor(const FakeRuntime* rt) : rt_(rt) {}
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float*, const int32_t*, const float*, int32_t batch, int32_t vocab, int32_t stride, int32_t,
                           float, bool, int32_t* out, float* lp, bool) override {
        Line("{\"call\":\"SampleTopKTopP\",\"batch\":" + std::to_string(batch) + ",\"last_tokens\":" + Arr(rt_->last()) + "}");
        for (int b = 0; b < batch; ++b) {
            int best = 0;
            for (int v = 1; v < vocab; ++v)
                if (logits[(size_t)b * stride + v] > logits[(size_t)b * stride + best]) best = v;
            out[b] = best;
            lp[b] = 0.f;
        }
        return RC_SUCCESS;
    }
    RetCode ApplyPenalty(const float*, const float*, const float*, const float*, const int64_t* slots, const int64_t*, const int64_t*,
                         const int64_t*, int32_t batch, int32_t, bool, float*) override {
        Line("{\"call\":\"ApplyPenalty\",\"batch\":" + std::to_string(batch) + ",\"slots\":" + Arr(slots, batch) + "}");
        return RC_SUCCESS;
    }

protected:
    const FakeRuntime* rt_;
};

class RulesPostProcessor final : public OldPostProcessor {
public:
    using OldPostProcessor::OldPostProcessor;
    RetCode SetLogitRule(int64_t slot, const LogitRule& r) override {
        std::vector<int32_t> allowed;
        for (size_t w = 0; w < r.allowed_bits.size(); ++w)
            for (int b = 0; b < 32; ++b)
                if ((r.allowed_bits[w] >> b) & 1u) allowed.push_back((int32_t)(w * 32 + b));
        Line("{\"call\":\"SetLogitRule\",\"slot\":" + std::to_string(slot) + ",\"bias_tokens\":" + Arr(r.bias_tokens) + ",\"bias_values\":" +
             Values(r.bias_values) + ",\"has_mask\":" + (r.has_mask ? "1" : "0") + ",\"mask_words\":" + std::to_string(r.allowed_bits.size()) +
             ",\"allowed\":" + Arr(allowed) + ",\"stops\":" + Arr(r.stop_tokens) + "}");
        return RC_SUCCESS;
    }
    RetCode EditLogits(float* logits, const int64_t* slots, const uint32_t* flags, int32_t batch, int32_t vocab, int32_t stride) override {
        if (batch == 0) return RC_SUCCESS;
        Line("{\"call\":\"EditLogits\",\"batch\":" + std::to_string(batch) + ",\"vocab\":" + std::to_string(vocab) + ",\"stride\":" +
             std::to_string(stride) + ",\"logits_null\":" + (logits ? "0" : "1") + ",\"slots\":" + Arr(slots, batch) + ",\"flags\":" +
             Arr(flags, batch) + ",\"last_tokens\":" + Arr(rt_->last()) + "}");
        return RC_SUCCESS;
    }
};

class PrintingConnection final : public Connection {
public:
    void OnProfiling(const std::shared_ptr<WorkerProfiler>&) override {}
    void OnTokenize(uint64_t, const std::vector<int>&) override {}
    void Send(const std::vector<Response>& rsps) override {
        std::lock_guard<std::mutex> g(mu_);
        for (const auto& r : rsps) {
            Line("{\"rsp\":" + std::to_string(r.id) + ",\"token\":" + std::to_string(r.token) + ",\"finished\":" +
                 (r.finish_flag != FinishFlag::NOT_FINISHED ? "1" : "0") + "}");
            if (r.finish_flag != FinishFlag::NOT_FINISHED) ++done_;
        }
        cv_.notify_all();
    }
    void NotifyFailure(uint64_t id, RetCode rc, const std::string& msg) override {
        std::lock_guard<std::mutex> g(mu_);
        Line("{\"failed\":" + std::to_string(id) + ",\"code\":\"" + (rc == RC_UNSUPPORTED ? "unsupported" : rc == RC_INVALID_VALUE ? "invalid" : "other") +
             "\",\"msg\":\"" + msg + "\"}");
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
    std::vector<int64_t> last;
    for (size_t b = 0; b + 1 < in.seq_starts.size(); ++b) last.push_back(in.token_inputs[in.seq_starts[b + 1] - 1]);
    Line("{\"phase\":\"" + g_phase + "\",\"step\":" + std::to_string(step) + ",\"req_list_changed\":" + (changed ? "1" : "0") + ",\"last_tokens\":" +
         Arr(last) + ",\"batch_slots\":" + Arr(in.batch_slots) + ",\"logit_flags\":" + Arr(in.logit_flags) + "}");
}

std::shared_ptr<Request> MakeRequest(uint64_t id, int gen) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = gen;
    r->early_stopping = false;
    r->token_ids = std::make_shared<std::vector<int>>(std::vector<int>{7, 8, (int)(500 + id)});
    return r;
}

// the rules of the valid workload: request id runs id + 1 steps.  1, 4 and 6 carry none
void ValidRule(Request* r) {
    switch (r->id) {
        case 2:   // a bias and a ban, and a bias that the ban overrides
            r->logit_bias = {{10, 1.5f}, {12, 2.f}};
            r->banned_tokens = {11, 12};
            break;
        case 3:   // min_new_tokens alone: the generator's stop 901 and the request's own 900
            r->min_new_tokens = 2;
            r->stop_tokens = std::make_shared<std::unordered_set<int>>(std::unordered_set<int>{900});
            break;
        case 5:   // a mask, a ban by -inf bias, and a min_new_tokens longer than the request lives
            r->allowed_tokens = std::make_shared<std::vector<int32_t>>(std::vector<int32_t>{505, 5, 999, 33});
            r->logit_bias = {{33, -INFINITY}};
            r->min_new_tokens = 10;
            break;
        default: break;
    }
}

// one invalid rule per request id 1 .. 8; 9 and 10 are fine (10 carries a valid rule)
void InvalidRule(Request* r) {
    switch (r->id) {
        case 1: r->logit_bias = {{1000, 1.f}}; break;                               // token out of range (vocab 1000)
        case 2: r->logit_bias = {{3, NAN}}; break;
        case 3: r->logit_bias = {{3, INFINITY}}; break;
        case 4: r->logit_bias = {{3, 1.f}, {4, 1.f}, {3, 2.f}}; break;              // two finite values for one token
        case 5: for (int t = 0; t < 513; ++t) r->banned_tokens.push_back(t); break;
        case 6:
            r->min_new_tokens = 1;
            r->stop_tokens = std::make_shared<std::unordered_set<int>>();
            for (int t = 0; t < 64; ++t) r->stop_tokens->insert(t);                 // + the generator's 901: 65
            break;
        case 7:   // nothing left alive on the first step
            r->allowed_tokens = std::make_shared<std::vector<int32_t>>(std::vector<int32_t>{20, 21, 901});
            r->banned_tokens = {20};
            r->logit_bias = {{21, -INFINITY}};
            r->min_new_tokens = 1;
            break;
        case 8: r->allowed_tokens = std::make_shared<std::vector<int32_t>>(std::vector<int32_t>{-1}); break;
        case 10:  // exactly one live token, 512 entries, 64 stops: the boundary that passes
            r->allowed_tokens = std::make_shared<std::vector<int32_t>>(std::vector<int32_t>{700, 901, 0});
            for (int t = 0; t < 512; ++t) r->banned_tokens.push_back(t);
            r->min_new_tokens = 1;
            r->stop_tokens = std::make_shared<std::unordered_set<int>>();
            for (int t = 600; t < 663; ++t) r->stop_tokens->insert(t);
            break;
        default: break;
    }
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
    gc.stop_tokens = {901};
    gc.enable_prefix_cache = false;
    gc.max_prefill_batch = 4;

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt(mc.vocab_size);
    RulesPostProcessor rules_pp(&rt);
    OldPostProcessor old_pp(&rt);
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.device_worker_pool_ = &pool;

    PrintingConnection conn;
    size_t want = 0;
    // n requests on four batch rows, queued before the generator thread starts (the admission order is deterministic): request id runs
    // id + 1 steps, so rows and slots free up one by one and later requests move into them
    auto batch_phase = [&](const char* phase, PostProcessor* pp, bool penalty, int n, void (*rule)(Request*)) {
        res.post_processor = pp;
        gc.enable_penalty = penalty;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = phase;
        Line(std::string("{\"begin\":\"") + phase + "\"}");   // (uploads and admission failures come in front of a phase's first step record)
        for (uint64_t id = 1; id <= (uint64_t)n; ++id) {
            auto r = MakeRequest(id, (int)id + 1);
            if (rule) rule(r.get());
            gen.Process(r);
        }
        want += n;
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    if (!batch_phase("rules_penalty", &rules_pp, true, 6, ValidRule)) return 2;
    if (!batch_phase("rules_plain", &rules_pp, false, 6, ValidRule)) return 2;
    if (!batch_phase("invalid", &rules_pp, true, 10, InvalidRule)) return 2;
    if (!batch_phase("old_backend", &old_pp, true, 6, ValidRule)) return 2;
    if (!batch_phase("nobody", &rules_pp, true, 6, nullptr)) return 2;
    if (!batch_phase("old_backend_nobody", &old_pp, true, 6, nullptr)) return 2;
    if (!batch_phase("nobody_plain", &rules_pp, false, 6, nullptr)) return 2;
    if (!batch_phase("old_backend_nobody_plain", &old_pp, false, 6, nullptr)) return 2;
    return 0;
}
