// Test driver for prompt logprobs on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   prompt_lp_trace  runs LLMGenerator + LLMEngine against a fake Runtime and a fake PostProcessor and prints one JSON line per step (what
//                    the generator packed), per backend call (what the backend received), per Response and per failure.
//                    tests/test_prompt_logprobs_host.py holds the expectations.
//
// The fake model repeats the last input token of every row, and every prompt ends in 500 + request id: the last token of a row names the
// request it belongs to at every step.  The fake SetPromptLogprobs lists the positions as the library does (rows s .. e-2 of every request
// with ask >= 0); the fake results name what they score: position at row r has logprob -token_inputs[r + 1], rank r - s, top tokens
// token_inputs[r + 1] + e and top logprobs -e in its first n slots, -7 / 7 behind them.
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

// a runtime from before prompt logprobs: SetPromptLogprobs / GetPromptLogprobs are the base class's (RC_UNSUPPORTED)
class OldRuntime : public Runtime {
public:
    explicit OldRuntime(int vocab) : vocab_(vocab) {}
    RetCode SetInputs(const StepInputs& in) override {
        B_ = in.batch;
        tok_.assign(in.token_inputs, in.token_inputs + in.num_tokens);
        seq_.assign(in.seq_starts, in.seq_starts + in.batch + 1);
        last_.clear();
        for (int64_t b = 0; b < in.batch; ++b) last_.push_back(in.token_inputs[in.seq_starts[b + 1] - 1]);
        Staged();
        return RC_SUCCESS;
    }
    RetCode Run(bool) override {
        logits_.assign((size_t)B_ * vocab_, 0.f);
        for (int64_t b = 0; b < B_; ++b) logits_[(size_t)b * vocab_ + last_[b]] = 1.f;
        Ran();
        return RC_SUCCESS;
    }
    float* GetLogits(int64_t* stride) override {
        *stride = vocab_;
        return logits_.data();
    }
    const std::vector<int64_t>& last() const { return last_; }

protected:
    virtual void Staged() {}
    virtual void Ran() {}
    int vocab_;
    int64_t B_ = 0;
    std::vector<int64_t> tok_, seq_, last_;
    std::vector<float> logits_;
};

class PromptRuntime final : public OldRuntime {
public:
    using OldRuntime::OldRuntime;
    RetCode SetPromptLogprobs(const int32_t* ask, int64_t batch) override {
        Line("{\"call\":\"SetPromptLogprobs\",\"batch\":" + std::to_string(batch) + ",\"ask\":" + Arr(ask, (size_t)batch) + ",\"seq_starts\":" + Arr(seq_) + "}");
        if (batch != B_) return RC_INVALID_VALUE;
        ask_.assign(ask, ask + batch);
        return RC_SUCCESS;
    }
    RetCode GetPromptLogprobs(PromptLogprobsView* out) override {
        Line("{\"call\":\"GetPromptLogprobs\",\"positions\":" + std::to_string(rows_.size()) + "}");
        out->positions = (int64_t)rows_.size();
        out->rows = rows_.data();
        out->logprobs = lp_.data();
        out->ranks = rank_.data();
        out->top_tokens = ttok_.data();
        out->top_logprobs = tlp_.data();
        return RC_SUCCESS;
    }

private:
    void Staged() override { ask_.clear(); }   // the ask belongs to one step
    void Ran() override {
        rows_.clear(); lp_.clear(); rank_.clear(); ttok_.clear(); tlp_.clear();
        for (size_t b = 0; b < ask_.size(); ++b) {
            if (ask_[b] < 0) continue;
            for (int64_t r = seq_[b]; r + 1 < seq_[b + 1]; ++r) {
                rows_.push_back((int32_t)r);
                lp_.push_back(-(float)tok_[r + 1]);
                rank_.push_back((int32_t)(r - seq_[b]));
                for (int e = 0; e < PostProcessor::kTopLogprobsMax; ++e) {
                    ttok_.push_back(e < ask_[b] ? (int32_t)tok_[r + 1] + e : -7);
                    tlp_.push_back(e < ask_[b] ? -(float)e : 7.f);
                }
            }
        }
    }
    std::vector<int32_t> ask_, rows_, rank_, ttok_;
    std::vector<float> lp_, tlp_;
};

class ArgMaxPostProcessor final : public PostProcessor {
public:
    explicit ArgMaxPostProcessor(const OldRuntime* const* rt) : rt_(rt) {}
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float*, const int32_t*, const float*, int32_t batch, int32_t vocab, int32_t stride, int32_t,
                           float, bool, int32_t* out, float* lp, bool) override {
        Line("{\"call\":\"SampleTopKTopP\",\"batch\":" + std::to_string(batch) + ",\"last_tokens\":" + Arr((*rt_)->last()) + "}");
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

private:
    const OldRuntime* const* rt_;
};

class PrintingConnection final : public Connection {
public:
    void OnProfiling(const std::shared_ptr<WorkerProfiler>&) override {}
    void OnTokenize(uint64_t, const std::vector<int>&) override {}
    void Send(const std::vector<Response>& rsps) override {
        std::lock_guard<std::mutex> g(mu_);
        for (const auto& r : rsps) {
            Line("{\"rsp\":" + std::to_string(r.id) + ",\"token\":" + std::to_string(r.token) + ",\"finished\":" +
                 (r.finish_flag != FinishFlag::NOT_FINISHED ? "1" : "0") + ",\"prompt_logprobs\":" + Arr(r.prompt_logprobs) + ",\"prompt_ranks\":" +
                 Arr(r.prompt_ranks) + ",\"prompt_top_tokens\":" + Arr(r.prompt_top_tokens) + ",\"prompt_top_logprobs\":" + Arr(r.prompt_top_logprobs) + "}");
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
         (hit ? "1" : "0") + ",\"start_pos\":" + Arr(in.start_pos) + ",\"seq_starts\":" + Arr(in.seq_starts) + ",\"token_inputs\":" + Arr(in.token_inputs) +
         ",\"prompt_logprobs_list\":" + Arr(in.prompt_logprobs_list) + "}");
}

std::shared_ptr<Request> MakeRequest(uint64_t id, const std::vector<int>& tokens, int gen, int prompt_logprobs) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = gen;
    r->early_stopping = false;
    r->token_ids = std::make_shared<std::vector<int>>(tokens);
    r->prompt_logprobs = prompt_logprobs;
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
    PromptRuntime new_rt(mc.vocab_size);
    OldRuntime old_rt(mc.vocab_size);
    const OldRuntime* cur = &new_rt;
    ArgMaxPostProcessor pp(&cur);
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.device_worker_pool_ = &pool;
    res.post_processor = &pp;

    PrintingConnection conn;
    size_t want = 0;
    // six requests on four batch rows, queued before the generator thread starts (the admission order is deterministic): request id has a
    // prompt of LEN[id] tokens (10 * id + 1, 10 * id + 2, .. and 500 + id last) and runs id + 1 steps, so rows free up one by one and
    // requests 5 and 6 are prefilled beside decode rows; ask[id] as the client sent it (25: clamped to 20, -5: to -1)
    static const int LEN[6] = {3, 4, 2, 3, 5, 1};
    auto batch_phase = [&](const char* phase, OldRuntime* rt, const int* ask) {
        cur = rt;
        res.items[0].runtime = rt;
        gc.enable_prefix_cache = false;
        gc.max_prefill_batch = 4;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = phase;
        for (uint64_t id = 1; id <= 6; ++id) {
            std::vector<int> p;
            for (int i = 1; i < LEN[id - 1]; ++i) p.push_back((int)(10 * id) + i);
            p.push_back((int)(500 + id));
            gen.Process(MakeRequest(id, p, (int)id + 1, ask[id - 1]));
        }
        want += 6;
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    const int mixed[6] = {-1, 0, 25, -5, 2, 0}, nobody[6] = {-1, -1, -1, -1, -1, -1}, one[6] = {-1, 1, -1, -1, -1, -1};
    if (!batch_phase("mixed", &new_rt, mixed)) return 2;
    {   // ---- the prefix cache: an asking request matches nothing and publishes; a request that does not ask hits what it published
        cur = &new_rt;
        res.items[0].runtime = &new_rt;
        gc.enable_prefix_cache = true;
        gc.max_prefill_batch = 1;
        std::vector<int> prompt;
        for (int i = 0; i < 12; ++i) prompt.push_back(100 + i);   // three full pages of four tokens ...
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        if (gen.Init() != RC_SUCCESS) return 2;
        static const char* names[4] = {"prefix_asking_cold", "prefix_plain_hit", "prefix_asking_again", "prefix_plain_again"};
        for (uint64_t id = 11; id <= 14; ++id) {
            g_phase = names[id - 11];
            std::vector<int> p = prompt;
            p.push_back((int)(500 + id));                         // ... and the token that names the request
            gen.Process(MakeRequest(id, p, 3, id % 2 ? 1 : -1));
            conn.WaitDone(++want);
            WaitIdle(gen);
        }
    }
    // ---- nobody asks: SetPromptLogprobs is never called
    if (!batch_phase("nobody", &new_rt, nobody)) return 2;
    // ---- a backend without prompt logprobs: the asking request fails alone ...
    if (!batch_phase("old_backend", &old_rt, one)) return 2;
    // ... and serves a workload in which nobody asks as before
    if (!batch_phase("old_backend_nobody", &old_rt, nobody)) return 2;
    return 0;
}
