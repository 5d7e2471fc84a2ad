// Test driver for the per-request features TOGETHER on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   chain_trace   runs LLMGenerator + LLMEngine against a fake Runtime, a fake tokenizer and a fake PostProcessor and prints one JSON line
//                 per step (every per-row list of ModelInput), per backend call (what the backend received), per Response and per failure.
//                 tests/test_chain_host.py holds the expectations.
//
// Twelve requests go through four batch rows, two prefills per step, with mixed generation lengths: rows leave from the front, the middle
// and the end of the batch while others join.  The fake model repeats the last input token of every row, and every prompt ends in
// 500 + request id: the last token of a row names the request it belongs to at every step, and everything a request carries is a function
// of its id (Spec below; tests/test_chain_host.py restates it).  The fake results name what they answer: the top-N entry e of request id
// at engine step s is token id * 10000 + s * 100 + e with logprob -e; the prompt position at input row r has logprob -token_inputs[r + 1]
// (a prompt token is 10 * id + i), rank r - s and top tokens token_inputs[r + 1] + e.  The fake edits change no logit.
//
// Request 9 carries a rule the generator refuses when it admits it; request 6 carries a rule the backend cannot take (a bias on token
// 999: SetLogitRule fails), so it fails on its first step -- beside request 7, which asks for top-N and prompt logprobs behind it.  In the
// second phase the backend has no TopLogprobs: every request that asks for top-N fails on its first step, and the order of the requests
// puts the two that are served (5 and 10) behind a failing neighbour each on the step that scores their prompts.
#include <math.h>
#include <stdlib.h>

#include <condition_variable>
#include <iostream>
#include <mutex>
#include <sstream>
#include <thread>

#include "common/adapter_registry.h"
#include "common/config.h"
#include "common/guide.h"
#include "common/request.h"
#include "common/resource.h"
#include "generator/llm_generator.h"
#include "tokenizer/tokenizer.h"

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

const int kVocab = 1000, kEos = 2, kRequests = 12;
const int kGen[kRequests + 1] = {0, 3, 1, 5, 2, 4, 3, 6, 2, 3, 2, 4, 3};

// token 500 + i (i = 1 .. 25) is the one letter 'a' + i -- request i's own token is its own letter --, everything else is empty
class FakeTokenizer final : public Tokenizer {
public:
    void Encode(const char*, uint32_t, std::vector<int>*) const override {}
    void Decode(int*, uint32_t, std::string*) const override {}
    int GetBosId() const override { return 1; }
    int GetEosId() const override { return kEos; }
    bool TokenBytes(int id, std::string* b) const override {
        b->clear();
        if (id > 500 && id <= 525) b->push_back((char)('a' + id - 500));
        return true;
    }
};

class FakeRuntime final : public Runtime {
public:
    RetCode SetInputs(const StepInputs& in) override {
        B_ = in.batch;
        tok_.assign(in.token_inputs, in.token_inputs + in.num_tokens);
        seq_.assign(in.seq_starts, in.seq_starts + in.batch + 1);
        last_.clear();
        for (int64_t b = 0; b < in.batch; ++b) last_.push_back(in.token_inputs[in.seq_starts[b + 1] - 1]);
        std::vector<int32_t> lora;
        if (in.lora_slots) lora.assign(in.lora_slots, in.lora_slots + in.batch);
        Line("{\"call\":\"SetInputs\",\"batch\":" + std::to_string(in.batch) + ",\"decoding_batches\":" + std::to_string(in.decoding_batches) +
             ",\"lora_slots\":" + Arr(lora) + ",\"last_tokens\":" + Arr(last_) + "}");
        ask_.clear();   // the ask belongs to one step
        return RC_SUCCESS;
    }
    RetCode SetPromptLogprobs(const int32_t* ask, int64_t batch) override {
        Line("{\"call\":\"SetPromptLogprobs\",\"batch\":" + std::to_string(batch) + ",\"ask\":" + Arr(ask, (size_t)batch) + ",\"last_tokens\":" + Arr(last_) + "}");
        if (batch != B_) return RC_INVALID_VALUE;
        ask_.assign(ask, ask + batch);
        return RC_SUCCESS;
    }
    RetCode Run(bool) override {
        ++step_;
        logits_.assign((size_t)B_ * kVocab, 0.f);
        for (int64_t b = 0; b < B_; ++b) logits_[(size_t)b * kVocab + last_[b]] = 1.f;
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
    float* GetLogits(int64_t* stride) override {
        *stride = kVocab;
        return logits_.data();
    }
    const std::vector<int64_t>& last() const { return last_; }
    int step() const { return step_; }   // engine steps so far, the running one included
    void NewPhase() { step_ = -1; }

private:
    int64_t B_ = 0;
    int step_ = -1;
    std::vector<int64_t> tok_, seq_, last_;
    std::vector<int32_t> ask_, rows_, rank_, ttok_;
    std::vector<float> lp_, tlp_, logits_;
};

class FakePostProcessor final : public PostProcessor {
public:
    explicit FakePostProcessor(const FakeRuntime* rt) : rt_(rt) {}
    bool has_top = true;
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float*, const float*, const int32_t*, const float*, int32_t, int32_t, int32_t, int32_t, float, bool, int32_t*,
                           float*, bool) override {
        return RC_UNSUPPORTED;   // the driver runs the per-request sampler only
    }
    RetCode ApplyPenalty(const float* temps, const float* rep, const float*, const float*, const int64_t* slots, const int64_t*, const int64_t*,
                         const int64_t*, int32_t batch, int32_t, bool changed, float*) override {
        Line("{\"call\":\"ApplyPenalty\",\"batch\":" + std::to_string(batch) + ",\"req_list_changed\":" + (changed ? "1" : "0") + ",\"temperatures\":" +
             Arr(temps, batch) + ",\"repetition\":" + Arr(rep, batch) + ",\"slots\":" + Arr(slots, batch) + Last());
        return RC_SUCCESS;
    }
    RetCode SampleRows(const float* logits, const float* temps, const int32_t* top_k, const float* top_p, const uint64_t* seeds,
                       const uint64_t* draws, int32_t batch, int32_t vocab, int32_t stride, int32_t* out, float* lp) override {
        if (batch == 0) return RC_SUCCESS;
        Line("{\"call\":\"SampleRows\",\"batch\":" + std::to_string(batch) + ",\"temps_null\":" + (temps ? "0" : "1") + ",\"top_k\":" + Arr(top_k, batch) +
             ",\"top_p\":" + Arr(top_p, batch) + ",\"seeds\":" + Arr(seeds, batch) + ",\"draws\":" + Arr(draws, batch) + Last());
        for (int b = 0; b < batch; ++b) {
            int best = 0;
            for (int v = 1; v < vocab; ++v)
                if (logits[(size_t)b * stride + v] > logits[(size_t)b * stride + best]) best = v;
            out[b] = best;
            lp[b] = -(float)rt_->step();
        }
        return RC_SUCCESS;
    }
    RetCode TopLogprobs(const float*, const float* temps, const int32_t* nlp, int32_t batch, int32_t, int32_t, const int32_t** tokens,
                        const float** logprobs, int32_t* rows) override {
        Line("{\"call\":\"TopLogprobs\",\"batch\":" + std::to_string(batch) + ",\"supported\":" + (has_top ? "1" : "0") + ",\"temps_null\":" +
             (temps ? "0" : "1") + ",\"num_logprobs\":" + Arr(nlp, batch) + Last());
        if (!has_top) return RC_UNSUPPORTED;
        tok_.clear();
        lp_.clear();
        int32_t asked = 0;
        for (int b = 0; b < batch; ++b) {
            if (nlp[b] <= 0) continue;
            const int32_t id = (int32_t)rt_->last()[b] - 500;
            for (int e = 0; e < kTopLogprobsMax; ++e) {
                tok_.push_back(e >= nlp[b] ? -7 : id * 10000 + rt_->step() * 100 + e);
                lp_.push_back(e >= nlp[b] ? 7.f : -(float)e);
            }
            ++asked;
        }
        *tokens = tok_.data();
        *logprobs = lp_.data();
        *rows = asked;
        return RC_SUCCESS;
    }
    RetCode SetLogitRule(int64_t slot, const LogitRule& r) override {
        bool refuse = false;
        for (int32_t t : r.bias_tokens) refuse = refuse || t == 999;
        Line("{\"call\":\"SetLogitRule\",\"slot\":" + std::to_string(slot) + ",\"bias_tokens\":" + Arr(r.bias_tokens) + ",\"stops\":" + Arr(r.stop_tokens) +
             ",\"refused\":" + (refuse ? "1" : "0") + "}");
        return refuse ? RC_OTHER_ERROR : RC_SUCCESS;
    }
    RetCode EditLogits(float*, const int64_t* slots, const uint32_t* flags, int32_t batch, int32_t, int32_t) override {
        if (batch == 0) return RC_SUCCESS;
        Line("{\"call\":\"EditLogits\",\"batch\":" + std::to_string(batch) + ",\"slots\":" + Arr(slots, batch) + ",\"flags\":" + Arr(flags, batch) + Last());
        return RC_SUCCESS;
    }
    RetCode SetGuideVocab(const uint8_t*, const int64_t* off, int32_t n_tok) override {
        Line("{\"call\":\"SetGuideVocab\",\"n_tok\":" + std::to_string(n_tok) + ",\"bytes\":" + std::to_string(off[n_tok]) + "}");
        return RC_SUCCESS;
    }
    RetCode LoadGuide(int32_t slot, const GuideDfa& dfa, const std::vector<int32_t>& ends) override {
        std::vector<int> tr(dfa.trans.begin(), dfa.trans.end()), ac(dfa.accept.begin(), dfa.accept.end());
        Line("{\"call\":\"LoadGuide\",\"slot\":" + std::to_string(slot) + ",\"n_states\":" + std::to_string(dfa.n_states) + ",\"ends\":" + Arr(ends) +
             ",\"trans\":" + Arr(tr) + ",\"accept\":" + Arr(ac) + "}");
        return RC_SUCCESS;
    }
    RetCode UnloadGuide(int32_t slot) override {
        Line("{\"call\":\"UnloadGuide\",\"slot\":" + std::to_string(slot) + "}");
        return RC_SUCCESS;
    }
    RetCode GuideEdit(float*, const int32_t* slots, const int32_t* states, int32_t batch, int32_t, int32_t) override {
        if (batch == 0) return RC_SUCCESS;
        Line("{\"call\":\"GuideEdit\",\"batch\":" + std::to_string(batch) + ",\"slots\":" + Arr(slots, (size_t)batch) + ",\"states\":" +
             Arr(states, (size_t)batch) + Last());
        return RC_SUCCESS;
    }

private:
    std::string Last() const { return ",\"step\":" + std::to_string(rt_->step()) + ",\"last_tokens\":" + Arr(rt_->last()) + "}"; }
    const FakeRuntime* rt_;
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
                 (r.finish_flag != FinishFlag::NOT_FINISHED ? "1" : "0") + ",\"logprob\":" + std::to_string((int)r.logprob) + ",\"top_tokens\":" +
                 Arr(r.top_tokens) + ",\"top_logprobs\":" + Arr(r.top_logprobs) + ",\"prompt_logprobs\":" + Arr(r.prompt_logprobs) + ",\"prompt_ranks\":" +
                 Arr(r.prompt_ranks) + ",\"prompt_top_tokens\":" + Arr(r.prompt_top_tokens) + ",\"prompt_top_logprobs\":" + Arr(r.prompt_top_logprobs) + "}");
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
    Line("{\"phase\":\"" + g_phase + "\",\"step\":" + std::to_string(step) + ",\"req_list_changed\":" + (changed ? "1" : "0") + ",\"decoding_batches\":" +
         std::to_string(in.decoding_batches) + ",\"last_tokens\":" + Arr(last) + ",\"seq_starts\":" + Arr(in.seq_starts) + ",\"start_pos\":" +
         Arr(in.start_pos) + ",\"temperatures\":" + Arr(in.temperatures) + ",\"top_p_list\":" + Arr(in.top_p_list) + ",\"top_k_list\":" + Arr(in.top_k_list) +
         ",\"seed_list\":" + Arr(in.seed_list) + ",\"draw_list\":" + Arr(in.draw_list) + ",\"repetition_penalty_list\":" + Arr(in.repetition_penalty_list) +
         ",\"presence_penalty_list\":" + Arr(in.presence_penalty_list) + ",\"frequency_penalty_list\":" + Arr(in.frequency_penalty_list) +
         ",\"batch_slots\":" + Arr(in.batch_slots) + ",\"lora_slots\":" + Arr(in.lora_slots) + ",\"num_logprobs_list\":" + Arr(in.num_logprobs_list) +
         ",\"prompt_logprobs_list\":" + Arr(in.prompt_logprobs_list) + ",\"logit_flags\":" + Arr(in.logit_flags) + ",\"guide_slots\":" + Arr(in.guide_slots) +
         ",\"guide_states\":" + Arr(in.guide_states) + "}");
}

// everything request `id` carries: a function of the id (tests/test_chain_host.py restates it)
std::shared_ptr<Request> Spec(uint64_t id) {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->generation_length = kGen[id];
    r->early_stopping = false;
    std::vector<int> p;
    for (int i = 1; i < 2 + (int)(id % 3); ++i) p.push_back((int)(10 * id) + i);
    p.push_back((int)(500 + id));
    r->token_ids = std::make_shared<std::vector<int>>(p);
    r->temperature = 0.5f + (float)id / 16.f;
    r->top_p = (float)id / 16.f;
    r->top_k = 1 + (int32_t)id;
    r->repetition_penalty = 1.f + (float)id / 8.f;
    r->presence_penalty = (float)id / 4.f;
    r->frequency_penalty = (float)id / 32.f;
    r->seed = id % 2 ? 1000 + id : 0;
    r->num_logprobs = (int32_t)(id * 7 % 5);
    r->prompt_logprobs = id % 4 == 0 ? -1 : (int32_t)(id % 4) - 1;
    r->lora_slot = (int32_t)(id % 3) - 1;
    if (id % 3 == 2) {   // 2, 5, 8, 11: a bias on the token `id` and a stop that min_new_tokens holds back
        r->logit_bias = {{(int32_t)id, 0.5f}};
        r->min_new_tokens = 1 + (int32_t)(id % 2);
        r->stop_tokens = std::make_shared<std::unordered_set<int>>(std::unordered_set<int>{900});
    }
    if (id == 3 || id == 7 || id == 10) {   // guided: its own letter, up to twenty times
        r->guide_regex = std::string(1, (char)('a' + id)) + "{1,20}";
        r->early_stopping = true;
    }
    if (id == 7) r->logit_bias = {{7, 0.25f}};       // a finite bias beside a guide
    if (id == 9) r->logit_bias = {{kVocab, 1.f}};    // outside the vocabulary: the generator refuses the request
    if (id == 6) r->logit_bias = {{999, 1.f}};       // the backend cannot take it: the request fails on its first step
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
    mc.vocab_size = kVocab;
    mc.cache_quant_bit = 8; mc.cache_quant_group = 8; mc.cache_layout = 3; mc.cache_mode = 1; mc.page_size = 4;
    GeneratorConfig gc;
    gc.top_k = 1;
    gc.max_running_batch = 4;
    gc.max_prefill_batch = 2;
    gc.max_input_tokens_per_request = 4096; gc.max_output_tokens_per_request = 4096; gc.max_total_tokens_per_request = 8192;
    gc.max_tokens_per_step = 8192;
    gc.max_cooldown_request = 2;
    gc.stop_tokens = {901};
    gc.enable_prefix_cache = false;
    gc.enable_penalty = true;
    gc.per_request_sampling = true;
    gc.sampling_seed = 42;

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt;
    FakeTokenizer tok;
    AdapterRegistry reg;
    reg.Publish(0);
    reg.Publish(1);
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 4096;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.device_worker_pool_ = &pool;
    res.tokenizer = &tok;
    res.adapters = &reg;

    PrintingConnection conn;
    size_t want = 0;
    // the requests are queued before the generator thread starts: the admission order is `order`
    auto phase = [&](const char* name, bool has_top, const std::vector<uint64_t>& order) {
        FakePostProcessor pp(&rt);
        pp.has_top = has_top;
        res.post_processor = &pp;
        rt.NewPhase();
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = name;
        Line(std::string("{\"begin\":\"") + name + "\"}");
        for (uint64_t id : order) gen.Process(Spec(id));
        want += kRequests;
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    if (!phase("all", true, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12})) return 2;
    if (!phase("no_top", false, {1, 5, 2, 10, 3, 4, 6, 7, 8, 9, 11, 12})) return 2;
    return 0;
}
