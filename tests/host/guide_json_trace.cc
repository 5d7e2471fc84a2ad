// Test driver for JSON-schema guided decoding on the host side (TEST INFRASTRUCTURE: a fake backend, never shipped).
//
//   guide_json_trace dfa            reads hex-coded schemas from stdin, one per line, and prints one JSON line per schema: the wide DFA of
//                                   CompileGuideJsonSchema (n_states; trans as the hex of its little-endian uint16 words; accept) or the
//                                   message it was refused with.
//   guide_json_trace hostbuild S V  times the allowed-token mask build of S states x V tokens on a 16-bit table as a single-thread loop on
//                                   the host (the work guide_build16_kernel does on the device) and prints the milliseconds.
//   guide_json_trace run            runs LLMGenerator + LLMEngine against a fake Runtime, a fake tokenizer and fake PostProcessors and
//                                   prints one JSON line per step, per post-processor call, per Response and per failure.
//                                   tests/test_guide_json_host.py holds the expectations.
//
// The fake tokenizer: id t < 256 is the byte t, 256 is EOS, 257 .. are the multi-byte pieces of kPieces, everything behind is empty.
// The fake model's logits are scripted by (request id, step, token): a request's temperature carries its id to the sampler.  The fake
// backend builds its masks token by token from the definition and writes -inf like the device does.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <thread>

#include "common/config.h"
#include "common/guide.h"
#include "common/guide_json.h"
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
    for (size_t i = 0; i < n; ++i) ss << (i ? "," : "") << (int64_t)v[i];
    ss << "]";
    return ss.str();
}
template <typename T>
std::string Arr(const std::vector<T>& v) { return Arr(v.data(), v.size()); }

std::string Unhex(const std::string& s) {
    std::string out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((char)strtol(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}
std::string JsonText(const std::string& s) {   // messages: printable ASCII only, quotes and backslashes escaped
    std::string out;
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { out.push_back('\\'); out.push_back((char)c); }
        else if (c < 0x20 || c >= 0x7f) out += "?";
        else out.push_back((char)c);
    }
    return out;
}

// ------------------------------------------------------------------------------------------------ dfa / hostbuild

int DfaMode() {
    static const char* d = "0123456789abcdef";
    std::string line;
    while (std::getline(std::cin, line)) {
        GuideDfa16 dfa;
        std::string err;
        if (!CompileGuideJsonSchema(Unhex(line), &dfa, &err)) {
            Line("{\"ok\":0,\"err\":\"" + JsonText(err) + "\"}");
            continue;
        }
        std::string hex;
        hex.reserve(dfa.trans.size() * 4);
        for (uint16_t w : dfa.trans)
            for (int b : {w & 255, w >> 8}) { hex.push_back(d[b >> 4]); hex.push_back(d[b & 15]); }
        Line("{\"ok\":1,\"n_states\":" + std::to_string(dfa.n_states) + ",\"trans\":\"" + hex + "\",\"accept\":" + Arr(dfa.accept) + "}");
    }
    return 0;
}

// guide_trace's host loop on a wide table: every (state, token) walk, single thread.  A synthetic automaton over eight letters in which a
// walk rarely dies, and tokens of 1 .. 9 bytes (5 on average), so that nearly every walk reads all its bytes
int HostBuildMode(int S, int V) {
    if (S < 1 || S > GuideDfa16::kMaxStates || V < 1) return 64;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<uint16_t> trans((size_t)S * 256, 0xFFFF);
    for (int s = 0; s < S; ++s)
        for (int c = 'a'; c <= 'h'; ++c) trans[(size_t)s * 256 + c] = rnd() % 50 == 0 ? 0xFFFF : (uint16_t)(rnd() % (uint64_t)S);
    std::string blob;
    std::vector<int64_t> off(1, 0);
    for (int t = 0; t < V; ++t) {
        const int len = 1 + (int)(rnd() % 9);
        for (int i = 0; i < len; ++i) blob.push_back((char)('a' + rnd() % 8));
        off.push_back((int64_t)blob.size());
    }
    const size_t words = ((size_t)V + 31) / 32;
    std::vector<uint32_t> mask((size_t)S * words, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < S; ++s)
        for (int t = 0; t < V; ++t) {
            int cur = s;
            int64_t i = off[(size_t)t];
            for (; i < off[(size_t)t + 1]; ++i) {
                cur = trans[(size_t)cur * 256 + (uint8_t)blob[(size_t)i]];
                if (cur == 0xFFFF) break;
            }
            if (i == off[(size_t)t + 1]) mask[(size_t)s * words + ((size_t)t >> 5)] |= 1u << (t & 31);
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t bits = 0;
    for (uint32_t w : mask) bits += (uint64_t)__builtin_popcount(w);
    Line("{\"host_build_ms\":" + std::to_string(ms) + ",\"states\":" + std::to_string(S) + ",\"tokens\":" + std::to_string(V) + ",\"bytes\":" +
         std::to_string(blob.size()) + ",\"allowed_bits\":" + std::to_string(bits) + "}");
    return 0;
}

// ------------------------------------------------------------------------------------------------ run: the fakes

const int kVocab = 300, kEos = 256;
const char* const kPieces[] = {"true", "false", "\"a", "\": ", ", \"", "12", "-4", "null", "{\""};   // ids 257 ..

class FakeTokenizer : public Tokenizer {
public:
    void Encode(const char*, uint32_t, std::vector<int>*) const override {}
    void Decode(int*, uint32_t, std::string*) const override {}
    int GetBosId() const override { return 1; }
    int GetEosId() const override { return kEos; }
    bool TokenBytes(int id, std::string* b) const override {
        b->clear();
        if (id >= 0 && id < 256) b->push_back((char)id);
        else if (id > kEos && id <= kEos + (int)(sizeof(kPieces) / sizeof(kPieces[0]))) *b = kPieces[id - kEos - 1];
        return true;
    }
};

class FakeRuntime final : public Runtime {
public:
    RetCode SetInputs(const StepInputs& in) override { B_ = in.batch; return RC_SUCCESS; }
    RetCode Run(bool) override { logits_.assign((size_t)B_ * kVocab, 0.f); return RC_SUCCESS; }
    float* GetLogits(int64_t* stride) override { *stride = kVocab; return logits_.data(); }

private:
    int64_t B_ = 0;
    std::vector<float> logits_;
};

// the scripted model: what request `id` thinks of token v on its n-th step; EOS is liked best wherever it is allowed, and the closing
// quote, bracket and brace next, so that unbounded strings and arrays end
float Score(int id, int step, int v) {
    uint64_t x = (uint64_t)id * 1000003ull + (uint64_t)step * 10007ull + (uint64_t)v * 101ull + 12345;
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (float)(x % 1000) / 1000.f + (v == kEos ? 10.f : 0.f) + ((v == '"' || v == ']' || v == '}') && step % 3 == 2 ? 5.f : 0.f);
}

// a backend with regex guides only: the sampler, the penalty, LoadGuide -- and no LoadGuide16
class NarrowPostProcessor : public PostProcessor {
public:
    RetCode InitPostProcessorMem(int, int, bool) override { return RC_SUCCESS; }
    RetCode SampleTopKTopP(const float* logits, const float* temps, const int32_t*, const float*, int32_t batch, int32_t vocab, int32_t stride,
                           int32_t, float, bool, int32_t* out, float* lp, bool) override {
        std::vector<int> ids;
        for (int b = 0; b < batch; ++b) {
            const int id = (int)temps[b];
            const int step = steps_[id]++;
            int best = -1;
            float best_score = -INFINITY;
            for (int v = 0; v < vocab; ++v) {
                const float s = logits[(size_t)b * stride + v] + Score(id, step, v);
                if (s > best_score) { best_score = s; best = v; }
            }
            out[b] = best;
            lp[b] = 0.f;
            ids.push_back(id);
        }
        Line("{\"call\":\"Sample\",\"ids\":" + Arr(ids) + ",\"tokens\":" + Arr(out, (size_t)batch) + "}");
        return RC_SUCCESS;
    }
    RetCode ApplyPenalty(const float*, const float*, const float*, const float*, const int64_t*, const int64_t*, const int64_t*, const int64_t*,
                         int32_t, int32_t, bool, float*) override {
        return RC_SUCCESS;
    }
    RetCode SetLogitRule(int64_t, const LogitRule&) override { return RC_SUCCESS; }
    RetCode EditLogits(float*, const int64_t*, const uint32_t*, int32_t, int32_t, int32_t) override { return RC_SUCCESS; }
    RetCode SetGuideVocab(const uint8_t* bytes, const int64_t* off, int32_t n_tok) override {
        vocab_.clear();
        for (int t = 0; t < n_tok; ++t) vocab_.emplace_back((const char*)bytes + off[t], (size_t)(off[t + 1] - off[t]));
        Line("{\"call\":\"SetGuideVocab\",\"n_tok\":" + std::to_string(n_tok) + "}");
        return RC_SUCCESS;
    }
    RetCode LoadGuide(int32_t slot, const GuideDfa& dfa, const std::vector<int32_t>& ends) override {
        Line("{\"call\":\"LoadGuide\",\"slot\":" + std::to_string(slot) + ",\"n_states\":" + std::to_string(dfa.n_states) + ",\"ends\":" + Arr(ends) + "}");
        if (slot < 0 || slot >= kGuideMaxSlots || kind_[slot]) return RC_INVALID_VALUE;
        dfa_[slot] = dfa;
        ends_[slot] = ends;
        kind_[slot] = 1;
        return RC_SUCCESS;
    }
    RetCode UnloadGuide(int32_t slot) override {
        Line("{\"call\":\"UnloadGuide\",\"slot\":" + std::to_string(slot) + "}");
        if (slot < 0 || slot >= kGuideMaxSlots || !kind_[slot]) return RC_INVALID_VALUE;
        kind_[slot] = 0;
        return RC_SUCCESS;
    }
    RetCode GuideEdit(float* logits, const int32_t* slots, const int32_t* states, int32_t batch, int32_t vocab, int32_t stride) override {
        if (batch == 0) return RC_SUCCESS;
        Line("{\"call\":\"GuideEdit\",\"batch\":" + std::to_string(batch) + ",\"slots\":" + Arr(slots, (size_t)batch) + ",\"states\":" +
             Arr(states, (size_t)batch) + "}");
        for (int b = 0; b < batch; ++b) {
            const int g = slots[b];
            if (g < 0) continue;
            if (g >= kGuideMaxSlots || !kind_[g] || states[b] < 0 || states[b] >= States(g)) return RC_INVALID_VALUE;
            for (int v = 0; v < vocab; ++v) {
                bool ok;
                if (std::find(ends_[g].begin(), ends_[g].end(), v) != ends_[g].end()) ok = Accepting(g, states[b]);
                else ok = v < (int)vocab_.size() && !vocab_[(size_t)v].empty() && Alive(g, states[b], vocab_[(size_t)v]);
                if (!ok) logits[(size_t)b * stride + v] = -INFINITY;
            }
        }
        return RC_SUCCESS;
    }

protected:
    int States(int g) const { return kind_[g] == 2 ? dfa16_[g].n_states : dfa_[g].n_states; }
    bool Accepting(int g, int s) const { return kind_[g] == 2 ? dfa16_[g].Accepting(s) : dfa_[g].Accepting(s); }
    bool Alive(int g, int s, const std::string& bytes) const {
        return kind_[g] == 2 ? dfa16_[g].Step(s, bytes) != GuideDfa16::kDead : dfa_[g].Step(s, bytes) != GuideDfa::kDead;
    }
    std::vector<std::string> vocab_;
    GuideDfa dfa_[kGuideMaxSlots];
    GuideDfa16 dfa16_[kGuideMaxSlots];
    std::vector<int32_t> ends_[kGuideMaxSlots];
    int kind_[kGuideMaxSlots] = {};   // 0 = empty, 1 = narrow, 2 = wide

private:
    std::map<int, int> steps_;
};

class WidePostProcessor final : public NarrowPostProcessor {
public:
    RetCode LoadGuide16(int32_t slot, const GuideDfa16& dfa, const std::vector<int32_t>& ends) override {
        Line("{\"call\":\"LoadGuide16\",\"slot\":" + std::to_string(slot) + ",\"n_states\":" + std::to_string(dfa.n_states) + ",\"ends\":" + Arr(ends) + "}");
        if (slot < 0 || slot >= kGuideMaxSlots || kind_[slot]) return RC_INVALID_VALUE;
        dfa16_[slot] = dfa;
        ends_[slot] = ends;
        kind_[slot] = 2;
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
                 (r.finish_flag == FinishFlag::NOT_FINISHED ? "0" : r.finish_flag == FinishFlag::LENGTH ? "\"length\"" : "\"eos\"") + "}");
            if (r.finish_flag != FinishFlag::NOT_FINISHED) ++done_;
        }
        cv_.notify_all();
    }
    void NotifyFailure(uint64_t id, RetCode rc, const std::string& msg) override {
        std::lock_guard<std::mutex> g(mu_);
        Line("{\"failed\":" + std::to_string(id) + ",\"code\":\"" + (rc == RC_UNSUPPORTED ? "unsupported" : rc == RC_INVALID_VALUE ? "invalid" : "other") +
             "\",\"msg\":\"" + JsonText(msg) + "\"}");
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

void Observe(void*, uint64_t step, const ModelInput& in, bool, bool) {
    std::vector<int> ids;
    for (float t : in.temperatures) ids.push_back((int)t);
    Line("{\"phase\":\"" + g_phase + "\",\"step\":" + std::to_string(step) + ",\"ids\":" + Arr(ids) + ",\"guide_slots\":" + Arr(in.guide_slots) +
         ",\"guide_states\":" + Arr(in.guide_states) + "}");
}

std::shared_ptr<Request> MakeRequest(uint64_t id, int gen, const std::string& schema, const std::string& regex = "") {
    auto r = std::make_shared<Request>();
    r->id = id;
    r->temperature = (float)id;   // carries the id to the fake sampler
    r->generation_length = gen;
    r->early_stopping = true;
    r->guide_json_schema = schema;
    r->guide_regex = regex;
    r->token_ids = std::make_shared<std::vector<int>>(std::vector<int>{7, 8, 9});
    return r;
}

void WaitIdle(LLMGenerator& gen) {
    while (!gen.IsIdle()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
}

// the schemas of the run, by name; the test compiles the same texts through `dfa` (argv: run prints them first)
const char* const kLong =   // some 330 bytes of fixed text: every one a state, so the walk passes state 256 and beyond
    "{\"type\":\"object\",\"properties\":{"
    "\"the_first_property_has_a_long_name_so_that_the_automaton_needs_many_states\":{\"type\":\"boolean\"},"
    "\"the_second_property_has_a_long_name_too_and_takes_a_small_integer_or_null\":{\"type\":[\"integer\",\"null\"]},"
    "\"the_third_property_is_an_enum_with_long_values\":{\"enum\":[\"the first long value of the enum\",\"the second long value of the enum\"]},"
    "\"the_fourth_property_is_a_short_string_of_at_most_three_characters_in_all\":{\"type\":\"string\",\"maxLength\":3}},"
    "\"required\":[\"the_first_property_has_a_long_name_so_that_the_automaton_needs_many_states\","
    "\"the_second_property_has_a_long_name_too_and_takes_a_small_integer_or_null\",\"the_third_property_is_an_enum_with_long_values\","
    "\"the_fourth_property_is_a_short_string_of_at_most_three_characters_in_all\"]}";
const char* const kSmall = "{\"type\":\"array\",\"items\":{\"type\":\"boolean\"},\"maxItems\":3}";
const char* const kBoth = "{\"type\":\"null\"}";   // a schema and, read as a regular expression, its own text

int RunMode() {
    ModelConfig mc;
    mc.hidden_dim = 64; mc.intermediate_dim = 64; mc.num_layers = 1; mc.num_heads = 2; mc.num_kv_heads = 2;
    mc.vocab_size = kVocab;
    mc.cache_quant_bit = 8; mc.cache_quant_group = 8; mc.cache_layout = 3; mc.cache_mode = 1; mc.page_size = 4;
    GeneratorConfig gc;
    gc.top_k = 1;
    gc.max_running_batch = 32;
    gc.max_input_tokens_per_request = 4096; gc.max_output_tokens_per_request = 4096; gc.max_total_tokens_per_request = 8192;
    gc.max_tokens_per_step = 8192;
    gc.max_cooldown_request = 2;
    gc.stop_tokens = {299};
    gc.enable_prefix_cache = false;
    gc.max_prefill_batch = 32;
    gc.enable_penalty = false;

    StaticThreadPool pool;
    pool.Init(1);
    FakeRuntime rt;
    FakeTokenizer tok;
    Resource res;
    res.tensor_parallel_size = 1;
    res.kv_cache_max_tokens = 8192;
    res.items.resize(1);
    res.items[0].runtime = &rt;
    res.device_worker_pool_ = &pool;
    res.tokenizer = &tok;

    Line(std::string("{\"schema\":\"long\",\"text\":\"") + JsonText(kLong) + "\"}");
    Line(std::string("{\"schema\":\"small\",\"text\":\"") + JsonText(kSmall) + "\"}");
    Line(std::string("{\"schema\":\"both\",\"text\":\"") + JsonText(kBoth) + "\"}");

    PrintingConnection conn;
    size_t want = 0;
    // every phase: the requests are queued before the generator thread starts, so the admission order is the order of `reqs`
    auto phase = [&](const char* name, PostProcessor* pp, const std::vector<std::shared_ptr<Request>>& reqs) {
        res.post_processor = pp;
        LLMGenerator gen(res, gc, mc, &conn);
        gen.SetStepObserver(Observe, nullptr);
        g_phase = name;
        Line(std::string("{\"begin\":\"") + name + "\"}");
        for (const auto& r : reqs) gen.Process(r);
        want += reqs.size();
        if (gen.Init() != RC_SUCCESS) return false;
        conn.WaitDone(want);
        WaitIdle(gen);
        return true;
    };
    // 1. schemas, a regex and a plain request side by side: 1 and 4 share a schema (one load); 5 is the regex whose text is 6's schema
    //    (two loads, of two kinds); 2 walks through more than 256 states; 3 is plain
    {
        WidePostProcessor pp;
        if (!phase("mixed", &pp,
                   {MakeRequest(1, 40, kSmall), MakeRequest(2, 500, kLong), MakeRequest(3, 3, ""), MakeRequest(4, 40, kSmall),
                    MakeRequest(5, 40, "", kBoth), MakeRequest(6, 40, kBoth)}))
            return 2;
    }
    // 2. every exclusion, both fields, a refused schema: each fails alone beside a guided request that is served
    {
        std::vector<std::shared_ptr<Request>> reqs;
        auto add = [&](uint64_t id, const std::string& schema) { reqs.push_back(MakeRequest(id, 40, schema)); return reqs.back().get(); };
        add(1, kSmall)->early_stopping = false;
        add(2, kSmall)->allowed_tokens = std::make_shared<std::vector<int32_t>>(std::vector<int32_t>{'[', ']'});
        add(3, kSmall)->banned_tokens = {5};
        add(4, kSmall)->min_new_tokens = 1;
        add(5, kSmall)->logit_bias = {{5, -INFINITY}};
        add(6, kSmall)->logit_bias = {{5, 1.5f}};   // a finite bias is fine
        add(7, kSmall)->guide_regex = "ok";         // both fields
        add(8, "{\"type\":\"string\",\"pattern\":\"a+\"}");
        add(9, "{\"type\":");
        add(10, kSmall);
        WidePostProcessor pp;
        if (!phase("exclusions", &pp, reqs)) return 2;
    }
    // 3. a backend with regex guides and without LoadGuide16: the schema's request fails alone, the regex and the plain one are served
    {
        NarrowPostProcessor pp;
        if (!phase("narrow_backend", &pp, {MakeRequest(1, 40, kSmall), MakeRequest(2, 8, "", "ok"), MakeRequest(3, 3, "")})) return 2;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "dfa") return DfaMode();
    if (mode == "hostbuild" && argc > 3) return HostBuildMode(atoi(argv[2]), atoi(argv[3]));
    if (mode == "run") return RunMode();
    std::cerr << "usage: guide_json_trace dfa | hostbuild STATES TOKENS | run" << std::endl;
    return 64;
}
