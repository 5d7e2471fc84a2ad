// A request scenario for differential runs (tests/test_gpu_tools.py): the same JSON drives this tree's offline_inference
// (--workload scenario --scenario-file f) and tests/host/ref_backend_driver (the reference's generator + engine).
//   {"generator": {"max_running_batch", "max_tokens_per_step", "max_prefill_batch", "max_cooldown_request", "enable_prefix_cache",
//                  "enable_penalty", "stop_tokens": [..]},
//    "kv_cache_max_tokens": N,
//    "requests": [{"id", "tokens": [..], "generation_length", "temperature", "top_p", "top_k", "repetition_penalty",
//                  "presence_penalty", "frequency_penalty", "early_stopping", "stop_tokens": [..], "seed", "num_logprobs", "prompt_logprobs",
//                  "logit_bias": [[token, value], ..], "allowed_tokens": [..], "banned_tokens": [..], "min_new_tokens"}]}
// "seed" (this tree's Request only: the sampling seed of --per-request-sampling, 0 or absent = none) is ignored for a request type without it.
// "num_logprobs" (this tree's Request only: ranked alternatives per generated token, 0 .. 20, 0 or absent = none) likewise.
// "prompt_logprobs" (this tree's Request only: logprob and rank of every prompt token, -1 or absent = off, 0 .. 20 = with that many ranked
// alternatives per position) likewise.
// "logit_bias" / "allowed_tokens" / "banned_tokens" / "min_new_tokens" (this tree's Request only: its logit rule; a value may be the string
// "-inf"; token ids are taken as written, an id outside the vocabulary fails the request) likewise.
// Templates: Request / GeneratorConfig are this tree's or the reference's types (same member names by construction).
#pragma once
#include <math.h>

#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <unordered_set>
#include <vector>

#include "../src/utils/mini_json.h"

namespace ppl { namespace llm { namespace scenario {

inline bool LoadScenario(const std::string& path, utils::JsonValue* doc) {
    std::ifstream ifs(path);
    if (!ifs.is_open()) return false;
    std::stringstream buf;
    buf << ifs.rdbuf();
    return utils::JsonParser(buf.str()).Parse(doc) && doc->Find("requests") != nullptr;
}

template <typename GeneratorConfigT>
void ScenarioGeneratorConfig(const utils::JsonValue& doc, GeneratorConfigT* gc) {
    const utils::JsonValue* g = doc.Find("generator");
    if (!g) return;
    gc->max_running_batch = (int)g->GetInt("max_running_batch", gc->max_running_batch);
    gc->max_tokens_per_step = (int)g->GetInt("max_tokens_per_step", gc->max_tokens_per_step);
    gc->max_cooldown_request = (int)g->GetInt("max_cooldown_request", gc->max_cooldown_request);
    gc->enable_prefix_cache = g->GetBool("enable_prefix_cache", gc->enable_prefix_cache);
    gc->enable_penalty = g->GetBool("enable_penalty", gc->enable_penalty);
    gc->max_prefill_batch = gc->enable_prefix_cache ? 1 : (int)g->GetInt("max_prefill_batch", gc->max_prefill_batch);  // offline_inference.cc:97-99
    if (const utils::JsonValue* st = g->Find("stop_tokens"))
        for (const auto& t : st->arr) gc->stop_tokens.insert((int)t.AsInt());
}

template <typename RequestT>
auto SetSeed(RequestT* q, uint64_t seed, int) -> decltype(q->seed = seed, void()) { q->seed = seed; }
template <typename RequestT>
void SetSeed(RequestT*, uint64_t, long) {}

template <typename RequestT>
auto SetNumLogprobs(RequestT* q, int32_t n, int) -> decltype(q->num_logprobs = n, void()) { q->num_logprobs = n; }
template <typename RequestT>
void SetNumLogprobs(RequestT*, int32_t, long) {}

template <typename RequestT>
auto SetPromptLogprobs(RequestT* q, int32_t n, int) -> decltype(q->prompt_logprobs = n, void()) { q->prompt_logprobs = n; }
template <typename RequestT>
void SetPromptLogprobs(RequestT*, int32_t, long) {}

template <typename RequestT>
auto SetLogitRule(RequestT* q, const utils::JsonValue& r, int) -> decltype(q->min_new_tokens = 0, void()) {
    if (const utils::JsonValue* lb = r.Find("logit_bias"))
        for (const auto& p : lb->arr) {
            if (p.arr.size() != 2) { q->logit_bias.emplace_back(-1, 0.f); continue; }   // malformed: a pair the generator refuses
            const float v = p.arr[1].type == utils::JsonValue::STRING && p.arr[1].str == "-inf" ? -INFINITY : (float)p.arr[1].num;
            q->logit_bias.emplace_back((int32_t)p.arr[0].AsInt(), v);
        }
    if (const utils::JsonValue* al = r.Find("allowed_tokens")) {
        q->allowed_tokens = std::make_shared<std::vector<int32_t>>();
        for (const auto& v : al->arr) q->allowed_tokens->push_back((int32_t)v.AsInt());
    }
    if (const utils::JsonValue* bn = r.Find("banned_tokens"))
        for (const auto& v : bn->arr) q->banned_tokens.push_back((int32_t)v.AsInt());
    q->min_new_tokens = (int32_t)r.GetInt("min_new_tokens", 0);
}
template <typename RequestT>
void SetLogitRule(RequestT*, const utils::JsonValue&, long) {}

template <typename RequestT>
std::vector<std::shared_ptr<RequestT>> ScenarioRequests(const utils::JsonValue& doc, int vocab_size) {
    std::vector<std::shared_ptr<RequestT>> out;
    for (const auto& r : doc.Find("requests")->arr) {
        auto q = std::make_shared<RequestT>((uint64_t)r.GetInt("id", (int64_t)out.size()), "", (float)r.GetNum("temperature", 1.0),
                                            (uint32_t)r.GetInt("generation_length", 8));
        q->top_p = (float)r.GetNum("top_p", 0.0);
        q->top_k = (int)r.GetInt("top_k", 1);
        q->repetition_penalty = (float)r.GetNum("repetition_penalty", 1.0);
        q->presence_penalty = (float)r.GetNum("presence_penalty", 0.0);
        q->frequency_penalty = (float)r.GetNum("frequency_penalty", 0.0);
        q->early_stopping = r.GetBool("early_stopping", true);
        SetSeed(q.get(), (uint64_t)r.GetInt("seed", 0), 0);
        SetNumLogprobs(q.get(), (int32_t)r.GetInt("num_logprobs", 0), 0);
        SetPromptLogprobs(q.get(), (int32_t)r.GetInt("prompt_logprobs", -1), 0);
        SetLogitRule(q.get(), r, 0);
        q->token_ids = std::make_shared<std::vector<int>>();
        if (const utils::JsonValue* t = r.Find("tokens"))
            for (const auto& v : t->arr) q->token_ids->push_back((int)(v.AsInt() % vocab_size));
        q->stop_tokens = std::make_shared<std::unordered_set<int>>();
        if (const utils::JsonValue* st = r.Find("stop_tokens"))
            for (const auto& v : st->arr) q->stop_tokens->insert((int)v.AsInt());
        out.push_back(q);
    }
    return out;
}

template <typename TokMap, typename FailedVec>
void PrintScenarioBody(const TokMap& tokens, const FailedVec& failed) {
    std::cout << "{\"tokens\":{";
    bool first = true;
    for (const auto& kv : tokens) {
        std::cout << (first ? "" : ",") << "\"" << kv.first << "\":[";
        for (size_t i = 0; i < kv.second.size(); ++i) std::cout << (i ? "," : "") << kv.second[i];
        std::cout << "]";
        first = false;
    }
    std::cout << "},\"failed\":[";
    for (size_t i = 0; i < failed.size(); ++i) std::cout << (i ? "," : "") << failed[i];
    std::cout << "]";
}

// {"tokens": {"id": [..]}, "failed": [ids]}
template <typename TokMap, typename FailedVec>
void PrintScenarioResult(const TokMap& tokens, const FailedVec& failed) {
    PrintScenarioBody(tokens, failed);
    std::cout << "}" << std::endl;
}

// (JSON has no infinity: a masked entry's logprob goes out as the lowest float)
template <typename T>
void PrintScenarioNumber(T v) {
    if (v < (T)-3.0e38) std::cout << "-3.4028235e38";
    else std::cout << v;
}

// what a request's first response brought when it asked for prompt logprobs (Response::prompt_*)
struct PromptLogprobs {
    std::vector<float> logprobs;
    std::vector<int32_t> ranks;
    std::vector<int32_t> top_tokens;   // n per position, flat
    std::vector<float> top_logprobs;
};

// ,"prompt_logprobs": {"id": [..]}, "prompt_ranks": {"id": [..]}, "prompt_top_tokens" / "prompt_top_logprobs": {"id": [[n per position]]}
// of the requests that asked (PromptMap: id -> PromptLogprobs); nothing when there is none
template <typename PromptMap>
void PrintScenarioPrompt(const PromptMap& prompt) {
    if (prompt.empty()) return;
    const auto prec = std::cout.precision(9);
    auto flat = [&](const char* key, auto member) {
        std::cout << ",\"" << key << "\":{";
        bool first = true;
        for (const auto& kv : prompt) {
            const auto& v = kv.second.*member;
            std::cout << (first ? "" : ",") << "\"" << kv.first << "\":[";
            for (size_t i = 0; i < v.size(); ++i) { if (i) std::cout << ","; PrintScenarioNumber(v[i]); }
            std::cout << "]";
            first = false;
        }
        std::cout << "}";
    };
    auto nested = [&](const char* key, auto member) {
        std::cout << ",\"" << key << "\":{";
        bool first = true;
        for (const auto& kv : prompt) {
            const auto& v = kv.second.*member;
            const size_t P = kv.second.logprobs.size(), n = P ? v.size() / P : 0;
            std::cout << (first ? "" : ",") << "\"" << kv.first << "\":[";
            for (size_t i = 0; i < P; ++i) {
                std::cout << (i ? "," : "") << "[";
                for (size_t j = 0; j < n; ++j) { if (j) std::cout << ","; PrintScenarioNumber(v[i * n + j]); }
                std::cout << "]";
            }
            std::cout << "]";
            first = false;
        }
        std::cout << "}";
    };
    flat("prompt_logprobs", &PromptLogprobs::logprobs);
    flat("prompt_ranks", &PromptLogprobs::ranks);
    nested("prompt_top_tokens", &PromptLogprobs::top_tokens);
    nested("prompt_top_logprobs", &PromptLogprobs::top_logprobs);
    std::cout.precision(prec);
}

// the same, plus "top_tokens" / "top_logprobs": {"id": [[..] per generated token]} of the requests that asked (TopMap: id -> per-token
// lists) and the prompt logprobs (PrintScenarioPrompt); without such a request the line is PrintScenarioResult's
template <typename TokMap, typename FailedVec, typename TopTokMap, typename TopLpMap, typename PromptMap = std::map<uint64_t, PromptLogprobs>>
void PrintScenarioResult(const TokMap& tokens, const FailedVec& failed, const TopTokMap& top_tokens, const TopLpMap& top_logprobs,
                         const PromptMap& prompt = PromptMap()) {
    PrintScenarioBody(tokens, failed);
    auto lists = [](const char* key, const auto& m) {
        std::cout << ",\"" << key << "\":{";
        bool first = true;
        for (const auto& kv : m) {
            std::cout << (first ? "" : ",") << "\"" << kv.first << "\":[";
            for (size_t i = 0; i < kv.second.size(); ++i) {
                std::cout << (i ? "," : "") << "[";
                for (size_t j = 0; j < kv.second[i].size(); ++j) {
                    if (j) std::cout << ",";
                    // (JSON has no infinity: a masked entry's logprob goes out as the lowest float)
                    if (kv.second[i][j] < -3.0e38) std::cout << "-3.4028235e38";
                    else std::cout << kv.second[i][j];
                }
                std::cout << "]";
            }
            std::cout << "]";
            first = false;
        }
        std::cout << "}";
    };
    if (!top_tokens.empty()) {
        const auto prec = std::cout.precision(9);
        lists("top_tokens", top_tokens);
        lists("top_logprobs", top_logprobs);
        std::cout.precision(prec);
    }
    PrintScenarioPrompt(prompt);
    std::cout << "}" << std::endl;
}

}}}  // namespace ppl::llm::scenario
