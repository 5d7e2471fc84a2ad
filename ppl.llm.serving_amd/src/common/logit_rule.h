// A request's logit rule as the backend receives it (PostProcessor::SetLogitRule), and the admission check that makes it from the
// request's fields (DESIGN.md "numerics", logit rules row; the same checks as pplhip_logit_rule_set and tests/logit_rules.py: validate).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

namespace ppl { namespace llm {

struct LogitRule final {
    std::vector<int32_t> bias_tokens;   // unique; a banned token is here with the value -inf
    std::vector<float> bias_values;     // finite or -inf
    bool has_mask = false;
    std::vector<uint32_t> allowed_bits;  // has_mask: ceil(vocab / 32) words, token v is bit v & 31 of word v >> 5
    std::vector<int32_t> stop_tokens;   // what bit 1 of a row's flags suppresses; empty when the request has no min_new_tokens
};

constexpr int32_t kLogitRuleBiasMax = 512;  // PostProcessor::kLogitBiasMax
constexpr int32_t kLogitRuleStopMax = 64;   // PostProcessor::kLogitStopMax

// Validates and merges: the ban wins over a bias of the same token; the stops (the generator's and the request's
// own, duplicates allowed) travel only when min_new_tokens > 0.  false: *err names the field at fault, *rule is unspecified.
inline bool BuildLogitRule(const std::vector<std::pair<int32_t, float>>& logit_bias, const std::vector<int32_t>* allowed_tokens,
                           const std::vector<int32_t>& banned_tokens, int32_t min_new_tokens,
                           const std::vector<int>& stop_tokens, int32_t vocab, LogitRule* rule, std::string* err) {
    *rule = LogitRule();
    if (min_new_tokens < 0) { *err = "min_new_tokens: negative"; return false; }
    std::unordered_set<int32_t> finite, bans;
    for (const auto& p : logit_bias) {
        if (p.first < 0 || p.first >= vocab) { *err = "logit_bias: token [" + std::to_string(p.first) + "] outside the vocabulary"; return false; }
        if (p.second != p.second || p.second == INFINITY) { *err = "logit_bias: the value of token [" + std::to_string(p.first) + "] is NaN or +inf"; return false; }
        if (p.second == -INFINITY) { bans.insert(p.first); continue; }
        if (!finite.insert(p.first).second) { *err = "logit_bias: token [" + std::to_string(p.first) + "] has two values"; return false; }
    }
    for (int32_t t : banned_tokens) {
        if (t < 0 || t >= vocab) { *err = "banned_tokens: token [" + std::to_string(t) + "] outside the vocabulary"; return false; }
        bans.insert(t);
    }
    for (const auto& p : logit_bias)
        if (p.second != -INFINITY && !bans.count(p.first)) {
            rule->bias_tokens.push_back(p.first);
            rule->bias_values.push_back(p.second);
        }
    std::vector<int32_t> sorted_bans(bans.begin(), bans.end());
    std::sort(sorted_bans.begin(), sorted_bans.end());
    for (int32_t t : sorted_bans) {
        rule->bias_tokens.push_back(t);
        rule->bias_values.push_back(-INFINITY);
    }
    if ((int32_t)rule->bias_tokens.size() > kLogitRuleBiasMax) {
        *err = "logit_bias: more than " + std::to_string(kLogitRuleBiasMax) + " biased and banned tokens";
        return false;
    }
    std::unordered_set<int32_t> stops;
    if (min_new_tokens > 0) {
        for (int t : stop_tokens) {
            if (t < 0 || t >= vocab) { *err = "stop_tokens: token [" + std::to_string(t) + "] outside the vocabulary"; return false; }
            stops.insert(t);
        }
        if ((int32_t)stops.size() > kLogitRuleStopMax) {
            *err = "stop_tokens: min_new_tokens can suppress at most " + std::to_string(kLogitRuleStopMax) + " stop tokens";
            return false;
        }
        rule->stop_tokens.assign(stops.begin(), stops.end());
        std::sort(rule->stop_tokens.begin(), rule->stop_tokens.end());
    }
    int64_t live = 0;
    if (allowed_tokens) {
        rule->has_mask = true;
        rule->allowed_bits.assign(((size_t)vocab + 31) / 32, 0u);
        for (int32_t t : *allowed_tokens) {
            if (t < 0 || t >= vocab) { *err = "allowed_tokens: token [" + std::to_string(t) + "] outside the vocabulary"; return false; }
            uint32_t& w = rule->allowed_bits[(size_t)t >> 5];
            const uint32_t bit = 1u << (t & 31);
            if (!(w & bit) && !bans.count(t) && !stops.count(t)) ++live;
            w |= bit;
        }
    } else {
        std::unordered_set<int32_t> dead(bans);
        dead.insert(stops.begin(), stops.end());
        live = (int64_t)vocab - (int64_t)dead.size();
    }
    if (live <= 0) {
        *err = std::string(allowed_tokens ? "allowed_tokens" : (!bans.empty() ? "banned_tokens" : "min_new_tokens")) +
               ": the rule leaves no token the request could produce on its first step";
        return false;
    }
    return true;
}

}}  // namespace ppl::llm
