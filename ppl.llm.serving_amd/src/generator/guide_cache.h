// Guided decoding: the backend's guide slots as a cache from (kind, pattern or schema, end tokens) to slot.  A request holds a reference on its slot from
// admission until it leaves; a slot without references stays loaded until its place is needed (least recently used first).  The cache
// talks to the backend through the engine's four guide calls and sends the tokenizer's vocabulary in front of the first guide, once.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../common/guide.h"
#include "../common/guide_json.h"
#include "../engine/llm_engine.h"
#include "../tokenizer/tokenizer.h"

namespace ppl { namespace llm {

class GuideCache final {
public:
    GuideCache(LLMEngine* engine, const Tokenizer* tokenizer, int32_t vocab_size)
        : engine_(engine), tokenizer_(tokenizer), vocab_size_(vocab_size) {}
    // the backend outlives the cache: its guide slots go back, so that the next one finds them empty
    ~GuideCache();

    // what a guide is written in: a regular expression (narrow automaton, LoadGuide) or a JSON schema (wide automaton, LoadGuide16)
    enum class Kind { kRegex, kJsonSchema };
    // a reference on the slot that holds `text` of `kind` with `end_tokens` (sorted, unique), compiled and loaded if no slot holds it yet.
    // The key carries the kind: a regex and a schema of the same text are two guides.  -1: the request cannot be guided, *err and
    // *errcode say why
    int32_t Acquire(Kind kind, const std::string& text, const std::vector<int32_t>& end_tokens, std::string* err,
                    ppl::common::RetCode* errcode);
    void Release(int32_t slot);
    // the automaton of a slot that a running request holds: the state after `bytes` from `state`, -1 for the dead state
    int32_t Step(int32_t slot, int32_t state, const std::string& bytes) const {
        const Slot& s = slots_[slot];
        const int to = s.wide ? s.dfa16.Step(state, bytes) : s.dfa.Step(state, bytes);
        return to == (s.wide ? GuideDfa16::kDead : GuideDfa::kDead) ? -1 : to;
    }
    bool Accepting(int32_t slot, int32_t state) const {
        return slots_[slot].wide ? slots_[slot].dfa16.Accepting(state) : slots_[slot].dfa.Accepting(state);
    }

private:
    bool SendVocab();

    struct Slot {
        std::string key;   // empty: nothing loaded
        bool wide = false;   // dfa16 holds the automaton (a JSON schema), not dfa
        GuideDfa dfa;
        GuideDfa16 dfa16;
        int32_t refs = 0;
        uint64_t last_use = 0;
    };
    LLMEngine* engine_;
    const Tokenizer* tokenizer_;
    int32_t vocab_size_;
    Slot slots_[PostProcessor::kGuideMaxSlots];
    uint64_t clock_ = 0;
    int vocab_sent_ = 0;   // 0 = not sent yet, 1 = the backend has the vocabulary, -1 = it refused
};

}}  // namespace ppl::llm
