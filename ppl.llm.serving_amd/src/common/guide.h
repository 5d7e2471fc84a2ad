// Guided decoding on the host (DESIGN.md "numerics", guided decoding row): a regular expression becomes a byte-level DFA, whose states the
// generator tracks per request and whose allowed-token masks the backend builds (PostProcessor::LoadGuide).
//
// Dialect (byte semantics, anchored at both ends): literals; a non-ASCII character as its UTF-8 byte sequence (one atom: a quantifier
// behind it repeats the character); `\` + a metacharacter; \n \t \r \xHH; `.` = any ASCII byte but \n; \d \w \s and \D \W \S (the latter
// within ASCII); classes [...] with ranges and ^ (negated within ASCII 0x00 .. 0x7f); groups ( ) and (?: ); |; * + ?; {m} {m,} {m,n} with
// n <= 256.  Refused with a message: anchors (^ $ \b \B \A \Z), backreferences, lookaround and every other (?...) form, lazy and
// possessive quantifiers, a non-ASCII character inside a class, an empty language, and an automaton of more than 255 states.
// A `{` that does not begin a well-formed quantifier is a literal, as are `}` and a `]` outside a class.
//
// Pipeline (guide_tree.h, shared with the JSON-schema front end of guide_json.h): Thompson NFA -> subset construction -> every state that
// cannot reach an accepting one becomes the dead state -> minimised by partition refinement.  State 0 is the start; states are numbered
// in breadth-first order of their first byte.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace ppl { namespace llm {

struct GuideDfa final {
    static constexpr int kDead = 255;       // the dead state: no row in `trans`, never left
    static constexpr int kMaxStates = 255;  // live states 0 .. 254 (PostProcessor::kGuideMaxStates)
    int n_states = 0;
    std::vector<uint8_t> trans;   // [n_states][256]: the next state, kDead when no match continues with that byte
    std::vector<uint8_t> accept;  // [n_states]: the bytes so far are a full match

    // the state after `bytes` from `state`; kDead as soon as the dead state is met (and for a state outside the automaton)
    int Step(int state, const uint8_t* bytes, size_t n) const {
        for (size_t i = 0; i < n; ++i) {
            if (state < 0 || state >= n_states) return kDead;
            state = trans[(size_t)state * 256 + bytes[i]];
        }
        return state >= 0 && state < n_states ? state : kDead;
    }
    int Step(int state, const std::string& bytes) const { return Step(state, (const uint8_t*)bytes.data(), bytes.size()); }
    bool Accepting(int state) const { return state >= 0 && state < n_states && accept[(size_t)state] != 0; }
};

// The wide automaton of a JSON schema (guide_json.h): 16-bit states, up to 4096 live ones.  State 255 is an ordinary state here
// (PostProcessor::LoadGuide16).
struct GuideDfa16 final {
    static constexpr int kDead = 0xFFFF;     // the dead state: no row in `trans`, never left
    static constexpr int kMaxStates = 4096;  // live states 0 .. 4095 (PostProcessor::kGuide16MaxStates)
    int n_states = 0;
    std::vector<uint16_t> trans;  // [n_states][256]
    std::vector<uint8_t> accept;  // [n_states]

    int Step(int state, const uint8_t* bytes, size_t n) const {
        for (size_t i = 0; i < n; ++i) {
            if (state < 0 || state >= n_states) return kDead;
            state = trans[(size_t)state * 256 + bytes[i]];
        }
        return state >= 0 && state < n_states ? state : kDead;
    }
    int Step(int state, const std::string& bytes) const { return Step(state, (const uint8_t*)bytes.data(), bytes.size()); }
    bool Accepting(int state) const { return state >= 0 && state < n_states && accept[(size_t)state] != 0; }
};

// false: *err says why (the construct and its position); *dfa is unspecified
bool CompileGuideRegex(const std::string& pattern, GuideDfa* dfa, std::string* err);

}}  // namespace ppl::llm
