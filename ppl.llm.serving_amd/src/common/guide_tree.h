// The shared back half of the guide compilers (guide.cc's regular expressions, guide_json.cc's JSON schemas): a front end builds a syntax
// tree over byte sets, and BuildAutomaton turns it into the minimal trimmed byte-level DFA:
//   Thompson NFA -> subset construction -> every state that cannot reach an accepting one becomes the dead state -> minimised (Hopcroft's
//   partition refinement) -> states numbered breadth-first from the start, bytes ascending, so that state 0 is the start.
// Bytes that no set of the tree tells apart share one column of work (a JSON automaton has some thirty such classes, not 256).
// Why Hopcroft and byte classes where the regex compiler alone had Moore's rounds over 256 columns: Moore needs one round per level of
// the automaton's depth, and a schema's automaton is a long chain (a list of up to 256 integers: 5378 states, as deep), so its cost is
// states x depth x 256 -- some 7 x 10^9 signature entries there and 10^12 at the 65,534-state working bound, inside request admission.
// The minimal automaton is unique and the numbering below does not depend on how it was found, so a pattern's table is what it was.
// The automaton comes out on 32-bit states; each front end narrows it to its own table type and enforces its own limit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <bitset>
#include <memory>
#include <string>
#include <vector>

namespace ppl { namespace llm { namespace guide_tree {

typedef std::bitset<256> ByteSet;

constexpr size_t kMaxNfaStates = 200000;   // counted repetitions copy their operand

struct Node {
    enum Type { EMPTY, SET, CAT, ALT, REPEAT } type = EMPTY;
    ByteSet set;
    std::vector<std::unique_ptr<Node>> kids;
    int min = 0, max = 0;   // REPEAT: max -1 = unbounded
};
typedef std::unique_ptr<Node> NodePtr;

ByteSet Range(int lo, int hi);
NodePtr MakeEmpty();
NodePtr MakeSet(const ByteSet& s);
NodePtr MakeLiteral(const std::string& bytes);             // the bytes in a row
NodePtr MakeCat(std::vector<NodePtr> kids);
NodePtr MakeAlt(std::vector<NodePtr> kids);                // no kid: matches nothing
NodePtr MakeRepeat(NodePtr kid, int min, int max);         // max -1: unbounded
NodePtr Clone(const Node& n);
// the nodes that the helpers above have made on this thread since ResetNodeCount(): a front end whose trees grow with its input (a
// schema's nesting) bounds its own work by it, before the NFA builder's cap can
size_t NodeCount();
void ResetNodeCount();

struct Automaton {
    int n_states = 0;
    std::vector<int32_t> next;    // [n_states][256]: the next state, -1 when no match continues with that byte
    std::vector<uint8_t> accept;  // [n_states]
};

enum class BuildError { kNone, kNfaTooLarge, kSubsetTooLarge, kEmptyLanguage };

// max_subset_states bounds the automaton BEFORE minimisation
BuildError BuildAutomaton(const Node& root, size_t max_subset_states, Automaton* out);

}}}  // namespace ppl::llm::guide_tree
