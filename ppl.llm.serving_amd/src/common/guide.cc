#include "guide.h"

#include <algorithm>
#include <deque>
#include <map>

#include "guide_tree.h"

namespace ppl { namespace llm {

namespace guide_tree {

ByteSet Range(int lo, int hi) {
    ByteSet s;
    for (int b = lo; b <= hi; ++b) s.set((size_t)b);
    return s;
}

namespace {
thread_local size_t g_nodes = 0;
NodePtr NewNode() {
    ++g_nodes;
    return NodePtr(new Node());
}
}  // namespace

size_t NodeCount() { return g_nodes; }
void ResetNodeCount() { g_nodes = 0; }

NodePtr MakeEmpty() { return NewNode(); }

NodePtr MakeSet(const ByteSet& s) {
    NodePtr n = NewNode();
    n->type = Node::SET;
    n->set = s;
    return n;
}

NodePtr MakeCat(std::vector<NodePtr> kids) {
    NodePtr n = NewNode();
    n->type = kids.empty() ? Node::EMPTY : Node::CAT;
    n->kids = std::move(kids);
    return n;
}

NodePtr MakeAlt(std::vector<NodePtr> kids) {
    NodePtr n = NewNode();
    n->type = Node::ALT;
    n->kids = std::move(kids);
    return n;
}

NodePtr MakeRepeat(NodePtr kid, int min, int max) {
    NodePtr n = NewNode();
    n->type = Node::REPEAT;
    n->min = min;
    n->max = max;
    n->kids.push_back(std::move(kid));
    return n;
}

NodePtr MakeLiteral(const std::string& bytes) {
    std::vector<NodePtr> kids;
    for (unsigned char c : bytes) kids.push_back(MakeSet(Range(c, c)));
    return MakeCat(std::move(kids));
}

NodePtr Clone(const Node& n) {
    NodePtr c = NewNode();
    c->type = n.type;
    c->set = n.set;
    c->min = n.min;
    c->max = n.max;
    for (const auto& k : n.kids) c->kids.push_back(Clone(*k));
    return c;
}

namespace {

// Thompson construction: a state has epsilon edges and at most one byte-set edge
struct Nfa {
    struct State {
        std::vector<int> eps;
        ByteSet set;
        int to = -1;
    };
    std::vector<State> st;
    bool too_large = false;

    int New() {
        if (st.size() >= kMaxNfaStates) { too_large = true; return 0; }
        st.emplace_back();
        return (int)st.size() - 1;
    }
    void Eps(int a, int b) { st[(size_t)a].eps.push_back(b); }

    // builds the fragment of n between two fresh states; returns (start, end)
    std::pair<int, int> Build(const Node& n) {
        if (too_large) return {0, 0};
        switch (n.type) {
            case Node::EMPTY: {
                const int s = New(), e = New();
                Eps(s, e);
                return {s, e};
            }
            case Node::SET: {
                const int s = New(), e = New();
                st[(size_t)s].set = n.set;
                st[(size_t)s].to = e;
                return {s, e};
            }
            case Node::CAT: {
                const int s = New();
                int cur = s;
                for (const auto& k : n.kids) {
                    const auto f = Build(*k);
                    Eps(cur, f.first);
                    cur = f.second;
                }
                return {s, cur};
            }
            case Node::ALT: {
                const int s = New(), e = New();
                for (const auto& k : n.kids) {
                    const auto f = Build(*k);
                    Eps(s, f.first);
                    Eps(f.second, e);
                }
                return {s, e};
            }
            case Node::REPEAT: {
                const Node& k = *n.kids[0];
                const int s = New();
                int cur = s;
                for (int i = 0; i < n.min && !too_large; ++i) {
                    const auto f = Build(k);
                    Eps(cur, f.first);
                    cur = f.second;
                }
                const int e = New();
                if (n.max == -1) {   // cur -> (k)* -> e
                    const auto f = Build(k);
                    Eps(cur, f.first);
                    Eps(f.second, f.first);
                    Eps(f.second, e);
                    Eps(cur, e);
                } else {
                    for (int i = n.min; i < n.max && !too_large; ++i) {
                        Eps(cur, e);
                        const auto f = Build(k);
                        Eps(cur, f.first);
                        cur = f.second;
                    }
                    Eps(cur, e);
                }
                return {s, e};
            }
        }
        return {0, 0};
    }
};

void Closure(const Nfa& nfa, std::vector<int>* set, std::vector<uint8_t>* mark) {
    std::vector<int> stack(*set);
    for (int s : *set) (*mark)[(size_t)s] = 1;
    while (!stack.empty()) {
        const int s = stack.back();
        stack.pop_back();
        for (int t : nfa.st[(size_t)s].eps)
            if (!(*mark)[(size_t)t]) {
                (*mark)[(size_t)t] = 1;
                set->push_back(t);
                stack.push_back(t);
            }
    }
    for (int s : *set) (*mark)[(size_t)s] = 0;
    std::sort(set->begin(), set->end());
}

// byte classes: two bytes are in one class when every set of the NFA holds both or neither.  cls_of[b] numbers the classes by their
// smallest byte, ascending; rep[c] is that byte
int ByteClasses(const Nfa& nfa, int cls_of[256], std::vector<int>* rep) {
    std::vector<ByteSet> sets;
    for (const auto& s : nfa.st)
        if (s.to >= 0 && std::find(sets.begin(), sets.end(), s.set) == sets.end()) sets.push_back(s.set);
    std::map<std::vector<bool>, int> ids;
    for (int b = 0; b < 256; ++b) {
        std::vector<bool> sig(sets.size());
        for (size_t i = 0; i < sets.size(); ++i) sig[i] = sets[i].test((size_t)b);
        auto it = ids.find(sig);
        if (it == ids.end()) {
            it = ids.emplace(sig, (int)ids.size()).first;
            rep->push_back(b);
        }
        cls_of[b] = it->second;
    }
    return (int)ids.size();
}

// Hopcroft's partition refinement on a complete automaton of n states (the last one may be a sink) over k symbols: next[s * k + c].
// Returns the block of every state; *n_blocks their number
std::vector<int> Minimise(int n, int k, const std::vector<int>& next, const std::vector<uint8_t>& acc, int* n_blocks) {
    // predecessors of every (state, symbol), as one array with offsets
    std::vector<int> off((size_t)n * k + 1, 0), pred((size_t)n * k);
    for (int s = 0; s < n; ++s)
        for (int c = 0; c < k; ++c) ++off[(size_t)next[(size_t)s * k + c] * k + c + 1];
    for (size_t i = 0; i < (size_t)n * k; ++i) off[i + 1] += off[i];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int s = 0; s < n; ++s)
            for (int c = 0; c < k; ++c) pred[(size_t)fill[(size_t)next[(size_t)s * k + c] * k + c]++] = s;
    }
    // the partition: elems holds the states block by block, block b is elems[first[b] .. last[b])
    std::vector<int> elems((size_t)n), loc((size_t)n), blk((size_t)n), first, last, marked;
    int n_acc = 0;
    for (int s = 0; s < n; ++s) n_acc += acc[(size_t)s] ? 1 : 0;
    {
        int a = 0, r = n_acc;
        for (int s = 0; s < n; ++s) {
            const int at = acc[(size_t)s] ? a++ : r++;
            elems[(size_t)at] = s;
            loc[(size_t)s] = at;
        }
    }
    auto new_block = [&](int b, int e) {
        first.push_back(b);
        last.push_back(e);
        marked.push_back(0);
        for (int i = b; i < e; ++i) blk[(size_t)elems[(size_t)i]] = (int)first.size() - 1;
    };
    if (n_acc > 0) new_block(0, n_acc);
    if (n_acc < n) new_block(n_acc, n);
    // (block, symbol) splitters.  One of the two first blocks suffices to begin with; after a split the new block, which is the smaller
    // half, always goes in: enough where the parent does not wait as a splitter, and needed beside it where it does
    std::vector<std::pair<int, int>> work;
    for (int c = 0; c < k; ++c) work.emplace_back(0, c);
    std::vector<int> hit, touched;
    while (!work.empty()) {
        const int a = work.back().first, c = work.back().second;
        work.pop_back();
        hit.clear();
        for (int i = first[(size_t)a]; i < last[(size_t)a]; ++i) {
            const size_t cell = (size_t)elems[(size_t)i] * k + c;
            for (int j = off[cell]; j < off[cell + 1]; ++j) hit.push_back(pred[(size_t)j]);
        }
        // move the hit states to the front of their blocks
        touched.clear();
        for (int s : hit) {
            const int b = blk[(size_t)s];
            const int at = first[(size_t)b] + marked[(size_t)b];
            if (loc[(size_t)s] < at) continue;   // marked already (a state has one successor per symbol, but `hit` may repeat it through A's members)
            if (marked[(size_t)b] == 0) touched.push_back(b);
            const int other = elems[(size_t)at];
            elems[(size_t)loc[(size_t)s]] = other;
            loc[(size_t)other] = loc[(size_t)s];
            elems[(size_t)at] = s;
            loc[(size_t)s] = at;
            ++marked[(size_t)b];
        }
        for (int b : touched) {
            const int m = marked[(size_t)b];
            marked[(size_t)b] = 0;
            const int size = last[(size_t)b] - first[(size_t)b];
            if (m == size) continue;
            // the smaller part becomes the new block
            const int nb = (int)first.size();
            if (m <= size - m) {
                new_block(first[(size_t)b], first[(size_t)b] + m);
                first[(size_t)b] += m;
            } else {
                new_block(first[(size_t)b] + m, last[(size_t)b]);
                last[(size_t)b] = first[(size_t)b] + m;
            }
            for (int c2 = 0; c2 < k; ++c2) work.emplace_back(nb, c2);
        }
    }
    *n_blocks = (int)first.size();
    return blk;
}

}  // namespace

BuildError BuildAutomaton(const Node& root, size_t max_subset_states, Automaton* out) {
    Nfa nfa;
    const auto whole = nfa.Build(root);
    if (nfa.too_large) return BuildError::kNfaTooLarge;
    const int final_state = whole.second;
    int cls_of[256];
    std::vector<int> cls_rep;
    const int k = ByteClasses(nfa, cls_of, &cls_rep);

    // subset construction, one column per byte class; states are found in the order of ascending bytes
    std::vector<std::vector<int>> subsets;
    std::map<std::vector<int>, int> ids;
    std::vector<int> next;   // [state][k], -1 = no NFA state left
    std::vector<uint8_t> mark(nfa.st.size(), 0);
    std::vector<int> start(1, whole.first);
    Closure(nfa, &start, &mark);
    ids[start] = 0;
    subsets.push_back(start);
    for (size_t i = 0; i < subsets.size(); ++i) {
        next.resize((i + 1) * (size_t)k, -1);
        std::vector<int> edges;   // only the states with a byte edge matter
        for (int s : subsets[i])
            if (nfa.st[(size_t)s].to >= 0) edges.push_back(s);
        for (int c = 0; c < k; ++c) {
            const size_t b = (size_t)cls_rep[(size_t)c];
            std::vector<int> to;
            for (int s : edges)
                if (nfa.st[(size_t)s].set.test(b)) to.push_back(nfa.st[(size_t)s].to);
            if (to.empty()) continue;
            std::sort(to.begin(), to.end());
            to.erase(std::unique(to.begin(), to.end()), to.end());
            Closure(nfa, &to, &mark);
            auto it = ids.find(to);
            if (it == ids.end()) {
                if (subsets.size() >= max_subset_states) return BuildError::kSubsetTooLarge;
                it = ids.emplace(to, (int)subsets.size()).first;
                subsets.push_back(to);
            }
            next[i * (size_t)k + (size_t)c] = it->second;
        }
    }
    const int n = (int)subsets.size();
    std::vector<uint8_t> acc((size_t)n, 0);
    for (int i = 0; i < n; ++i) acc[(size_t)i] = std::binary_search(subsets[(size_t)i].begin(), subsets[(size_t)i].end(), final_state);

    // trim: a state that reaches no accepting state is dead
    std::vector<std::vector<int>> rev((size_t)n);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < k; ++c)
            if (next[(size_t)i * k + c] >= 0) rev[(size_t)next[(size_t)i * k + c]].push_back(i);
    std::vector<uint8_t> live((size_t)n, 0);
    std::deque<int> queue;
    for (int i = 0; i < n; ++i)
        if (acc[(size_t)i]) { live[(size_t)i] = 1; queue.push_back(i); }
    while (!queue.empty()) {
        const int s = queue.front();
        queue.pop_front();
        for (int p : rev[(size_t)s])
            if (!live[(size_t)p]) { live[(size_t)p] = 1; queue.push_back(p); }
    }
    if (!live[0]) return BuildError::kEmptyLanguage;

    // minimise the live states plus one sink (state n) that stands for the dead state
    std::vector<int> full((size_t)(n + 1) * k, n);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < k; ++c) {
            const int to = next[(size_t)i * k + c];
            if (live[(size_t)i] && to >= 0 && live[(size_t)to]) full[(size_t)i * k + c] = to;
        }
    std::vector<uint8_t> acc_full((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) acc_full[(size_t)i] = live[(size_t)i] && acc[(size_t)i];
    int n_blocks = 0;
    const std::vector<int> blk = Minimise(n + 1, k, full, acc_full, &n_blocks);
    const int dead_blk = blk[(size_t)n];   // (every state that is not live is in it: it behaves like the sink)

    // number the classes breadth-first from the start, bytes ascending
    std::vector<int> rep((size_t)n_blocks, -1), order((size_t)n_blocks, -1);
    for (int i = n - 1; i >= 0; --i)
        if (live[(size_t)i]) rep[(size_t)blk[(size_t)i]] = i;
    std::vector<int> bfs;
    order[(size_t)blk[0]] = 0;
    bfs.push_back(blk[0]);
    for (size_t i = 0; i < bfs.size(); ++i) {
        const int r = rep[(size_t)bfs[i]];
        for (int c = 0; c < k; ++c) {
            const int to = blk[(size_t)full[(size_t)r * k + c]];
            if (to == dead_blk || order[(size_t)to] >= 0) continue;
            order[(size_t)to] = (int)bfs.size();
            bfs.push_back(to);
        }
    }
    const int live_states = (int)bfs.size();
    out->n_states = live_states;
    out->next.assign((size_t)live_states * 256, -1);
    out->accept.assign((size_t)live_states, 0);
    for (int s = 0; s < live_states; ++s) {
        const int r = rep[(size_t)bfs[(size_t)s]];
        out->accept[(size_t)s] = acc[(size_t)r];
        for (int b = 0; b < 256; ++b) {
            const int to = blk[(size_t)full[(size_t)r * k + cls_of[b]]];
            if (to != dead_blk) out->next[(size_t)s * 256 + (size_t)b] = order[(size_t)to];
        }
    }
    return BuildError::kNone;
}

}  // namespace guide_tree

namespace {

using namespace guide_tree;

constexpr int kMaxRepeat = 256;
constexpr size_t kMaxSubsetStates = 2048;  // before minimisation; a larger automaton is refused as too large

ByteSet Ascii() { return Range(0, 127); }
ByteSet Digits() { return Range('0', '9'); }
ByteSet WordChars() { return Range('a', 'z') | Range('A', 'Z') | Range('0', '9') | Range('_', '_'); }
ByteSet Spaces() {
    ByteSet s;
    for (char ch : {' ', '\t', '\n', '\r', '\f', '\v'}) s.set((size_t)(uint8_t)ch);
    return s;
}

class Parser {
public:
    Parser(const std::string& p, std::string* err) : p_(p), err_(err) {}

    NodePtr Parse() {
        NodePtr n = Alt();
        if (!n) return nullptr;
        if (pos_ < p_.size()) return Fail("unmatched ')'");   // Alt() stops only there
        return n;
    }

private:
    NodePtr Fail(const std::string& what) {
        if (err_->empty()) *err_ = what + " at offset " + std::to_string(pos_);
        return nullptr;
    }
    bool More() const { return pos_ < p_.size(); }
    uint8_t Peek() const { return (uint8_t)p_[pos_]; }

    NodePtr Alt() {
        NodePtr first = Cat();
        if (!first) return nullptr;
        if (!More() || Peek() != '|') return first;
        NodePtr alt(new Node());
        alt->type = Node::ALT;
        alt->kids.push_back(std::move(first));
        while (More() && Peek() == '|') {
            ++pos_;
            NodePtr next = Cat();
            if (!next) return nullptr;
            alt->kids.push_back(std::move(next));
        }
        return alt;
    }

    NodePtr Cat() {
        NodePtr cat(new Node());
        cat->type = Node::CAT;
        while (More() && Peek() != '|' && Peek() != ')') {
            NodePtr atom = Atom();
            if (!atom) return nullptr;
            atom = Quantified(std::move(atom));
            if (!atom) return nullptr;
            cat->kids.push_back(std::move(atom));
        }
        if (cat->kids.empty()) cat->type = Node::EMPTY;
        return cat;
    }

    // {m} {m,} {m,n} at pos_: true and the position behind it; false (nothing consumed) when the text is no well-formed quantifier
    bool Braces(int* lo, int* hi, bool* refused) {
        size_t i = pos_ + 1;
        auto number = [&](int* v) {
            const size_t begin = i;
            int64_t x = 0;
            while (i < p_.size() && p_[i] >= '0' && p_[i] <= '9' && i - begin < 9) x = x * 10 + (p_[i++] - '0');
            *v = (int)x;
            return i > begin;
        };
        if (i < p_.size() && p_[i] == ',') {   // {,n}: not in the dialect, and no literal either where another engine repeats
            *refused = true;
            return false;
        }
        if (!number(lo)) return false;
        if (i < p_.size() && p_[i] == '}') { *hi = *lo; pos_ = i + 1; return true; }
        if (i >= p_.size() || p_[i] != ',') return false;
        ++i;
        if (i < p_.size() && p_[i] == '}') { *hi = -1; pos_ = i + 1; return true; }
        if (!number(hi)) return false;
        if (i >= p_.size() || p_[i] != '}') return false;
        pos_ = i + 1;
        return true;
    }

    NodePtr Quantified(NodePtr atom) {
        if (!More()) return atom;
        int lo = 0, hi = 0;
        const uint8_t c = Peek();
        if (c == '*') { lo = 0; hi = -1; ++pos_; }
        else if (c == '+') { lo = 1; hi = -1; ++pos_; }
        else if (c == '?') { lo = 0; hi = 1; ++pos_; }
        else if (c == '{') {
            bool refused = false;
            if (!Braces(&lo, &hi, &refused)) {
                if (refused) return Fail("quantifier {,n} is not supported: write {0,n}");
                return atom;   // a literal '{': the next atom
            }
            if (lo > kMaxRepeat || hi > kMaxRepeat) return Fail("repetition count above " + std::to_string(kMaxRepeat));
            if (hi != -1 && hi < lo) return Fail("repetition {m,n} with n < m");
        } else {
            return atom;
        }
        if (More() && (Peek() == '?' || Peek() == '+')) return Fail("lazy and possessive quantifiers are not supported");
        if (More() && (Peek() == '*' || (Peek() == '{' && IsBraces()))) return Fail("a quantifier behind a quantifier");
        NodePtr rep(new Node());
        rep->type = Node::REPEAT;
        rep->min = lo;
        rep->max = hi;
        rep->kids.push_back(std::move(atom));
        return rep;
    }

    bool IsBraces() {
        const size_t keep = pos_;
        int lo, hi;
        bool refused = false;
        const bool yes = Braces(&lo, &hi, &refused);
        pos_ = keep;
        return yes || refused;
    }

    static int Hex(uint8_t c) {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return -1;
    }

    // behind a backslash (pos_ at the escaped character): a set (class shorthands) or one byte.  in_class: no anchors to report
    bool Escape(ByteSet* set) {
        if (!More()) { Fail("pattern ends in a backslash"); return false; }
        const uint8_t c = Peek();
        ++pos_;
        switch (c) {
            case 'd': *set = Digits(); return true;
            case 'w': *set = WordChars(); return true;
            case 's': *set = Spaces(); return true;
            case 'D': *set = Ascii() & ~Digits(); return true;
            case 'W': *set = Ascii() & ~WordChars(); return true;
            case 'S': *set = Ascii() & ~Spaces(); return true;
            case 'n': *set = Range('\n', '\n'); return true;
            case 't': *set = Range('\t', '\t'); return true;
            case 'r': *set = Range('\r', '\r'); return true;
            case 'x': {
                if (pos_ + 2 > p_.size() || Hex((uint8_t)p_[pos_]) < 0 || Hex((uint8_t)p_[pos_ + 1]) < 0) {
                    Fail("\\x needs two hex digits");
                    return false;
                }
                const int v = Hex((uint8_t)p_[pos_]) * 16 + Hex((uint8_t)p_[pos_ + 1]);
                pos_ += 2;
                *set = Range(v, v);
                return true;
            }
            default: break;
        }
        --pos_;
        if (c == 'b' || c == 'B' || c == 'A' || c == 'Z' || c == 'z') { Fail("anchors are not supported (the pattern is anchored at both ends)"); return false; }
        if (c >= '0' && c <= '9') { Fail("backreferences and octal escapes are not supported"); return false; }
        if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c >= 0x80) { Fail(std::string("unknown escape \\") + (char)c); return false; }
        ++pos_;
        *set = Range(c, c);   // an escaped metacharacter or other ASCII punctuation: itself
        return true;
    }

    // a UTF-8 character at pos_ as a concatenation of its bytes
    NodePtr Utf8() {
        const uint8_t c = Peek();
        const int n = (c & 0xE0) == 0xC0 ? 2 : (c & 0xF0) == 0xE0 ? 3 : (c & 0xF8) == 0xF0 ? 4 : 0;
        if (n == 0 || pos_ + (size_t)n > p_.size()) return Fail("invalid UTF-8 in the pattern");
        uint32_t cp = c & (0xFF >> (n + 1));
        for (int i = 1; i < n; ++i) {
            const uint8_t cc = (uint8_t)p_[pos_ + (size_t)i];
            if ((cc & 0xC0) != 0x80) return Fail("invalid UTF-8 in the pattern");
            cp = (cp << 6) | (cc & 0x3F);
        }
        static const uint32_t kMin[5] = {0, 0, 0x80, 0x800, 0x10000};
        if (cp < kMin[n] || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return Fail("invalid UTF-8 in the pattern");
        NodePtr cat(new Node());
        cat->type = Node::CAT;
        for (int i = 0; i < n; ++i) {
            const uint8_t cc = (uint8_t)p_[pos_ + (size_t)i];
            cat->kids.push_back(MakeSet(Range(cc, cc)));
        }
        pos_ += (size_t)n;
        return cat;
    }

    NodePtr Class() {   // pos_ behind '['
        bool negate = false;
        if (More() && Peek() == '^') { negate = true; ++pos_; }
        ByteSet set;
        bool first = true;
        while (true) {
            if (!More()) return Fail("unterminated class");
            uint8_t c = Peek();
            if (c == ']' && !first) { ++pos_; break; }
            first = false;
            ByteSet item;
            bool single = true;   // one byte: may begin a range
            if (c >= 0x80) return Fail("a non-ASCII character inside a class is not supported");
            ++pos_;
            if (c == '\\') {
                if (!Escape(&item)) return nullptr;
                single = item.count() == 1;
            } else {
                item = Range(c, c);
            }
            if (single && pos_ + 1 < p_.size() && p_[pos_] == '-' && p_[pos_ + 1] != ']') {
                ++pos_;
                uint8_t d = Peek();
                if (d >= 0x80) return Fail("a non-ASCII character inside a class is not supported");
                ++pos_;
                ByteSet end = Range(d, d);
                if (d == '\\') {
                    if (!Escape(&end)) return nullptr;
                    if (end.count() != 1) return Fail("a class shorthand as the end of a range");
                }
                int lo = 0, hi = 0;
                while (!item.test((size_t)lo)) ++lo;
                while (!end.test((size_t)hi)) ++hi;
                if (hi < lo) return Fail("a range that runs backwards");
                item = Range(lo, hi);
            }
            set |= item;
        }
        if (negate) set = Ascii() & ~set;
        return MakeSet(set);
    }

    NodePtr Atom() {
        const uint8_t c = Peek();
        switch (c) {
            case '(': {
                ++pos_;
                if (More() && Peek() == '?') {
                    if (pos_ + 1 < p_.size() && p_[pos_ + 1] == ':') pos_ += 2;
                    else return Fail("lookaround, named groups and inline flags are not supported: only ( ) and (?: )");
                }
                NodePtr inner = Alt();
                if (!inner) return nullptr;
                if (!More() || Peek() != ')') return Fail("unterminated group");
                ++pos_;
                return inner;
            }
            case '[': ++pos_; return Class();
            case '.': ++pos_; return MakeSet(Ascii() & ~Range('\n', '\n'));
            case '^': case '$': return Fail("anchors are not supported (the pattern is anchored at both ends)");
            case '*': case '+': case '?': return Fail("nothing to repeat");
            case '\\': {
                ++pos_;
                ByteSet set;
                if (!Escape(&set)) return nullptr;
                return MakeSet(set);
            }
            default: break;
        }
        if (c >= 0x80) return Utf8();
        ++pos_;
        return MakeSet(Range(c, c));
    }

    const std::string& p_;
    std::string* err_;
    size_t pos_ = 0;
};

}  // namespace

bool CompileGuideRegex(const std::string& pattern, GuideDfa* dfa, std::string* err) {
    err->clear();
    Parser parser(pattern, err);
    NodePtr root = parser.Parse();
    if (!root) {
        *err = "guide_regex: " + *err;
        return false;
    }
    Automaton a;
    switch (BuildAutomaton(*root, kMaxSubsetStates, &a)) {
        case BuildError::kNfaTooLarge:
            *err = "guide_regex: the pattern's counted repetitions expand to more than " + std::to_string(kMaxNfaStates) + " NFA states";
            return false;
        case BuildError::kSubsetTooLarge:
            *err = "guide_regex: the automaton has more than " + std::to_string(kMaxSubsetStates) +
                   " states before minimisation; at most " + std::to_string(GuideDfa::kMaxStates) + " are supported";
            return false;
        case BuildError::kEmptyLanguage:
            *err = "guide_regex: the pattern matches nothing (empty language)";
            return false;
        case BuildError::kNone: break;
    }
    if (a.n_states > GuideDfa::kMaxStates) {
        *err = "guide_regex: the minimal automaton has " + std::to_string(a.n_states) + " states; at most " +
               std::to_string(GuideDfa::kMaxStates) + " are supported";
        return false;
    }
    dfa->n_states = a.n_states;
    dfa->trans.resize(a.next.size());
    for (size_t i = 0; i < a.next.size(); ++i) dfa->trans[i] = a.next[i] < 0 ? (uint8_t)GuideDfa::kDead : (uint8_t)a.next[i];
    dfa->accept = a.accept;
    return true;
}

}}  // namespace ppl::llm
