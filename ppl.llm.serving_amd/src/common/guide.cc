#include "guide.h"

#include <algorithm>
#include <bitset>
#include <deque>
#include <map>
#include <memory>

namespace ppl { namespace llm {

namespace {

typedef std::bitset<256> ByteSet;

constexpr int kMaxRepeat = 256;
constexpr size_t kMaxNfaStates = 200000;   // counted repetitions copy their operand
constexpr size_t kMaxSubsetStates = 2048;  // before minimisation; a larger automaton is refused as too large

struct Node {
    enum Type { EMPTY, SET, CAT, ALT, REPEAT } type = EMPTY;
    ByteSet set;
    std::vector<std::unique_ptr<Node>> kids;
    int min = 0, max = 0;   // REPEAT: max -1 = unbounded
};
typedef std::unique_ptr<Node> NodePtr;

NodePtr MakeSet(const ByteSet& s) {
    NodePtr n(new Node());
    n->type = Node::SET;
    n->set = s;
    return n;
}

ByteSet Range(int lo, int hi) {
    ByteSet s;
    for (int b = lo; b <= hi; ++b) s.set((size_t)b);
    return s;
}
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

}  // namespace

bool CompileGuideRegex(const std::string& pattern, GuideDfa* dfa, std::string* err) {
    err->clear();
    Parser parser(pattern, err);
    NodePtr root = parser.Parse();
    if (!root) {
        *err = "guide_regex: " + *err;
        return false;
    }
    Nfa nfa;
    const auto whole = nfa.Build(*root);
    if (nfa.too_large) {
        *err = "guide_regex: the pattern's counted repetitions expand to more than " + std::to_string(kMaxNfaStates) + " NFA states";
        return false;
    }
    const int final_state = whole.second;

    // subset construction
    std::vector<std::vector<int>> subsets;
    std::map<std::vector<int>, int> ids;
    std::vector<std::vector<int>> next;   // [state][256], -1 = no NFA state left
    std::vector<uint8_t> mark(nfa.st.size(), 0);
    std::vector<int> start(1, whole.first);
    Closure(nfa, &start, &mark);
    ids[start] = 0;
    subsets.push_back(start);
    for (size_t i = 0; i < subsets.size(); ++i) {
        next.emplace_back(256, -1);
        // only the states with a byte edge matter
        std::vector<int> edges;
        for (int s : subsets[i])
            if (nfa.st[(size_t)s].to >= 0) edges.push_back(s);
        for (int b = 0; b < 256; ++b) {
            std::vector<int> to;
            for (int s : edges)
                if (nfa.st[(size_t)s].set.test((size_t)b)) to.push_back(nfa.st[(size_t)s].to);
            if (to.empty()) continue;
            std::sort(to.begin(), to.end());
            to.erase(std::unique(to.begin(), to.end()), to.end());
            Closure(nfa, &to, &mark);
            auto it = ids.find(to);
            if (it == ids.end()) {
                if (subsets.size() >= kMaxSubsetStates) {
                    *err = "guide_regex: the automaton has more than " + std::to_string(kMaxSubsetStates) +
                           " states before minimisation; at most " + std::to_string(GuideDfa::kMaxStates) + " are supported";
                    return false;
                }
                it = ids.emplace(to, (int)subsets.size()).first;
                subsets.push_back(to);
            }
            next[i][(size_t)b] = it->second;
        }
    }
    const int n = (int)subsets.size();
    std::vector<uint8_t> acc((size_t)n, 0);
    for (int i = 0; i < n; ++i) acc[(size_t)i] = std::binary_search(subsets[(size_t)i].begin(), subsets[(size_t)i].end(), final_state);

    // trim: a state that reaches no accepting state is dead
    std::vector<std::vector<int>> rev((size_t)n);
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < 256; ++b)
            if (next[(size_t)i][(size_t)b] >= 0) rev[(size_t)next[(size_t)i][(size_t)b]].push_back(i);
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
    if (!live[0]) {
        *err = "guide_regex: the pattern matches nothing (empty language)";
        return false;
    }
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < 256; ++b)
            if (next[(size_t)i][(size_t)b] >= 0 && !live[(size_t)next[(size_t)i][(size_t)b]]) next[(size_t)i][(size_t)b] = -1;

    // minimise by partition refinement (Moore): the class of a live state, -1 for the dead one; refined by the classes of its 256 successors
    std::vector<int> cls((size_t)n, -1);
    for (int i = 0; i < n; ++i)
        if (live[(size_t)i]) cls[(size_t)i] = acc[(size_t)i] ? 1 : 0;
    int n_cls = 0;
    while (true) {
        std::map<std::vector<int>, int> sig_ids;
        std::vector<int> fresh((size_t)n, -1);
        std::vector<int> sig(257);
        for (int i = 0; i < n; ++i) {
            if (!live[(size_t)i]) continue;
            sig[0] = cls[(size_t)i];
            for (int b = 0; b < 256; ++b) {
                const int to = next[(size_t)i][(size_t)b];
                sig[(size_t)b + 1] = to < 0 ? -1 : cls[(size_t)to];
            }
            fresh[(size_t)i] = sig_ids.emplace(sig, (int)sig_ids.size()).first->second;
        }
        const int count = (int)sig_ids.size();
        cls.swap(fresh);
        if (count == n_cls) break;
        n_cls = count;
    }

    // number the classes breadth-first from the start, bytes ascending
    std::vector<int> rep((size_t)n_cls, -1), order((size_t)n_cls, -1);
    for (int i = n - 1; i >= 0; --i)
        if (live[(size_t)i]) rep[(size_t)cls[(size_t)i]] = i;
    std::vector<int> bfs;
    order[(size_t)cls[0]] = 0;
    bfs.push_back(cls[0]);
    for (size_t i = 0; i < bfs.size(); ++i) {
        const int r = rep[(size_t)bfs[i]];
        for (int b = 0; b < 256; ++b) {
            const int to = next[(size_t)r][(size_t)b];
            if (to < 0 || order[(size_t)cls[(size_t)to]] >= 0) continue;
            order[(size_t)cls[(size_t)to]] = (int)bfs.size();
            bfs.push_back(cls[(size_t)to]);
        }
    }
    const int live_states = (int)bfs.size();
    if (live_states > GuideDfa::kMaxStates) {
        *err = "guide_regex: the minimal automaton has " + std::to_string(live_states) + " states; at most " +
               std::to_string(GuideDfa::kMaxStates) + " are supported";
        return false;
    }
    dfa->n_states = live_states;
    dfa->trans.assign((size_t)live_states * 256, (uint8_t)GuideDfa::kDead);
    dfa->accept.assign((size_t)live_states, 0);
    for (int k = 0; k < live_states; ++k) {
        const int r = rep[(size_t)bfs[(size_t)k]];
        dfa->accept[(size_t)k] = acc[(size_t)r];
        for (int b = 0; b < 256; ++b) {
            const int to = next[(size_t)r][(size_t)b];
            if (to >= 0) dfa->trans[(size_t)k * 256 + (size_t)b] = (uint8_t)order[(size_t)cls[(size_t)to]];
        }
    }
    return true;
}

}}  // namespace ppl::llm
