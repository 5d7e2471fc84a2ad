#include "guide_json.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../utils/mini_json.h"
#include "guide_tree.h"

namespace ppl { namespace llm {

namespace {

using namespace guide_tree;
using utils::JsonValue;

constexpr int kMaxBound = 256;
// the syntax tree of a schema: an array keeps its item twice, an object a member once per member that may come first, and a $ref is
// expanded at every use, so the tree can double with every level of nesting.  Nothing is copied or descended into beyond this many nodes
// (more would pass the NFA builder's cap of as many states anyway, except where a repetition runs zero times)
constexpr size_t kMaxTreeNodes = kMaxNfaStates;

const char* const kTypes[] = {"object", "string", "integer", "number", "boolean", "null", "array"};
const char* const kAnnotations[] = {"title", "description", "default", "examples", "$schema", "$id", "format", "$defs", "definitions"};
const char* const kConstraints[] = {"type", "properties", "required", "additionalProperties", "items", "minItems", "maxItems",
                                    "minLength", "maxLength", "enum", "const", "anyOf", "$ref"};

template <size_t N>
bool Among(const char* const (&list)[N], const std::string& s) {
    for (const char* w : list)
        if (s == w) return true;
    return false;
}

NodePtr Opt(NodePtr n) { return MakeRepeat(std::move(n), 0, 1); }
NodePtr Byte(char c) { return MakeSet(Range((uint8_t)c, (uint8_t)c)); }
NodePtr Space() { return Opt(Byte(' ')); }
NodePtr Digit() { return MakeSet(Range('0', '9')); }

template <typename... T>
NodePtr Cat(T... kids) {
    std::vector<NodePtr> v;
    (v.push_back(std::move(kids)), ...);
    return MakeCat(std::move(v));
}

// one character of a JSON string: an unescaped ASCII character, an escape, or a well-formed UTF-8 sequence of 2 .. 4 bytes
NodePtr Char() {
    ByteSet plain = Range(0x20, 0x7F);
    plain.reset('"');
    plain.reset('\\');
    ByteSet simple, hex = Range('0', '9') | Range('a', 'f') | Range('A', 'F');
    for (char c : {'"', '\\', '/', 'b', 'f', 'n', 'r', 't'}) simple.set((size_t)(uint8_t)c);
    auto cont = [] { return MakeSet(Range(0x80, 0xBF)); };
    auto set = [](int lo, int hi) { return MakeSet(Range(lo, hi)); };
    std::vector<NodePtr> alt;
    alt.push_back(MakeSet(plain));
    alt.push_back(Cat(Byte('\\'), MakeSet(simple)));
    // \uXXXX outside the surrogates (D800 .. DFFF), or a high surrogate with its low one: one character either way.  A lone escaped
    // surrogate is left out: with it a pair could also count as two characters, and minLength would admit too short a string
    auto one = [](const char* chars) {
        ByteSet s;
        for (const char* c = chars; *c; ++c) s.set((size_t)(uint8_t)*c);
        return MakeSet(s);
    };
    auto hexes = [&](int n) { return MakeRepeat(MakeSet(hex), n, n); };
    std::vector<NodePtr> code;
    code.push_back(Cat(one("0123456789abcefABCEF"), hexes(3)));
    code.push_back(Cat(one("dD"), one("01234567"), hexes(2)));
    code.push_back(Cat(one("dD"), one("89abAB"), hexes(2), MakeLiteral("\\u"), one("dD"), one("cdefCDEF"), hexes(2)));
    alt.push_back(Cat(MakeLiteral("\\u"), MakeAlt(std::move(code))));
    alt.push_back(Cat(set(0xC2, 0xDF), cont()));                              // U+0080 .. U+07FF (C0, C1: overlong)
    alt.push_back(Cat(set(0xE0, 0xE0), set(0xA0, 0xBF), cont()));             // U+0800 .. (E0 80-9F: overlong)
    alt.push_back(Cat(set(0xE1, 0xEC), cont(), cont()));
    alt.push_back(Cat(set(0xED, 0xED), set(0x80, 0x9F), cont()));             // (ED A0-BF: the surrogates)
    alt.push_back(Cat(set(0xEE, 0xEF), cont(), cont()));
    alt.push_back(Cat(set(0xF0, 0xF0), set(0x90, 0xBF), cont(), cont()));     // U+10000 .. (F0 80-8F: overlong)
    alt.push_back(Cat(set(0xF1, 0xF3), cont(), cont(), cont()));
    alt.push_back(Cat(set(0xF4, 0xF4), set(0x80, 0x8F), cont(), cont()));     // .. U+10FFFF
    return MakeAlt(std::move(alt));
}

NodePtr Integer() {
    std::vector<NodePtr> alt;
    alt.push_back(Byte('0'));
    alt.push_back(Cat(MakeSet(Range('1', '9')), MakeRepeat(Digit(), 0, 17)));
    return Cat(Opt(Byte('-')), MakeAlt(std::move(alt)));
}

NodePtr Number() {
    ByteSet e, sign;
    e.set('e'); e.set('E');
    sign.set('+'); sign.set('-');
    return Cat(Integer(), Opt(Cat(Byte('.'), MakeRepeat(Digit(), 1, 17))),
               Opt(Cat(MakeSet(e), Opt(MakeSet(sign)), MakeRepeat(Digit(), 1, 3))));
}

bool ValidUtf8(const std::string& s) {
    for (size_t i = 0; i < s.size();) {
        const uint8_t c = (uint8_t)s[i];
        if (c < 0x80) { ++i; continue; }
        const int n = (c & 0xE0) == 0xC0 ? 2 : (c & 0xF0) == 0xE0 ? 3 : (c & 0xF8) == 0xF0 ? 4 : 0;
        if (n == 0 || i + (size_t)n > s.size()) return false;
        uint32_t cp = c & (0xFF >> (n + 1));
        for (int k = 1; k < n; ++k) {
            const uint8_t cc = (uint8_t)s[i + (size_t)k];
            if ((cc & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (cc & 0x3F);
        }
        static const uint32_t kMin[5] = {0, 0, 0x80, 0x800, 0x10000};
        if (cp < kMin[n] || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
        i += (size_t)n;
    }
    return true;
}

// the canonical text of a string: the short escapes where JSON has one, \u00XX for the other control bytes, everything else as it is
std::string StringText(const std::string& s) {
    std::string out = "\"";
    for (unsigned char c : s) {
        switch (c) {
            case '"': out += "\\\""; break;
            case '\\': out += "\\\\"; break;
            case '\b': out += "\\b"; break;
            case '\f': out += "\\f"; break;
            case '\n': out += "\\n"; break;
            case '\r': out += "\\r"; break;
            case '\t': out += "\\t"; break;
            default:
                if (c < 0x20) {
                    char buf[8];
                    snprintf(buf, sizeof(buf), "\\u%04x", c);
                    out += buf;
                } else {
                    out.push_back((char)c);
                }
        }
    }
    return out + "\"";
}

bool Integral(double x) { return x == floor(x) && fabs(x) < 1e15; }

// the canonical text of a number: an integer without a fraction, anything else with the fewest digits that read back as the same double
std::string NumberText(double x) {
    char buf[40];
    if (Integral(x)) {
        snprintf(buf, sizeof(buf), "%lld", (long long)x);
        return buf;
    }
    for (int p = 1; p <= 17; ++p) {
        snprintf(buf, sizeof(buf), "%.*g", p, x);
        if (strtod(buf, nullptr) == x) break;
    }
    return buf;
}

class Compiler {
public:
    explicit Compiler(const JsonValue& root) : root_(root) {}
    std::string err;

    NodePtr Document() {
        NodePtr v = Value(root_, "#");
        if (!v) return nullptr;
        return Cat(Space(), std::move(v));
    }

private:
    NodePtr Fail(const std::string& what) {
        if (err.empty()) err = what;
        return nullptr;
    }
    static std::string At(const std::string& ptr, const std::string& key) { return "'" + key + "' at " + ptr + "/" + key; }

    // the tree has outgrown its budget: refused at the keyword whose operand was about to be built or copied once more
    bool TooLarge(const std::string& ptr, const std::string& key) {
        if (NodeCount() <= kMaxTreeNodes) return false;
        Fail("the schema expands to more than " + std::to_string(kMaxTreeNodes) + " syntax nodes at " + At(ptr, key) +
             ": it nests too deeply");
        return true;
    }

    // every keyword of s other than `allowed` and the annotations is a constraint that `key` cannot stand beside
    bool Alone(const JsonValue& s, const std::string& ptr, const std::string& key, const std::vector<std::string>& allowed) {
        for (const auto& k : s.keys)
            if (k != key && !Among(kAnnotations, k) && std::find(allowed.begin(), allowed.end(), k) == allowed.end()) {
                Fail(At(ptr, key) + " beside '" + k + "' is not supported: it must stand alone");
                return false;
            }
        return true;
    }

    // a length bound: -2 = refused
    int Bound(const JsonValue& s, const std::string& ptr, const char* key, int dflt) {
        const JsonValue* v = s.Find(key);
        if (!v) return dflt;
        if (v->type != JsonValue::NUMBER || v->num < 0 || v->num != floor(v->num)) {
            Fail(At(ptr, key) + " is not a non-negative integer");
            return -2;
        }
        if (v->num > kMaxBound) {
            Fail(At(ptr, key) + " is above " + std::to_string(kMaxBound));
            return -2;
        }
        return (int)v->num;
    }

    NodePtr Value(const JsonValue& s, const std::string& ptr) {
        if (s.type != JsonValue::OBJECT) return Fail("the schema at " + ptr + " is not an object");
        for (const auto& k : s.keys)
            if (!Among(kAnnotations, k) && !Among(kConstraints, k)) return Fail("keyword " + At(ptr, k) + " is not supported");
        if (const JsonValue* ref = s.Find("$ref")) return Ref(s, *ref, ptr);
        if (const JsonValue* any = s.Find("anyOf")) {
            if (!Alone(s, ptr, "anyOf", {})) return nullptr;
            if (any->type != JsonValue::ARRAY || any->arr.empty()) return Fail(At(ptr, "anyOf") + " is not a list of schemas: empty language");
            std::vector<NodePtr> alt;
            for (size_t i = 0; i < any->arr.size(); ++i) {
                if (TooLarge(ptr, "anyOf")) return nullptr;
                NodePtr v = Value(any->arr[i], ptr + "/anyOf/" + std::to_string(i));
                if (!v) return nullptr;
                alt.push_back(std::move(v));
            }
            return MakeAlt(std::move(alt));
        }
        std::vector<std::string> types;
        const JsonValue* type = s.Find("type");
        if (type) {
            if (type->type == JsonValue::STRING) types.push_back(type->str);
            else if (type->type == JsonValue::ARRAY)
                for (const auto& t : type->arr) {
                    if (t.type != JsonValue::STRING) return Fail(At(ptr, "type") + " is not a name or a list of names");
                    if (std::find(types.begin(), types.end(), t.str) == types.end()) types.push_back(t.str);
                }
            else return Fail(At(ptr, "type") + " is not a name or a list of names");
            for (const auto& t : types)
                if (!Among(kTypes, t)) return Fail(At(ptr, "type") + " names the unknown type '" + t + "'");
        }
        const char* en = s.Find("const") ? "const" : s.Find("enum") ? "enum" : nullptr;
        if (en) return Enum(s, ptr, en, type ? &types : nullptr);
        if (!type) return Fail("no 'type' at " + ptr + ": a schema without a type allows any value, which is recursive");
        if (types.empty()) return Fail(At(ptr, "type") + " is an empty list: empty language");
        std::vector<NodePtr> alt;
        for (const auto& t : types) {
            NodePtr v = Typed(t, s, ptr);
            if (!v) return nullptr;
            alt.push_back(std::move(v));
        }
        if (alt.size() == 1) return std::move(alt[0]);
        return MakeAlt(std::move(alt));
    }

    NodePtr Ref(const JsonValue& s, const JsonValue& ref, const std::string& ptr) {
        if (!Alone(s, ptr, "$ref", {})) return nullptr;
        if (ref.type != JsonValue::STRING) return Fail(At(ptr, "$ref") + " is not a string");
        const JsonValue* target = nullptr;
        for (const char* base : {"$defs", "definitions"}) {
            const std::string prefix = std::string("#/") + base + "/";
            if (ref.str.compare(0, prefix.size(), prefix) != 0) continue;
            const JsonValue* defs = root_.Find(base);
            target = defs ? defs->Find(ref.str.substr(prefix.size())) : nullptr;
            if (!target) return Fail(At(ptr, "$ref") + ": nothing at " + ref.str);
        }
        if (!target) return Fail(At(ptr, "$ref") + " points to " + ref.str + ": only #/$defs/NAME and #/definitions/NAME are supported");
        if (std::find(stack_.begin(), stack_.end(), target) != stack_.end())
            return Fail("recursive " + At(ptr, "$ref") + " to " + ref.str + ": recursion is not a regular language");
        if (TooLarge(ptr, "$ref")) return nullptr;
        stack_.push_back(target);
        NodePtr v = Value(*target, ref.str);
        stack_.pop_back();
        return v;
    }

    static bool Scalar(const JsonValue& v) { return v.type != JsonValue::ARRAY && v.type != JsonValue::OBJECT; }
    static bool HasType(const JsonValue& v, const std::vector<std::string>& types) {
        for (const auto& t : types) {
            if (t == "null" && v.type == JsonValue::NUL) return true;
            if (t == "boolean" && v.type == JsonValue::BOOL) return true;
            if (t == "string" && v.type == JsonValue::STRING) return true;
            if (t == "number" && v.type == JsonValue::NUMBER) return true;
            if (t == "integer" && v.type == JsonValue::NUMBER && Integral(v.num)) return true;
        }
        return false;
    }

    NodePtr Enum(const JsonValue& s, const std::string& ptr, const char* key, const std::vector<std::string>* types) {
        if (!Alone(s, ptr, key, {"type"})) return nullptr;
        const JsonValue& e = *s.Find(key);
        std::vector<const JsonValue*> values;
        if (std::string(key) == "const") values.push_back(&e);
        else if (e.type != JsonValue::ARRAY) return Fail(At(ptr, key) + " is not a list");
        else
            for (const auto& v : e.arr) values.push_back(&v);
        std::vector<std::string> texts;
        for (const JsonValue* v : values) {
            if (!Scalar(*v)) return Fail(At(ptr, key) + " holds a non-scalar: only strings, numbers, booleans and null are supported");
            if (types && !HasType(*v, *types)) continue;
            std::string text;
            switch (v->type) {
                case JsonValue::NUL: text = "null"; break;
                case JsonValue::BOOL: text = v->b ? "true" : "false"; break;
                case JsonValue::NUMBER:
                    if (!isfinite(v->num)) return Fail(At(ptr, key) + " holds a number that is not finite (it has no JSON text)");
                    text = NumberText(v->num);
                    break;
                default:
                    if (!ValidUtf8(v->str)) return Fail(At(ptr, key) + " holds a string that is not well-formed UTF-8");
                    text = StringText(v->str);
            }
            if (std::find(texts.begin(), texts.end(), text) == texts.end()) texts.push_back(text);
        }
        if (texts.empty()) return Fail(At(ptr, key) + " leaves no value: empty language");
        std::vector<NodePtr> alt;
        for (const auto& t : texts) alt.push_back(MakeLiteral(t));
        if (alt.size() == 1) return std::move(alt[0]);
        return MakeAlt(std::move(alt));
    }

    NodePtr Typed(const std::string& t, const JsonValue& s, const std::string& ptr) {
        if (t == "null") return MakeLiteral("null");
        if (t == "boolean") {
            std::vector<NodePtr> alt;
            alt.push_back(MakeLiteral("true"));
            alt.push_back(MakeLiteral("false"));
            return MakeAlt(std::move(alt));
        }
        if (t == "integer") return Integer();
        if (t == "number") return Number();
        if (t == "string") {
            const int lo = Bound(s, ptr, "minLength", 0), hi = Bound(s, ptr, "maxLength", -1);
            if (lo == -2 || hi == -2) return nullptr;
            if (hi != -1 && lo > hi) return Fail(At(ptr, "minLength") + " is above maxLength: empty language");
            return Cat(Byte('"'), MakeRepeat(Char(), lo, hi), Byte('"'));
        }
        if (t == "array") return Array(s, ptr);
        return Object(s, ptr);
    }

    static NodePtr Comma() { return Cat(Byte(','), Space()); }

    NodePtr Array(const JsonValue& s, const std::string& ptr) {
        const int lo = Bound(s, ptr, "minItems", 0), hi = Bound(s, ptr, "maxItems", -1);
        if (lo == -2 || hi == -2) return nullptr;
        if (hi != -1 && lo > hi) return Fail(At(ptr, "minItems") + " is above maxItems: empty language");
        if (hi == 0) return MakeLiteral("[]");
        const JsonValue* items = s.Find("items");
        if (!items) return Fail("no 'items' at " + ptr + ": an array of any value is recursive");
        NodePtr item = Value(*items, ptr + "/items");
        if (!item) return nullptr;
        if (TooLarge(ptr, "items")) return nullptr;
        NodePtr body;
        if (hi == 1) {   // nothing follows the one item
            body = std::move(item);
        } else {
            NodePtr more = MakeRepeat(Cat(Comma(), Clone(*item)), std::max(lo - 1, 0), hi == -1 ? -1 : hi - 1);
            body = Cat(std::move(item), std::move(more));
        }
        if (lo == 0) body = Opt(std::move(body));
        return Cat(Byte('['), std::move(body), Byte(']'));
    }

    NodePtr Object(const JsonValue& s, const std::string& ptr) {
        static const JsonValue kNone;
        const JsonValue* props = s.Find("properties");
        if (props && props->type != JsonValue::OBJECT) return Fail(At(ptr, "properties") + " is not an object");
        if (!props) props = &kNone;
        std::vector<std::string> required;
        if (const JsonValue* r = s.Find("required")) {
            if (r->type != JsonValue::ARRAY) return Fail(At(ptr, "required") + " is not a list of names");
            for (const auto& name : r->arr) {
                if (name.type != JsonValue::STRING) return Fail(At(ptr, "required") + " is not a list of names");
                if (!props->Find(name.str))
                    return Fail(At(ptr, "required") + " names '" + name.str + "', which 'properties' does not declare: empty language");
                required.push_back(name.str);
            }
        }
        const size_t n = props->keys.size();
        std::vector<NodePtr> member(n);
        std::vector<bool> req(n);
        for (size_t i = 0; i < n; ++i) {
            const std::string& key = props->keys[i];
            if (!ValidUtf8(key)) return Fail(At(ptr, "properties") + " has a name that is not well-formed UTF-8");
            NodePtr v = Value(*props->Find(key), ptr + "/properties/" + key);
            if (!v) return nullptr;
            if (TooLarge(ptr, "properties")) return nullptr;
            member[i] = Cat(MakeLiteral(StringText(key) + ":"), Space(), std::move(v));
            req[i] = std::find(required.begin(), required.end(), key) != required.end();
        }
        // behind a member: every later one with its comma, the optional ones optionally
        auto behind = [&](size_t i) {
            std::vector<NodePtr> cat;
            for (size_t j = i; j < n && NodeCount() <= kMaxTreeNodes; ++j) {
                NodePtr m = Cat(Comma(), Clone(*member[j]));
                cat.push_back(req[j] ? std::move(m) : Opt(std::move(m)));
            }
            return MakeCat(std::move(cat));
        };
        // the first member is the first required one or any optional one in front of it; no member at all where nothing is required
        std::vector<NodePtr> first;
        bool may_be_empty = true;
        for (size_t i = 0; i < n; ++i) {
            if (TooLarge(ptr, "properties")) return nullptr;
            first.push_back(Cat(Clone(*member[i]), behind(i + 1)));
            if (req[i]) { may_be_empty = false; break; }
        }
        if (TooLarge(ptr, "properties")) return nullptr;
        if (may_be_empty) first.push_back(MakeEmpty());
        return Cat(Byte('{'), MakeAlt(std::move(first)), Byte('}'));
    }

    const JsonValue& root_;
    std::vector<const JsonValue*> stack_;   // the $ref targets being expanded
};

}  // namespace

bool CompileGuideJsonSchema(const std::string& schema, GuideDfa16* dfa, std::string* err) {
    err->clear();
    JsonValue root;
    utils::JsonParser parser(schema);
    if (!parser.Parse(&root)) {
        *err = "guide_json_schema: the schema is not valid JSON";
        return false;
    }
    ResetNodeCount();
    Compiler compiler(root);
    NodePtr tree = compiler.Document();
    if (!tree) {
        *err = "guide_json_schema: " + compiler.err;
        return false;
    }
    Automaton a;
    switch (BuildAutomaton(*tree, kGuideJsonMaxSubsetStates, &a)) {
        case BuildError::kNfaTooLarge:
            *err = "guide_json_schema: the schema's bounded repetitions expand to more than " + std::to_string(kMaxNfaStates) + " NFA states";
            return false;
        case BuildError::kSubsetTooLarge:
            *err = "guide_json_schema: the automaton has more than " + std::to_string(kGuideJsonMaxSubsetStates) +
                   " states before minimisation; at most " + std::to_string(GuideDfa16::kMaxStates) + " are supported after it";
            return false;
        case BuildError::kEmptyLanguage:
            *err = "guide_json_schema: the schema matches nothing (empty language)";
            return false;
        case BuildError::kNone: break;
    }
    if (a.n_states > GuideDfa16::kMaxStates) {
        *err = "guide_json_schema: the minimal automaton has " + std::to_string(a.n_states) + " states; at most " +
               std::to_string(GuideDfa16::kMaxStates) + " are supported";
        return false;
    }
    dfa->n_states = a.n_states;
    dfa->trans.resize(a.next.size());
    for (size_t i = 0; i < a.next.size(); ++i) dfa->trans[i] = a.next[i] < 0 ? (uint16_t)GuideDfa16::kDead : (uint16_t)a.next[i];
    dfa->accept = a.accept;
    return true;
}

}}  // namespace ppl::llm
