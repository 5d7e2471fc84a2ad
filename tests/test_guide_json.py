"""The JSON-schema guide compiler (src/common/guide_json.cc through build/guide_json_trace dfa).

Per schema: strings drawn from the automaton by seeded random walks to acceptance all parse as JSON and pass a small validator written
here; a hand list of valid documents in the fixed whitespace form is accepted; near-misses are refused at the byte that makes them wrong;
the automaton is trimmed and minimal (the checks of tests/test_guide_regex.py).  Every refusal comes with the keyword and its JSON pointer.
The limits: a schema of more than 255 and at most 4096 states compiles, one above 4096 is refused with both numbers, and guide_regex keeps
its own limit of 255."""
import json
import re

import numpy as np
import pytest

from tests import guide as G8
from tests import guide16 as G

STR = {"type": "string"}
INT = {"type": "integer"}

PERSON = {"type": "object", "properties": {
    "name": STR, "email": STR, "age": INT, "tags": {"type": "array", "items": STR},
    "address": {"type": "object", "properties": {"street": STR, "city": STR, "zip": STR}, "required": ["street", "city", "zip"]},
    "active": {"type": "boolean"}, "score": {"type": "number"}},
    "required": ["name", "email", "age", "tags", "address", "active", "score"]}

# (name, schema, valid documents, near-misses as (document, the offset of the first byte that is refused; len = it only ends too early))
CASES = [
    ("string", {"type": "string", "title": "a string", "description": "skipped", "default": "x", "examples": ["y"], "format": "email"},
     ['""', ' "abc"', '"é€😀"', r'"\"\\\/\b\f\n\r\té😀"', '"\x7f"'],
     [('"a\x01"', 2), ('"a\nb"', 2), (b'"\xed\xa0\x80"', 2), (b'"\xc0\xaf"', 1), (b'"\xe0\x80\xaf"', 2), (b'"\xf4\x90\x80\x80"', 2),
      (b'"\xf0\x80\x80\x80"', 2), (b'"\xf8"', 1), (b'"\x80"', 1), (r'"\x"', 2), (r'"\ud800"', 7), (r'"\udc00"', 4), ('  "a"', 1), ('"a" ', 3),
      ('"a', 2)]),
    ("string_bounds", {"type": "string", "minLength": 2, "maxLength": 3},
     ['"ab"', '"abc"', '"é€"', r'"\né"', '"😀a"', r'"\ud83d\ude00a"', r'"\u00e9\uD83D\uDE00\t"'],
     [('"a"', 2), ('"abcd"', 4), ('""', 1), ('"😀"', 5), (r'"\ud83d\ude00"', 13), ('"éé€a"', 8)]),
    ("integer", INT,
     ["0", "-0", "7", " 42", "-123456789012345678", "999999999999999999"],
     [("01", 1), ("-01", 2), ("1234567890123456789", 18), ("+1", 0), ("1.0", 1), ("1e3", 1), ("-", 1), ("", 0)]),
    ("number", {"type": "number"},
     ["0", "-0.5", "3.14159", "1e10", "1E-3", "2.5e+308", "0.12345678901234567"],
     [("01", 1), (".5", 0), ("1.", 2), ("1.e3", 2), ("1e", 2), ("1e1234", 5), ("0.123456789012345678", 19), ("1e+", 3), ("NaN", 0)]),
    ("scalars", {"type": ["boolean", "null", "integer"]},
     ["true", "false", "null", "12", " null"],
     [("True", 0), ("nul", 3), ("nulll", 4), ('"x"', 0)]),
    ("optional_everywhere", {"type": "object", "properties": {"a": INT, "b": INT, "c": INT, "d": INT}, "required": ["c"],
                             "additionalProperties": False},
     ['{"c": 1}', '{"a": 1, "c": 2}', '{"b":1,"c":2}', '{"a": 1, "b": 2, "c": 3, "d": 4}', '{"c": 3,"d": 4}', ' {"a":1,"c":3,"d":4}'],
     [('{}', 1), ('{"a": 1}', 7), ('{"a": 1, "d": 4}', 10), ('{"c": 1, "a": 2}', 10), ('{"c": 1,}', 8), ('{"c": 1, }', 9), ('{"c":  1}', 6),
      ('{"c" : 1}', 4), ('{ "c": 1}', 1), ('{"c": 1, "c": 2}', 10), ('{"e": 1}', 2), ('{"c": 1} ', 8)]),
    ("all_optional", {"type": "object", "properties": {"x": {"type": "boolean"}, "y": {"type": "null"}}},
     ['{}', '{"x": true}', '{"y": null}', '{"x": false, "y": null}'],
     [('{"y": null, "x": true}', 10), ('{,}', 1), ('{"x": true,}', 11)]),
    ("nested", {"type": "object", "properties": {"p": {"type": "object", "properties": {"q": {"type": "object", "properties": {"r": INT},
                                                                                                 "required": ["r"]}}, "required": ["q"]},
                                                  "s": STR}, "required": ["p", "s"]},
     ['{"p": {"q": {"r": 1}}, "s": "x"}', '{"p":{"q":{"r":-5}},"s":""}'],
     [('{"p": {"q": {}}, "s": "x"}', 13), ('{"s": "x", "p": {"q": {"r": 1}}}', 2), ('{"p": {"q": {"r": 1}}}', 21)]),
    ("array_bounds", {"type": "array", "items": INT, "minItems": 1, "maxItems": 3},
     ["[1]", "[1, 2]", "[1,2,3]", " [0, -1,2]"],
     [("[]", 1), ("[1, 2, 3, 4]", 8), ("[1,]", 3), ("[1 ,2]", 2), ("[1,  2]", 4), ("[ 1]", 1), ("[1, 2", 5)]),
    ("array_of_objects", {"type": "array", "items": {"type": "object", "properties": {"k": STR, "v": {"type": "number"}}, "required": ["k"]}},
     ["[]", '[{"k": "a"}]', '[{"k": "a", "v": 1.5}, {"k": "b"}]'],
     [('[{"v": 1}]', 3), ('[{"k": "a"},]', 12), ("[[]]", 1)]),
    ("any_of", {"anyOf": [{"type": "string", "maxLength": 2}, {"type": "array", "items": {"type": "boolean"}, "maxItems": 0}, {"const": 7}]},
     ['"ab"', "[]", "7", ' ""'],
     [('"abc"', 3), ("[true]", 1), ("8", 0), ("77", 1)]),
    ("refs", {"$schema": "https://json-schema.org/draft/2020-12/schema", "$id": "x", "type": "object",
              "properties": {"from": {"$ref": "#/$defs/point"}, "to": {"$ref": "#/definitions/pt"}},
              "required": ["from", "to"],
              "$defs": {"point": {"type": "object", "properties": {"x": INT, "y": INT}, "required": ["x", "y"]}},
              "definitions": {"pt": {"$ref": "#/$defs/point", "description": "through a second reference"}}},
     ['{"from": {"x": 1, "y": 2}, "to": {"x": 3, "y": 4}}'],
     [('{"from": {"x": 1}, "to": {"x": 3, "y": 4}}', 16), ('{"from": {"x": 1, "y": 2}}', 25)]),
    ("enums", {"type": "object", "properties": {
        "e": {"enum": ["plain", "q\"uo\\te", "tab\there", "é€😀", "", 3, 2.5, -1e-7, True, None]},
        "t": {"type": "string", "enum": ["s", 1, None]}, "c": {"const": "only"}}, "required": ["e", "t", "c"]},
     ['{"e": "plain", "t": "s", "c": "only"}', '{"e": "q\\"uo\\\\te", "t": "s", "c": "only"}', '{"e": "tab\\there", "t": "s", "c": "only"}',
      '{"e": "é€😀", "t": "s", "c": "only"}', '{"e": "", "t": "s", "c": "only"}', '{"e": 3, "t": "s", "c": "only"}',
      '{"e": 2.5, "t": "s", "c": "only"}', '{"e": -1e-07, "t": "s", "c": "only"}', '{"e": true, "t": "s", "c": "only"}',
      '{"e": null, "t": "s", "c": "only"}'],
     [('{"e": "plai", "t": "s", "c": "only"}', 11), ('{"e": 3.0, "t": "s", "c": "only"}', 7), ('{"e": 3, "t": 1, "c": "only"}', 14),
      ('{"e": 3, "t": null, "c": "only"}', 14), ('{"e": 3, "t": "s", "c": "onl"}', 28), ('{"e": "tab\there", "t": "s", "c": "only"}', 10),
      ('{"e": false, "t": "s", "c": "only"}', 6)]),
    ("person", PERSON,
     ['{"name": "Ada", "email": "a@b.c", "age": 36, "tags": ["x", "y"], "address": {"street": "1 Main", "city": "Z", "zip": "8000"}, '
      '"active": true, "score": 9.5}'],
     [('{"name": "Ada", "age": 36}', 17)]),
]
NAMES = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def compiled():
    return G.compile_schemas([c[1] for c in CASES])


def dfa(compiled, idx):
    rec = compiled[idx]
    assert rec["ok"] == 1, rec
    assert 1 <= rec["n_states"] <= G.MAX_STATES
    return rec["trans"], rec["accept"]


# ----------------------------------------------------------------------------------------------------------- the validator

def resolve(schema, root):
    while "$ref" in schema:
        base, name = schema["$ref"].split("/")[1:]
        schema = root[base][name]
    return schema


def has_type(v, t):
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    return isinstance(v, {"string": str, "array": list, "object": dict}[t])


def same(a, b):
    """JSON equality: true is not 1"""
    return type(a) is type(b) and a == b or (has_type(a, "number") and has_type(b, "number") and a == b)


def valid(v, schema, root):
    schema = resolve(schema, root)
    if "anyOf" in schema:
        return any(valid(v, s, root) for s in schema["anyOf"])
    if "const" in schema and not same(v, schema["const"]):
        return False
    if "enum" in schema and not any(same(v, e) for e in schema["enum"]):
        return False
    if "type" in schema:
        types = schema["type"] if isinstance(schema["type"], list) else [schema["type"]]
        if not any(has_type(v, t) for t in types):
            return False
    elif "const" not in schema and "enum" not in schema:
        return False
    if isinstance(v, str):
        if not schema.get("minLength", 0) <= len(v) <= schema.get("maxLength", 1 << 30):
            return False
    if isinstance(v, list):
        if not schema.get("minItems", 0) <= len(v) <= schema.get("maxItems", 1 << 30):
            return False
        if not all(valid(x, schema["items"], root) for x in v):
            return False
    if isinstance(v, dict):
        props = schema.get("properties", {})
        if any(k not in v for k in schema.get("required", [])) or any(k not in props for k in v):   # nothing undeclared is produced
            return False
        if [k for k in props if k in v] != list(v):    # in the schema's order
            return False
        if not all(valid(x, props[k], root) for k, x in v.items()):
            return False
    return True


def test_the_validator_itself():
    root = CASES[NAMES.index("refs")][1]
    assert valid({"from": {"x": 1, "y": 2}, "to": {"x": 3, "y": 4}}, root, root)
    assert not valid({"from": {"x": 1, "y": 2}, "to": {"x": 3}}, root, root)
    assert not valid({"from": {"x": 1, "y": True}, "to": {"x": 3, "y": 4}}, root, root)
    assert not valid(True, {"enum": [1]}, {}) and valid(1.0, {"enum": [1]}, {}) and not valid(1.5, INT, {})
    assert not valid("abcd", {"type": "string", "maxLength": 3}, {}) and not valid([1, 2], {"type": "array", "items": INT, "maxItems": 1}, {})
    assert not valid({"b": 1, "a": 2}, {"type": "object", "properties": {"a": INT, "b": INT}}, {})


# ----------------------------------------------------------------------------------------------------------- per schema

def distances(trans, accept):
    """bytes from every state to the nearest accepting one"""
    S = len(trans)
    dist = np.where(accept != 0, 0, S + 1).astype(np.int64)
    for _ in range(S):
        nxt = np.where(trans == G.DEAD, S + 1, dist[np.minimum(trans, S - 1)] + 1).min(axis=1)
        new = np.minimum(dist, nxt)
        if (new == dist).all():
            break
        dist = new
    return dist


def sample(trans, accept, dist, rng, wander):
    """one accepted string: `wander` random steps (a random successor state, then a random byte that leads there, so that the many
    bytes of a string's body do not crowd out the structure), then the shortest way to acceptance"""
    out = bytearray()
    s = 0
    for step in range(4000):
        row = trans[s]
        live = np.nonzero(row != G.DEAD)[0]
        if step >= wander:
            if accept[s]:
                return bytes(out)
            live = live[dist[row[live]] == dist[s] - 1]
        elif accept[s] and (len(live) == 0 or rng.random() < 0.2):
            return bytes(out)
        targets = np.unique(row[live])
        to = targets[rng.integers(len(targets))]
        choices = live[row[live] == to]
        b = int(choices[rng.integers(len(choices))])
        out.append(b)
        s = int(to)
    raise AssertionError("the walk found no accepting state")


@pytest.mark.parametrize("idx", range(len(CASES)), ids=NAMES)
def test_sampled_strings_parse_and_validate(compiled, idx):
    name, schema, _, _ = CASES[idx]
    trans, accept = dfa(compiled, idx)
    rng = np.random.default_rng(1000 + idx)
    dist = distances(trans, accept)
    seen = set()
    for i in range(150):
        text = sample(trans, accept, dist, rng, wander=int(rng.integers(0, 120)))
        seen.add(text)
        doc = json.loads(text.decode("utf-8"))     # strict UTF-8, strict JSON
        assert valid(doc, schema, schema), (name, text)
    assert len(seen) > (1 if name != "scalars" else 0)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=NAMES)
def test_valid_documents_are_accepted(compiled, idx):
    name, schema, docs, _ = CASES[idx]
    trans, accept = dfa(compiled, idx)
    for d in docs:
        data = d.encode("utf-8") if isinstance(d, str) else d
        assert valid(json.loads(data.decode("utf-8")), schema, schema), (name, d)    # the list itself is right
        assert G.accepts(trans, accept, data) == (True, len(data)), (name, d)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=NAMES)
def test_near_misses_are_refused_at_the_right_byte(compiled, idx):
    name, _, _, misses = CASES[idx]
    trans, accept = dfa(compiled, idx)
    for d, at in misses:
        data = d.encode("utf-8") if isinstance(d, str) else d
        assert G.accepts(trans, accept, data) == (False, at), (name, d)


def test_the_near_misses_cover_the_list():
    """missing required key, wrong order, trailing comma, raw control byte, lone surrogate bytes, overlong UTF-8, leading zero, a 19-digit
    integer, maxItems + 1 items: each is among the near-misses above"""
    flat = [(n, d if isinstance(d, bytes) else d.encode()) for n, _, _, misses in CASES for d, _ in misses]
    assert ("optional_everywhere", b'{"a": 1}') in flat and ("optional_everywhere", b'{"c": 1, "a": 2}') in flat
    assert ("optional_everywhere", b'{"c": 1,}') in flat and ("string", b'"a\x01"') in flat and ("string", b'"\xed\xa0\x80"') in flat
    assert ("string", b'"\xc0\xaf"') in flat and ("integer", b"01") in flat and ("integer", b"1234567890123456789") in flat
    assert ("array_bounds", b"[1, 2, 3, 4]") in flat


@pytest.mark.parametrize("idx", range(len(CASES)), ids=NAMES)
def test_automaton_is_trimmed_and_minimal(compiled, idx):
    trans, accept = dfa(compiled, idx)
    S = len(trans)
    assert ((trans < S) | (trans == G.DEAD)).all()
    reach = accept != 0
    for _ in range(S):
        new = reach | ((trans != G.DEAD) & reach[np.minimum(trans, S - 1)]).any(axis=1)
        if (new == reach).all():
            break
        reach = new
    assert reach.all(), "a live state that reaches no accepting state"
    seen, frontier = {0}, [0]
    while frontier:
        s = frontier.pop()
        for t in set(trans[s].tolist()) - {G.DEAD}:
            if t not in seen:
                seen.add(t)
                frontier.append(t)
    assert seen == set(range(S)), "an unreachable state"
    # minimal: Moore's refinement from {accepting, not} splits every pair of states apart
    cls = accept.astype(np.int64)
    while True:
        succ = np.where(trans == G.DEAD, -1, cls[np.minimum(trans, S - 1)])
        _, new = np.unique(np.column_stack([cls, succ]), axis=0, return_inverse=True)
        new = new.reshape(-1)
        if len(set(new.tolist())) == len(set(cls.tolist())):
            break
        cls = new
    assert len(set(cls.tolist())) == S, "two equivalent states"


def test_state_counts_of_the_documented_fragments(compiled):
    """DESIGN.md's table.  One state above a bare fragment's count is the optional space in front of the value"""
    obj3 = {"type": "object", "properties": {"a": STR, "b": STR, "c": STR}, "required": ["a", "b", "c"]}
    tool = {"type": "object", "properties": {
        "tool": {"enum": ["search", "fetch", "run"]}, "limit": INT,
        "args": {"type": "array", "items": {"type": "object", "properties": {"k": STR, "v": STR}, "required": ["k", "v"]}}},
        "required": ["tool", "limit", "args"]}
    recs = G.compile_schemas([STR, INT, {"type": "number"}, obj3, PERSON, tool])
    assert [r["n_states"] for r in recs] == [23, 21, 44, 86, 307, 124]


# ----------------------------------------------------------------------------------------------------------- refusals

REFUSED = [
    ({"type": "object", "properties": {"a": {"$ref": "#/$defs/n"}}, "$defs": {"n": {"type": "object", "properties": {"next": {"$ref": "#/$defs/n"}}}}},
     ["recursive", "'$ref'", "#/$defs/n/properties/next/$ref"]),
    ({"type": "object", "properties": {"a": {}}}, ["'type'", "#/properties/a", "recursive"]),
    ({"description": "anything"}, ["'type'", "at #"]),
    ({"type": "array"}, ["'items'", "at #", "recursive"]),
    ({"type": "array", "items": {"title": "anything"}}, ["'type'", "#/items"]),
    ({"oneOf": [STR, INT]}, ["'oneOf'", "#/oneOf"]),
    ({"allOf": [STR]}, ["'allOf'", "#/allOf"]),
    ({"not": STR}, ["'not'", "#/not"]),
    ({"if": STR, "then": STR, "else": INT}, ["'if'", "#/if"]),
    ({"type": "object", "properties": {"s": {"type": "string", "pattern": "a+"}}}, ["'pattern'", "#/properties/s/pattern"]),
    ({"type": "object", "patternProperties": {"a": STR}}, ["'patternProperties'", "#/patternProperties"]),
    ({"type": "integer", "minimum": 0}, ["'minimum'", "#/minimum"]),
    ({"type": "integer", "maximum": 9}, ["'maximum'", "#/maximum"]),
    ({"type": "number", "multipleOf": 2}, ["'multipleOf'", "#/multipleOf"]),
    ({"type": "array", "items": INT, "uniqueItems": True}, ["'uniqueItems'", "#/uniqueItems"]),
    ({"type": "array", "prefixItems": [INT]}, ["'prefixItems'", "#/prefixItems"]),
    ({"type": "string", "contentEncoding": "base64"}, ["'contentEncoding'", "#/contentEncoding"]),
    ({"enum": [1, [2]]}, ["'enum'", "#/enum", "non-scalar"]),
    ({"const": {"a": 1}}, ["'const'", "#/const", "non-scalar"]),
    ({"type": "string", "maxLength": 257}, ["'maxLength'", "#/maxLength", "256"]),
    ({"type": "string", "minLength": 300}, ["'minLength'", "#/minLength", "256"]),
    ({"type": "object", "properties": {"l": {"type": "array", "items": INT, "maxItems": 1000}}}, ["'maxItems'", "#/properties/l/maxItems", "256"]),
    ({"type": "array", "items": INT, "minItems": 257}, ["'minItems'", "#/minItems", "256"]),
    ({"type": "string", "minLength": 3, "maxLength": 2}, ["'minLength'", "#/minLength", "empty language"]),
    ({"type": "array", "items": INT, "minItems": 2, "maxItems": 1}, ["'minItems'", "#/minItems", "empty language"]),
    ({"enum": []}, ["'enum'", "#/enum", "empty language"]),
    ({"type": "string", "enum": [1, 2]}, ["'enum'", "#/enum", "empty language"]),
    ({"type": []}, ["'type'", "#/type", "empty language"]),
    ({"anyOf": []}, ["'anyOf'", "#/anyOf", "empty language"]),
    ({"type": "object", "properties": {"a": INT}, "required": ["b"]}, ["'required'", "#/required", "empty language"]),
    ({"type": "text"}, ["'type'", "#/type", "text"]),
    ({"$ref": "#/$defs/missing"}, ["'$ref'", "#/$ref", "missing"]),
    ({"$ref": "other.json#/a"}, ["'$ref'", "#/$ref"]),
    ({"$ref": "#/$defs/a", "type": "string", "$defs": {"a": STR}}, ["'$ref'", "#/$ref", "'type'"]),
    ({"anyOf": [STR], "type": "string"}, ["'anyOf'", "#/anyOf", "'type'"]),
    ({"enum": ["a"], "maxLength": 3}, ["'enum'", "#/enum", "'maxLength'"]),
    ("[1, 2]", ["not an object"]),
    ('{"type": ', ["not valid JSON"]),
    ({"type": "array", "items": {"type": "string", "maxLength": 256}, "maxItems": 256}, ["NFA states"]),
    ('{"enum": [1, 1e999]}', ["'enum'", "#/enum", "not finite"]),
    ('{"const": -1e999}', ["'const'", "#/const", "not finite"]),
]


def nested_arrays(depth, max_items):
    s = {"type": "null"}
    for _ in range(depth):
        s = {"type": "array", "items": s, "maxItems": max_items}
    return s


def nested_objects(depth):
    """every level: an optional property in front of the one that nests, so that the nesting member may come first or second and the
    tree keeps it several times"""
    s = {"type": "null"}
    for _ in range(depth):
        s = {"type": "object", "properties": {"x": {"type": "null"}, "a": s}}
    return s


def chained_refs(depth):
    defs = {f"d{depth}": {"type": "null"}}
    for k in range(depth):
        defs[f"d{k}"] = {"anyOf": [{"$ref": f"#/$defs/d{k + 1}"}, {"$ref": f"#/$defs/d{k + 1}"}]}   # no copy: two expansions per level
    return {"$ref": "#/$defs/d0", "$defs": defs}


# schemas of about a kilobyte whose syntax tree doubles or more with every level of nesting: the compiler bounds its own work
DEEP = [
    ("arrays_of_two", nested_arrays(40, 2), ["syntax nodes", "'items'", "/items"]),
    ("arrays_of_none_or_one", {"type": "array", "items": nested_arrays(40, 2), "maxItems": 0}, None),      # "[]": nothing is expanded
    ("objects", nested_objects(40), ["syntax nodes", "'properties'", "/properties"]),
    ("refs", chained_refs(40), ["syntax nodes", "#/$defs/d"]),
    ("refs_expanded", {"type": "object", "properties": {f"p{k}": {"$ref": "#/$defs/d0"} for k in range(3)},
                       "$defs": {**{f"d{k}": {"type": "object", "properties": {"x": {"$ref": f"#/$defs/d{k + 1}"},
                                                                                 "y": {"$ref": f"#/$defs/d{k + 1}"}}} for k in range(30)},
                                 "d30": {"type": "null"}}}, ["syntax nodes", "#/$defs/d"]),
]


@pytest.mark.parametrize("idx", range(len(DEEP)), ids=[d[0] for d in DEEP])
def test_deep_nesting_is_settled_within_a_second(idx):
    import time
    name, schema, words = DEEP[idx]
    assert len(json.dumps(schema)) < 8000
    t0 = time.monotonic()
    rec = G.compile_schemas([schema])[0]
    took = time.monotonic() - t0
    print(f"{name}: {took:.3f} s, ok={rec['ok']}, {rec.get('n_states', rec.get('err'))}")
    assert took < 1.0, took
    if words is None:
        assert rec["ok"] == 1 and G.accepts(rec["trans"], rec["accept"], b"[]") == (True, 2)
        return
    assert rec["ok"] == 0 and rec["err"].startswith("guide_json_schema: "), rec.get("n_states")
    for w in words:
        assert w in rec["err"], (w, rec["err"])


def test_single_item_nesting_compiles_in_linear_time():
    """the shape that doubled the tree without ever reaching the NFA cap: arrays of at most one item, 60 deep"""
    import time
    t0 = time.monotonic()
    rec = G.compile_schemas([nested_arrays(60, 1)])[0]
    took = time.monotonic() - t0
    assert took < 1.0, took
    assert rec["ok"] == 1 and rec["n_states"] < 400
    assert G.accepts(rec["trans"], rec["accept"], b"[" * 60 + b"null" + b"]" * 60)[0] is True
    assert G.accepts(rec["trans"], rec["accept"], b"[" * 7 + b"]" * 7)[0] is True
    assert G.accepts(rec["trans"], rec["accept"], b"[" * 60 + b"null,null" + b"]" * 60) == (False, 64)     # a second item
    assert G.accepts(rec["trans"], rec["accept"], b"[[null]]") == (False, 2)                                # null sits 60 deep only


@pytest.mark.parametrize("idx", range(len(REFUSED)), ids=[f"r{i}" for i in range(len(REFUSED))])
def test_refusals(idx):
    schema, words = REFUSED[idx]
    rec = G.compile_schemas([schema])[0]
    assert rec["ok"] == 0, (schema, rec.get("n_states"))
    assert rec["err"].startswith("guide_json_schema: "), rec
    for w in words:
        assert w in rec["err"], (w, rec["err"])


# ----------------------------------------------------------------------------------------------------------- the limits

def ints(n):
    return {"type": "array", "items": INT, "maxItems": n}


def test_limits():
    recs = G.compile_schemas([PERSON, ints(100), ints(150), ints(256)])
    assert recs[0]["ok"] == 1 and 255 < recs[0]["n_states"] <= 4096            # what guide_regex's 255 states cannot hold
    assert recs[1]["ok"] == 1 and recs[2]["ok"] == 1
    # a list of up to n integers takes a fixed number of states per item: the count at 256 items follows from those at 100 and 150 ...
    per_item, rest = divmod(recs[2]["n_states"] - recs[1]["n_states"], 50)
    assert rest == 0 and per_item >= 20
    want = recs[2]["n_states"] + per_item * (256 - 150)
    assert 4096 < want < 65534
    # ... and that count, beyond the cap and within the working bound, is what the refusal names beside the cap
    assert recs[3]["ok"] == 0
    m = re.fullmatch(r"guide_json_schema: the minimal automaton has (\d+) states; at most 4096 are supported", recs[3]["err"])
    assert m and int(m.group(1)) == want, recs[3]["err"]


def test_the_cap_itself_compiles():
    """the largest list of integers that fits, found from the per-item count: at most 4096 states, and one item more is refused"""
    a, b = (r["n_states"] for r in G.compile_schemas([ints(100), ints(150)]))
    per_item = (b - a) // 50
    n = 150 + (4096 - b) // per_item
    fits, over = G.compile_schemas([ints(n), ints(n + 1)])
    assert fits["ok"] == 1 and 4096 - per_item < fits["n_states"] <= 4096
    assert over["ok"] == 0 and "4096" in over["err"]
    assert G.accepts(fits["trans"], fits["accept"], b"[" + b", ".join(b"7" for _ in range(n)) + b"]") == (True, 3 * n)
    assert G.accepts(fits["trans"], fits["accept"], b"[" + b", ".join(b"7" for _ in range(n + 1)) + b"]")[0] is False


def test_guide_regex_keeps_its_limit():
    assert len(G8.compile_regex("a{254}")[0]) == 255
    with pytest.raises(AssertionError, match="255"):
        G8.compile_regex("a{255}")
    with pytest.raises(AssertionError, match="255"):
        G8.compile_regex("[ab]{150}c[ab]{150}")
