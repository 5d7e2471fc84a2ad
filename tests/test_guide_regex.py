"""The guide compiler (src/common/guide.cc through build/guide_trace dfa): for every pattern, every string up to length 6 over the pattern's
own alphabet plus one foreign byte is accepted exactly when Python's re.fullmatch on bytes accepts it, and a state other than the dead one
means "prefix of some match" (by graph search on the table: every live state reaches an accepting one, the dead state is never left).
Every construct outside the dialect, an empty language and an automaton of more than 255 states are refused with a message.

A non-ASCII character is one atom of the dialect (a quantifier behind it repeats the character), so for Python's bytes engine it is wrapped
into a group."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "guide_trace")
DEAD = 255
MAX_LEN = 6

# (pattern, alphabet or None = the pattern's own literal characters)
PATTERNS = [
    ("abc", None),                                   # literals
    ("a|bc|", None),                                 # alternation with an empty branch
    ("(yes|no|nay)", None),                          # an alternation of words
    ("(?:ab)*c", None),                              # non-capturing group, star
    ("(ab)+", None),                                 # group, plus
    ("ab?c", None),                                  # optional
    ("a{3}", None),                                  # {m}
    ("a{2,}b", None),                                # {m,}
    ("(ab){1,2}c{0,3}", "abc"),                      # {m,n}, {0,n}
    ("a.c", "abc\n"),                                # . is not a newline
    ("[a-c]x[^a-c]", "abcxy"),                       # class range and negation
    ("[]a]b", "]ab"),                                # a leading ] is a literal
    ("[a\\-c]+", "a-bc"),                            # an escaped - in a class
    ("[^\\d]\\d", "a1"),                             # negated shorthand in a class
    ("\\d+\\.\\d{1,2}", "12."),                      # \d and an escaped metacharacter
    ("\\w+\\s\\w+", "a_ \t"),                        # \w \s
    ("\\D\\W\\S", "a1 -"),                           # \D \W \S
    ("a\\n\\t\\rb", "ab\n\t\r"),                     # \n \t \r
    ("\\x41\\x7a", "Az"),                            # \xHH
    ("\\(\\)\\[\\]\\{\\}", "()[]{}"),                    # escaped metacharacters
    ("\\|\\*\\+\\?\\.\\\\", "|*+?.\\"),                   # the other escaped metacharacters
    ("a{b", "a{b"),                                  # a { that begins no quantifier is a literal
    ("a}b]", "a}b]"),                                # } and ] outside a class are literals
    ("[0-9]{3}-[0-9]{2}", "0189-"),                  # counted digits around a literal
    ("(19|20)[0-9]-(0[1-9]|1[0-2])", "0129-"),       # the shape of a date (a whole one: test_long_matches)
    ('\\{"a": (true|false)\\}', '{"a: t'),           # a flat JSON object: longer than 6, so its prefixes and the dead state are checked
    ('\\{"n":[1-9]?\\}', '{"n:1}'),                  # a flat JSON object with an optional digit: {"n":} is within reach
    ("é", None),                                # a multi-byte literal
    ("é+a|€", None),                       # a quantifier repeats the character, three-byte literal
    ("(a|b)*abb", None),                             # the textbook subset construction
    ("(a*)*b", None),                                # nested stars
    ("(|a)(|b)", None),                              # empty alternatives
    ("x*", None),                                    # the empty string matches
]

LONG_ONLY = next(i for i, (p, _) in enumerate(PATTERNS) if "true" in p)   # its shortest match has 11 bytes

REFUSED = [
    ("^abc", "anchor"), ("abc$", "anchor"), ("a\\b", "anchor"), ("\\Aabc", "anchor"), ("abc\\Z", "anchor"),
    ("(a)\\1", "backreference"), ("(?=a)a", "lookaround"), ("(?!a)b", "lookaround"), ("(?<=a)b", "lookaround"), ("(?P<n>a)", "named"),
    ("(?i)a", "flags"), ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{1,2}?", "lazy"), ("a*+", "possessive"),
    ("a**", "quantifier"), ("*a", "repeat"), ("(ab", "group"), ("ab)", "unmatched"), ("[ab", "class"), ("[é]", "non-ASCII"),
    ("a{3,2}", "n < m"), ("a{257}", "256"), ("a{,3}", "{,n}"), ("\\q", "escape"), ("\\xZ1", "hex"), ("[z-a]", "backwards"), ("ab\\", "backslash"),
]


def py_pattern(p):
    """the pattern for re on bytes: every non-ASCII character as a group of its bytes"""
    out = b""
    for ch in p:
        enc = ch.encode("utf-8")
        out += enc if len(enc) == 1 else b"(?:" + enc + b")"
    return out


def alphabet(p, given):
    chars = given if given is not None else "".join(c for c in p if c.isalnum() or ord(c) > 127)
    own = sorted(set(chars.encode("utf-8")))
    foreign = next(b for b in b"#~%Q" if b not in own)
    return own + [foreign]


def compile_all(patterns):
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    text = "".join(p.encode("utf-8").hex() + "\n" for p in patterns)
    out = subprocess.run([BIN, "dfa"], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(recs) == len(patterns)
    return recs


@pytest.fixture(scope="module")
def compiled():
    return compile_all([p for p, _ in PATTERNS])


@pytest.mark.parametrize("idx", range(len(PATTERNS)), ids=[f"p{i}" for i in range(len(PATTERNS))])
def test_pattern_against_re(compiled, idx):
    pattern, given = PATTERNS[idx]
    rec = compiled[idx]
    assert rec["ok"] == 1, rec
    S = rec["n_states"]
    assert 1 <= S <= 255
    trans = np.array(rec["trans"], dtype=np.int64).reshape(S, 256)
    accept = np.array(rec["accept"], dtype=bool)
    assert ((trans < S) | (trans == DEAD)).all()
    # trimmed: every live state reaches an accepting one (so "not dead" is "a prefix of some match"), and every state is reachable
    reach = accept.copy()
    for _ in range(S):
        nxt = np.where(trans == DEAD, 0, trans)
        reach = reach | ((trans != DEAD) & reach[nxt]).any(axis=1)
    assert reach.all(), "a live state that reaches no accepting state"
    seen = {0}
    frontier = [0]
    while frontier:
        s = frontier.pop()
        for t in set(trans[s].tolist()) - {DEAD}:
            if t not in seen:
                seen.add(t)
                frontier.append(t)
    assert seen == set(range(S)), "an unreachable state"
    # minimal: no two states with the same acceptance and the same row
    rows = {(bool(accept[s]), trans[s].tobytes()) for s in range(S)}
    assert len(rows) == S
    rx = re.compile(py_pattern(pattern))
    alpha = alphabet(pattern, given)
    assert len(alpha) <= 7
    table = trans.tolist()
    acc = accept.tolist()
    matched = 0
    stack = [(b"", 0)]   # every string up to MAX_LEN with the state it leads to, depth first
    while stack:
        text, s = stack.pop()
        ours = s != DEAD and acc[s]
        theirs = rx.fullmatch(text) is not None
        assert ours == theirs, (pattern, text, ours, theirs)
        matched += theirs
        if len(text) < MAX_LEN:
            for b in alpha:
                stack.append((text + bytes([b]), DEAD if s == DEAD else table[s][b]))
    if pattern != PATTERNS[LONG_ONLY][0]:
        assert matched > 0, "the enumeration never reached a match"


def test_long_matches():
    """matches longer than the enumeration: a date, a flat JSON object"""
    pats = ["(19|20)[0-9]{2}-(0[1-9]|1[0-2])-(0[1-9]|[12][0-9]|3[01])", '\\{"ok": (true|false), "n": [1-9][0-9]{0,2}\\}']
    recs = compile_all(pats)
    cases = [[b"2026-10-19", b"1999-01-31", b"2026-13-01", b"2026-10-32", b"2026-10-1", b"2026-10-190"],
             [b'{"ok": true, "n": 7}', b'{"ok": false, "n": 120}', b'{"ok": maybe, "n": 7}', b'{"ok": true, "n": 07}', b'{"ok": true, "n": 1000}']]
    for p, rec, strings in zip(pats, recs, cases):
        assert rec["ok"] == 1, rec
        trans = np.array(rec["trans"]).reshape(rec["n_states"], 256)
        for s in strings:
            st = 0
            for b in s:
                st = int(trans[st, b])
                if st == DEAD:
                    break
            assert (st != DEAD and bool(rec["accept"][st])) == (re.fullmatch(p.encode(), s) is not None), (p, s)


@pytest.mark.parametrize("idx", range(len(REFUSED)), ids=[f"r{i}" for i in range(len(REFUSED))])
def test_refused_constructs(idx):
    pattern, _ = REFUSED[idx]
    rec = compile_all([pattern])[0]
    assert rec["ok"] == 0, (pattern, rec.get("n_states"))
    assert rec["err"].startswith("guide_regex: ") and len(rec["err"]) > 20, rec


def test_size_limit_and_empty_language():
    recs = compile_all(["a{254}", "a{255}", "[ab]{200}c[ab]{100}", "a[^\\x00-\\x7f]", "[^\\x00-\\x7f]|b"])
    assert recs[0]["ok"] == 1 and recs[0]["n_states"] == 255          # 255 live states: the limit itself
    assert recs[1]["ok"] == 0 and "255" in recs[1]["err"]             # 256 live states
    assert recs[2]["ok"] == 0 and "states" in recs[2]["err"]
    assert recs[3]["ok"] == 0 and "empty language" in recs[3]["err"]  # a negated class is taken within ASCII: nothing is left
    assert recs[4]["ok"] == 1 and recs[4]["n_states"] == 2            # the dead branch is trimmed, the other one stays
