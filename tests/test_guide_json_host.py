"""JSON-schema guides on the host side (tests/host/guide_json_trace.cc run: the generator and the engine over a fake backend with scripted
logits): a request with guide_json_schema is admitted under the conditions of guide_regex and fails alone under each exclusion, with both
fields set, with a refused schema and on a backend without LoadGuide16; two requests with one schema share a slot and a regex of the same
text does not; the per-request state follows the bytes of every emitted token through states beyond 255; every finished answer is a JSON
document that fits its schema."""
import json
import os
import subprocess

import pytest

from tests import guide as G8
from tests import guide16 as G
from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "guide_json_trace")
EOS, GEN_STOP = 256, 299
PIECES = ["true", "false", "\"a", "\": ", ", \"", "12", "-4", "null", "{\""]   # tests/host/guide_json_trace.cc kPieces: ids 257 ..


def token_bytes(t):
    if t < 256:
        return bytes([t])
    if EOS < t <= EOS + len(PIECES):
        return PIECES[t - EOS - 1].encode()
    return b""


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN, "run"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.fixture(scope="module")
def automata(trace):
    """name -> (schema text, trans, accept) of the run's schemas, compiled once more through `dfa`; "regex": the schema `both` as a pattern"""
    texts = {r["schema"]: r["text"] for r in trace if "schema" in r}
    assert sorted(texts) == ["both", "long", "small"]
    names = sorted(texts)
    recs = G.compile_schemas([texts[n] for n in names])
    out = {n: (texts[n], r["trans"], r["accept"]) for n, r in zip(names, recs)}
    out["regex"] = (texts["both"],) + G8.compile_regex(texts["both"])
    return out


def phase(trace, name):
    first = next(k for k, r in enumerate(trace) if r.get("begin") == name)
    out = []
    for r in trace[first + 1:]:
        if "begin" in r:
            break
        out.append(r)
    return out


def answers(recs):
    """id -> (tokens, how it finished)"""
    toks, fin = {}, {}
    for r in recs:
        if "rsp" in r:
            toks.setdefault(r["rsp"], []).append(r["token"])
            if r["finished"] != 0:
                fin[r["rsp"]] = r["finished"]
    return toks, fin


def failures(recs):
    return {r["failed"]: r for r in recs if "failed" in r}


def text_of(tokens):
    return b"".join(token_bytes(t) for t in tokens)


MIXED = {1: "small", 2: "long", 4: "small", 5: "regex", 6: "both"}     # request id -> its automaton


def test_admission_and_loads(trace, automata):
    recs = phase(trace, "mixed")
    assert not failures(recs)
    loads = [r for r in recs if r.get("call") in ("LoadGuide", "LoadGuide16")]
    # 1 and 4 share a slot; the regex and the schema of the same text are two guides of two kinds
    assert [(r["call"], r["slot"]) for r in loads] == [("LoadGuide16", 0), ("LoadGuide16", 1), ("LoadGuide", 2), ("LoadGuide16", 3)]
    assert [r["n_states"] for r in loads] == [len(automata[n][1]) for n in ("small", "long", "regex", "both")]
    assert all(r["ends"] == [EOS, GEN_STOP] for r in loads)
    assert sum(1 for r in recs if r.get("call") == "SetGuideVocab") == 1
    first = next(r for r in recs if "step" in r)
    assert first["ids"] == [1, 2, 3, 4, 5, 6] and first["guide_slots"] == [0, 1, -1, 0, 2, 3]
    assert all(recs.index(r) < recs.index(first) for r in loads)
    assert len(automata["long"][1]) > 256 and len(automata["regex"][1]) != len(automata["both"][1])


def test_state_sequence_beyond_255(trace, automata):
    recs = phase(trace, "mixed")
    produced, top = {}, {}
    samples = [r for r in recs if r.get("call") == "Sample"]
    steps = [r for r in recs if "step" in r]
    assert len(samples) == len(steps)
    for st, sm in zip(steps, samples):
        assert st["ids"] == sm["ids"]
        for i, slot, state in zip(st["ids"], st["guide_slots"], st["guide_states"]):
            if i not in MIXED:
                assert slot == -1 and state == 0
                continue
            trans = automata[MIXED[i]][1]
            dead = G8.DEAD if MIXED[i] == "regex" else G.DEAD
            s = 0
            for b in text_of(produced.get(i, [])):
                s = int(trans[s, b])
                assert s != dead
            assert state == s, (i, produced.get(i), state, s)
            top[i] = max(top.get(i, 0), state)
        for i, t in zip(sm["ids"], sm["tokens"]):
            produced.setdefault(i, []).append(t)
    assert top[2] >= 256 and top[2] > 300, "the long schema's request never went beyond state 255"
    # the GuideEdit calls carry those states to the backend
    assert max(s for r in recs if r.get("call") == "GuideEdit" for s in r["states"]) == top[2]


def test_answers_fit_their_schemas(trace, automata):
    recs = phase(trace, "mixed")
    toks, fin = answers(recs)
    for i, name in MIXED.items():
        assert fin[i] == "eos" and toks[i][-1] == EOS, (i, fin.get(i))
        text = text_of(toks[i][:-1])
        if name == "regex":
            assert text == automata["both"][0].encode()       # the pattern matches its own text and nothing else
            continue
        schema = json.loads(automata[name][0])
        doc = json.loads(text.decode("utf-8"))
        if name == "small":
            assert isinstance(doc, list) and len(doc) <= 3 and all(isinstance(x, bool) for x in doc)
        elif name == "both":
            assert doc is None
        else:
            assert list(doc) == list(schema["properties"])
            a, b, c, d = doc.values()
            assert isinstance(a, bool) and (b is None or (isinstance(b, int) and not isinstance(b, bool)))
            assert c in schema["properties"][list(doc)[2]]["enum"] and isinstance(d, str) and len(d) <= 3
    assert fin[3] == "length" and len(toks[3]) == 3
    assert any(t > EOS for i in MIXED for t in toks[i]), "nobody used a multi-byte token"


def test_exclusions_fail_alone(trace):
    recs = phase(trace, "exclusions")
    fails = failures(recs)
    want = {1: "guide_json_schema: needs early_stopping", 2: "guide_json_schema: cannot be combined with allowed_tokens",
            3: "guide_json_schema: cannot be combined with banned_tokens", 4: "guide_json_schema: cannot be combined with min_new_tokens",
            5: "guide_json_schema: cannot be combined with a -inf logit_bias", 7: "guide_json_schema: cannot be combined with guide_regex",
            8: "guide_json_schema: keyword 'pattern' at #/pattern", 9: "guide_json_schema: the schema is not valid JSON"}
    assert sorted(fails) == sorted(want)
    for i, text in want.items():
        assert fails[i]["code"] == "invalid" and text in fails[i]["msg"] and f"id [{i}]" in fails[i]["msg"], fails[i]
    toks, fin = answers(recs)
    for i in (6, 10):   # a finite bias is fine; the last one is plainly served
        assert fin[i] == "eos"
        doc = json.loads(text_of(toks[i][:-1]).decode())
        assert isinstance(doc, list) and len(doc) <= 3
    loads = [r for r in recs if r.get("call") in ("LoadGuide", "LoadGuide16")]
    assert [(r["call"], r["slot"]) for r in loads] == [("LoadGuide16", 0)]   # 6 and 10 share the schema; the refused ones loaded nothing


def test_backend_without_wide_guides_fails_the_asking_request_alone(trace):
    recs = phase(trace, "narrow_backend")
    fails = failures(recs)
    assert list(fails) == [1] and fails[1]["code"] == "unsupported" and "no LoadGuide16" in fails[1]["msg"]
    toks, fin = answers(recs)
    assert fin == {2: "eos", 3: "length"} and text_of(toks[2][:-1]) == b"ok" and len(toks[3]) == 3
    assert [r["call"] for r in recs if r.get("call") in ("LoadGuide", "LoadGuide16")] == ["LoadGuide"]
    # the refused request holds no slot: the regex's guide went into slot 0
    assert next(r for r in recs if "step" in r)["guide_slots"] == [0, -1]
