"""Guided decoding on the host side (tests/host/guide_trace.cc run: the generator and the engine over a fake backend with scripted logits):
the per-request automaton state follows the bytes of every emitted token; GuideEdit runs only on steps with an asking row and in batch-row
order; one load per distinct (pattern, end tokens); a slot is reused after its requests left; the 17th concurrent pattern fails alone; each
exclusion, an invalid pattern, a backend without guides and a tokenizer without TokenBytes fail the asking request alone; an injected
disagreement between backend and host fails only its request."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "guide_trace")
EOS, GEN_STOP = 256, 299
PIECES = ["yes", "no", "maybe", "ye", "s", "ma", "ybe", "12", "-4"]   # tests/host/guide_trace.cc kPieces: ids 257 ..
DEAD = 255


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


def loads(recs):
    return [r for r in recs if r.get("call") == "LoadGuide"]


def check_states(recs, patterns):
    """every step record's guide_states are the walk of the loaded automaton over the tokens the request has been answered with so far"""
    dfa = {r["slot"]: np.array(r["trans"]).reshape(r["n_states"], 256) for r in loads(recs)}
    produced = {}
    samples = [r for r in recs if r.get("call") == "Sample"]
    steps = [r for r in recs if "step" in r]
    assert len(samples) == len(steps)
    for st, sm in zip(steps, samples):
        assert st["ids"] == sm["ids"]
        for i, slot, state in zip(st["ids"], st["guide_slots"], st["guide_states"]):
            if i not in patterns:
                assert slot == -1 and state == 0
                continue
            assert slot >= 0
            s = 0
            for t in produced.get(i, []):
                for b in token_bytes(t):
                    s = int(dfa[slot][s, b])
            assert state == s != DEAD, (i, produced.get(i), state, s)
        for i, t in zip(sm["ids"], sm["tokens"]):
            produced.setdefault(i, []).append(t)


def test_state_sequence_and_full_matches(trace):
    recs = phase(trace, "mixed")
    patterns = {1: "(yes|no|maybe)", 2: "[0-9]{3}-[0-9]{4}", 4: "(yes|no|maybe)", 5: "[ab]{6,8}"}
    check_states(recs, patterns)
    toks, fin = answers(recs)
    assert not failures(recs)
    for i in (1, 2, 4):   # they end on an end token, and their bytes match in full
        assert fin[i] == "eos" and toks[i][-1] == EOS
        text = b"".join(token_bytes(t) for t in toks[i][:-1])
        assert re.fullmatch(patterns[i].encode(), text), (i, text)
    # cut off by its length limit (4 tokens of a pattern that needs 6 bytes): a prefix of a match
    assert fin[5] == "length" and len(toks[5]) == 4
    assert re.fullmatch(b"[ab]{4}", b"".join(token_bytes(t) for t in toks[5]))
    assert fin[3] == "length" and len(toks[3]) == 3           # the plain request runs its three steps
    # multi-byte tokens are walked byte by byte: somebody used one
    assert any(t > EOS for i in (1, 4) for t in toks[i])


def test_one_load_per_distinct_pattern(trace):
    recs = phase(trace, "mixed")
    got = loads(recs)
    assert [r["slot"] for r in got] == [0, 1, 2]                      # requests 1 and 4 share slot 0
    assert all(r["ends"] == [EOS, GEN_STOP] for r in got)             # the tokenizer's EOS and the generator's stop token
    assert sum(1 for r in recs if r.get("call") == "SetGuideVocab") == 1
    first = next(r for r in recs if "step" in r)
    assert first["ids"] == [1, 2, 3, 4, 5] and first["guide_slots"] == [0, 1, -1, 0, 2]
    # the set-up calls come in front of the first step
    k_step = recs.index(first)
    assert all(recs.index(r) < k_step for r in got)
    for r in recs:
        if r.get("call") == "GuideEdit":
            assert any(s >= 0 for s in r["slots"])


def test_seventeenth_concurrent_pattern_fails_alone(trace):
    recs = phase(trace, "slots")
    assert sorted(r["slot"] for r in loads(recs)) == list(range(16))
    fails = failures(recs)
    assert list(fails) == [116] and "all 16 guide slots" in fails[116]["msg"]
    toks, fin = answers(recs)
    for i in range(100, 116):
        assert fin[i] == "eos"
        assert b"".join(token_bytes(t) for t in toks[i][:-1]) == b"x" + bytes([ord("a") + i - 100]) * 2
    assert fin[117] == "length"
    assert not any(r.get("call") == "UnloadGuide" for r in recs)


def test_slot_reuse_after_release(trace):
    recs = phase(trace, "slots_reuse")
    first = next(r for r in recs if "step" in r)
    last = [k for k, r in enumerate(recs) if "step" in r][-1]
    calls = [r for r in recs[:recs.index(first)] if r.get("call") in ("UnloadGuide", "LoadGuide")]
    # the new pattern takes the place of the slot used longest ago (slot 0); the old pattern "xc{2}" is still loaded in slot 2: no load
    assert [(r["call"], r["slot"]) for r in calls] == [("UnloadGuide", 0), ("LoadGuide", 0)]
    # a generator that ends gives every slot back to the backend, which outlives it
    assert sorted(r["slot"] for r in recs[last:] if r.get("call") == "UnloadGuide") == list(range(16))
    assert first["ids"] == [200, 201] and first["guide_slots"] == [0, 2]
    toks, fin = answers(recs)
    assert fin == {200: "eos", 201: "eos"}
    assert b"".join(token_bytes(t) for t in toks[200][:-1]) == b"neww"
    assert b"".join(token_bytes(t) for t in toks[201][:-1]) == b"xcc"


def test_exclusions_fail_alone(trace):
    recs = phase(trace, "exclusions")
    fails = failures(recs)
    want = {1: "early_stopping", 2: "allowed_tokens", 3: "banned_tokens", 4: "min_new_tokens", 5: "-inf logit_bias", 7: "unterminated group",
            8: "at most 255"}
    assert sorted(fails) == sorted(want)
    for i, text in want.items():
        assert fails[i]["code"] == "invalid" and text in fails[i]["msg"] and f"id [{i}]" in fails[i]["msg"], fails[i]
    toks, fin = answers(recs)
    for i in (6, 9):   # a finite bias is fine; the last one is plainly served
        assert fin[i] == "eos" and b"".join(token_bytes(t) for t in toks[i][:-1]) == b"ok"
    assert len(loads(recs)) == 1   # 6 and 9 share the pattern; the refused ones loaded nothing


@pytest.mark.parametrize("name, text", [("old_backend", "no GuideEdit"), ("old_tokenizer", "TokenBytes"), ("no_tokenizer", "TokenBytes")])
def test_backend_or_tokenizer_without_guides(trace, name, text):
    recs = phase(trace, name)
    fails = failures(recs)
    assert list(fails) == [1] and fails[1]["code"] == "unsupported" and text in fails[1]["msg"]
    toks, fin = answers(recs)
    assert fin == {2: "length"} and len(toks[2]) == 3
    assert not any(r.get("call") in ("SetGuideVocab", "LoadGuide", "GuideEdit") for r in recs)


def test_injected_disagreement_fails_only_its_request(trace):
    recs = phase(trace, "disagree")
    fails = failures(recs)
    assert list(fails) == [1] and fails[1]["code"] == "other" and "internal error" in fails[1]["msg"]
    toks, fin = answers(recs)
    assert fin[2] == "eos" and re.fullmatch(b"[xy]", b"".join(token_bytes(t) for t in toks[2][:-1]))
    assert fin[3] == "length" and len(toks[3]) == 3
    assert 1 not in fin
    # its slot reference was released with it: the step after it left carries only the plain request
    last = [r for r in recs if "step" in r][-1]
    assert last["ids"] == [3] and last["guide_slots"] == [-1]


def test_nobody_asks_nothing_new_is_called(trace):
    recs = phase(trace, "nobody")
    assert not any(r.get("call") in ("SetGuideVocab", "LoadGuide", "UnloadGuide", "GuideEdit") for r in recs)
    assert all(set(r["guide_slots"]) == {-1} for r in recs if "step" in r)
