"""Logit rules on the host side (tests/host/rules_trace.cc: the generator and the engine over a fake backend): a rule is validated when its
request is admitted and uploaded once, with the request's slot, before its first step; the flags follow the batch rows; bit 1 lasts
min_new_tokens steps; EditLogits runs in front of the penalty and only on steps with a flag; a reused slot carries no stale flags; an
invalid rule or a backend without logit rules fails the asking request alone; with no rule anywhere nothing new is called."""
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "rules_trace")
GEN = {i: i + 1 for i in range(1, 7)}                    # request id runs id + 1 steps
NO_SLOT = 2 ** 63 - 1
# tests/host/rules_trace.cc ValidRule: what each asking request must have uploaded, and its flags by the number of tokens it has produced
RULES = {
    2: dict(bias_tokens=[10, 11, 12], bias_values=[1.5, "-inf", "-inf"], has_mask=0, allowed=[], stops=[]),
    3: dict(bias_tokens=[], bias_values=[], has_mask=0, allowed=[], stops=[900, 901]),
    5: dict(bias_tokens=[33], bias_values=["-inf"], has_mask=1, allowed=[5, 33, 505, 999], stops=[901]),
}
MIN_NEW = {3: 2, 5: 10}


def flags_of(i, produced):
    f = 0
    if i in (2, 5):
        f |= 1
    if i in MIN_NEW and produced < MIN_NEW[i]:
        f |= 2
    return f


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _phase(trace, phase):
    """the records between a phase's begin marker and the next one (the last step's responses arrive while the generator is idle)"""
    first = next(k for k, r in enumerate(trace) if r.get("begin") == phase)
    out = []
    for r in trace[first + 1:]:
        if "begin" in r:
            break
        out.append(r)
    return out


def _steps(records):
    """[(uploads in front of the step, step record, post-processor calls of that step)]"""
    out, pending = [], []
    for r in records:
        if "phase" in r:
            out.append((pending, r, []))
            pending = []
        elif r.get("call") == "SetLogitRule":
            pending.append(r)
        elif "call" in r:
            out[-1][2].append(r)
    assert not pending
    return out


@pytest.mark.parametrize("phase,penalty", [("rules_penalty", True), ("rules_plain", False)])
def test_rules_upload_once_and_flags_follow_the_rows(trace, phase, penalty):
    rec = _phase(trace, phase)
    produced = {i: 0 for i in GEN}
    slot_of, uploads, rows_seen = {}, {i: 0 for i in GEN}, {i: set() for i in GEN}
    asker_slots_before, reused = set(), False
    for ups, step, calls in _steps(rec):
        ids = [t - 500 for t in step["last_tokens"]]
        new = [i for i in ids if i not in slot_of]
        # a rule goes up exactly once, in front of the request's first step, with the request's slot, in admission order
        assert [u["slot"] for u in ups] == [step["batch_slots"][ids.index(i)] for i in new if i in RULES]
        for u, i in zip(ups, [i for i in new if i in RULES]):
            assert {k: u[k] for k in RULES[i]} == RULES[i], (i, u)
            assert u["mask_words"] == (32 if RULES[i]["has_mask"] else 0)       # ceil(1000 / 32)
            uploads[i] += 1
        for row, i in enumerate(ids):
            s = step["batch_slots"][row]
            if i in new:
                slot_of[i] = s
                if i not in RULES and s in asker_slots_before:
                    reused = True                                                # a slot that held a rule, now owned by a request without one
            assert slot_of[i] == s                                               # the slot is stable while the request lives
            assert (s != NO_SLOT) if (penalty or i in RULES) else (s == NO_SLOT)
            rows_seen[i].add(row)
            if i in RULES:
                asker_slots_before.add(s)
        live = [s for s in step["batch_slots"] if s != NO_SLOT]
        assert len(set(live)) == len(live) and all(0 <= s < 4 for s in live)
        want = [flags_of(i, produced[i]) for i in ids]
        assert step["logit_flags"] == want, (step, want)
        names = [c["call"] for c in calls]
        expect = (["EditLogits"] if any(want) else []) + (["ApplyPenalty"] if penalty else []) + ["SampleTopKTopP"]
        assert names == expect, (step, names)                                    # in front of the penalty, only on steps with a flag
        if any(want):
            e = calls[0]
            assert e["flags"] == want and e["slots"] == step["batch_slots"] and e["batch"] == len(ids)
            assert e["vocab"] == e["stride"] == 1000 and e["logits_null"] == 0 and e["last_tokens"] == step["last_tokens"]
        for i in ids:
            produced[i] += 1
    assert uploads == {i: int(i in RULES) for i in GEN}
    assert produced == GEN
    assert max(len(r) for r in rows_seen.values()) > 1                           # compaction moved somebody, and its flags with it
    assert reused or not penalty
    # bit 1 was set for exactly the first min_new_tokens steps of request 3 (request 5 lives 6 < 10 steps: on all of them)
    seq = {i: [s["logit_flags"][[t - 500 for t in s["last_tokens"]].index(i)] for _, s, _ in _steps(rec) if 500 + i in s["last_tokens"]]
           for i in (3, 5)}
    assert seq[3] == [2, 2, 0, 0] and seq[5] == [3] * 6
    assert not [r for r in rec if "failed" in r]
    for i in GEN:
        rs = [r for r in rec if r.get("rsp") == i]
        assert len(rs) == GEN[i] and [r["finished"] for r in rs] == [0] * (GEN[i] - 1) + [1]


def test_invalid_rules_fail_their_request_alone(trace):
    rec = _phase(trace, "invalid")
    failed = {r["failed"]: r for r in rec if "failed" in r}
    field = {1: "logit_bias", 2: "logit_bias", 3: "logit_bias", 4: "logit_bias", 5: "logit_bias", 6: "stop_tokens", 7: "allowed_tokens",
             8: "allowed_tokens"}
    assert sorted(failed) == sorted(field)
    for i, f in field.items():
        assert failed[i]["code"] == "invalid" and f"id [{i}] {f}:" in failed[i]["msg"], failed[i]
        assert not [r for r in rec if r.get("rsp") == i]
    for i in (9, 10):                                                            # the batch goes on; 10 sits on every boundary that passes
        rs = [r for r in rec if r.get("rsp") == i]
        assert len(rs) == i + 1 and rs[-1]["finished"] == 1
    ups = [r for r in rec if r.get("call") == "SetLogitRule"]
    assert len(ups) == 1 and len(ups[0]["bias_tokens"]) == 512 and len(ups[0]["stops"]) == 64 and ups[0]["allowed"] == [0, 700, 901]
    # no failed request ever had a row
    assert all(t - 500 in (9, 10) for _, s, _ in _steps(rec) for t in s["last_tokens"])


def test_backend_without_logit_rules_fails_the_asking_requests_only(trace):
    rec = _phase(trace, "old_backend")
    failed = [r for r in rec if "failed" in r]
    assert sorted((r["failed"], r["code"]) for r in failed) == [(2, "unsupported"), (3, "unsupported"), (5, "unsupported")]
    assert all("EditLogits" in r["msg"] for r in failed)
    for i in (1, 4, 6):
        rs = [r for r in rec if r.get("rsp") == i]
        assert len(rs) == GEN[i] and rs[-1]["finished"] == 1
    for _, s, calls in _steps(rec):
        assert not any(s["logit_flags"]) and [c["call"] for c in calls] == ["ApplyPenalty", "SampleTopKTopP"]
        assert not {502, 503, 505} & set(s["last_tokens"])                       # failed at admission: never in a batch


@pytest.mark.parametrize("new,old", [("nobody", "old_backend_nobody"), ("nobody_plain", "old_backend_nobody_plain")])
def test_without_rules_the_trace_is_the_one_of_a_backend_without_them(trace, new, old):
    a, b = _phase(trace, new), _phase(trace, old)
    strip = lambda rec: [{k: v for k, v in r.items() if k != "phase"} for r in rec if "rsp" not in r]
    assert strip(a) == strip(b)                                                  # (the responses arrive on another thread)
    assert not [r for r in a if r.get("call") in ("SetLogitRule", "EditLogits") or "failed" in r]
    assert all(not any(s["logit_flags"]) for _, s, _ in _steps(a))
    if new == "nobody_plain":
        assert all(s == NO_SLOT for _, st, _ in _steps(a) for s in st["batch_slots"])   # no slot is taken without the penalty
    assert len([r for r in a if "rsp" in r]) == sum(GEN.values())
