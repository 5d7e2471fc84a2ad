"""Prompt logprobs on the host side (tests/host/prompt_lp_trace.cc: the generator and the engine over a fake backend): the ask is clamped
at admission, travels with its batch row and is taken back after the request's first step; the arrays arrive on the response that carries
the request's first token, in the request's order, also when it is prefilled beside decode rows after a compaction; an asking request
takes no prefix-cache hit and still publishes, so that an identical request that does not ask hits; nobody asking means no call; a
backend without prompt logprobs fails the asking request alone."""
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "prompt_lp_trace")
# tests/host/prompt_lp_trace.cc: request id has LEN[id] prompt tokens, runs id + 1 steps and asks for ASKED[id] (25 and -5 as the client sent them)
GEN = {i: i + 1 for i in range(1, 7)}
LEN = {1: 3, 2: 4, 3: 2, 4: 3, 5: 5, 6: 1}
ASKED = {1: -1, 2: 0, 3: 25, 4: -5, 5: 2, 6: 0}
N = {i: max(-1, min(a, 20)) for i, a in ASKED.items()}


def prompt(i):
    return [10 * i + k for k in range(1, LEN[i])] + [500 + i]


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _phase(trace, phase):
    """the records from the first step record of a phase up to the next phase's first; the last step's responses arrive while the
    generator is idle, before the next phase starts"""
    out, inside = [], False
    for r in trace:
        if "phase" in r:
            inside = r["phase"] == phase
        if inside:
            out.append(r)
    return out


def _steps(records):
    """[(step record, [backend calls of that step])]"""
    out = []
    for r in records:
        if "phase" in r:
            out.append((r, []))
        elif "call" in r:
            out[-1][1].append(r)
    return out


def _last_tokens(calls):
    return next(c for c in calls if c["call"] == "SampleTopKTopP")["last_tokens"]


def _want(i):
    """the fake backend's answer for request i: what Response i must carry with its first token"""
    p, n = prompt(i), N[i]
    if n < 0 or len(p) < 2:
        return [], [], [], []
    tgt = p[1:]
    return ([-t for t in tgt], list(range(len(tgt))), [t + e for t in tgt for e in range(n)], [-e for _ in tgt for e in range(n)])


def test_clamp_rows_and_first_response_only(trace):
    rec = _phase(trace, "mixed")
    first_step = {}
    for k, (step, calls) in enumerate(_steps(rec)):
        ids = [t - 500 for t in _last_tokens(calls)]
        lens = [b - a for a, b in zip(step["seq_starts"], step["seq_starts"][1:])]
        for i in ids:
            first_step.setdefault(i, k)
        # a request carries its clamped ask on its first step and -1 afterwards
        assert step["prompt_logprobs_list"] == [N[i] if first_step[i] == k else -1 for i in ids], (k, step)
        names = [c["call"] for c in calls]
        if any(a >= 0 for a in step["prompt_logprobs_list"]):
            assert names == ["SetPromptLogprobs", "SampleTopKTopP", "GetPromptLogprobs"]      # between the inputs and the run; read after the sampler
            assert calls[0]["ask"] == step["prompt_logprobs_list"] and calls[0]["batch"] == len(ids) and calls[0]["seq_starts"] == step["seq_starts"]
            want_positions = sum(n - 1 for n, a in zip(lens, step["prompt_logprobs_list"]) if a >= 0)
            assert calls[2]["positions"] == want_positions
        else:
            assert names == ["SampleTopKTopP"]
    # requests 5 and 6 were prefilled beside decode rows, behind them in the batch, after a compaction
    assert first_step[5] > 0 and first_step[6] > first_step[5]
    for i in GEN:
        rs = [r for r in rec if r.get("rsp") == i]
        assert len(rs) == GEN[i] and [r["finished"] for r in rs] == [0] * (GEN[i] - 1) + [1] and all(r["token"] == 500 + i for r in rs)
        lp, ranks, ttok, tlp = _want(i)
        assert (rs[0]["prompt_logprobs"], rs[0]["prompt_ranks"], rs[0]["prompt_top_tokens"], rs[0]["prompt_top_logprobs"]) == (lp, ranks, ttok, tlp), (i, rs[0])
        assert len(rs[0]["prompt_logprobs"]) == (LEN[i] - 1 if N[i] >= 0 else 0)
        for r in rs[1:]:
            assert r["prompt_logprobs"] == r["prompt_ranks"] == r["prompt_top_tokens"] == r["prompt_top_logprobs"] == []
    assert not [r for r in rec if "failed" in r]


def test_asking_request_takes_no_prefix_hit_and_publishes(trace):
    cold, plain, again, plain2 = (_phase(trace, p) for p in ("prefix_asking_cold", "prefix_plain_hit", "prefix_asking_again", "prefix_plain_again"))
    for rec, i in ((cold, 11), (again, 13)):             # on a cold cache and on a cache that holds its whole prompt: position 0, 13 rows
        s0, calls = _steps(rec)[0]
        assert s0["prefix_hit"] == 0 and s0["start_pos"] == [0] and s0["seq_starts"] == [0, 13] and s0["prompt_logprobs_list"] == [1]
        assert calls[0]["call"] == "SetPromptLogprobs" and calls[0]["ask"] == [1]
        rs = [r for r in rec if r.get("rsp") == i]
        tgt = list(range(101, 112)) + [500 + i]
        assert rs[0]["prompt_logprobs"] == [-t for t in tgt] and rs[0]["prompt_ranks"] == list(range(12)) and rs[0]["prompt_top_tokens"] == tgt
        assert all(r["prompt_logprobs"] == [] for r in rs[1:]) and len(rs) == 3
    for rec in (plain, plain2):                          # the identical request that does not ask hits the pages the asking one published
        s0, calls = _steps(rec)[0]
        assert s0["prefix_hit"] == 1 and s0["start_pos"] == [12] and s0["seq_starts"] == [0, 1]
        assert [c["call"] for c in calls] == ["SampleTopKTopP"]
    assert not [r for r in trace if "failed" in r and r["failed"] in (11, 12, 13, 14)]


def test_nobody_asks_nothing_is_called(trace):
    rec = _phase(trace, "nobody")
    steps = _steps(rec)
    assert steps and all([c["call"] for c in calls] == ["SampleTopKTopP"] for _, calls in steps)
    assert all(set(s["prompt_logprobs_list"]) == {-1} for s, _ in steps)
    rs = [r for r in rec if "rsp" in r]
    assert len(rs) == sum(GEN.values()) and all(r["prompt_logprobs"] == [] and r["prompt_top_tokens"] == [] for r in rs)


def test_backend_without_prompt_logprobs_fails_the_asking_request_only(trace):
    rec = _phase(trace, "old_backend")
    failed = [r for r in rec if "failed" in r]
    assert [(r["failed"], r["unsupported"]) for r in failed] == [(2, 1)]
    assert not [r for r in rec if r.get("rsp") == 2]
    for i in (1, 3, 4, 5, 6):
        rs = [r for r in rec if r.get("rsp") == i]
        assert len(rs) == GEN[i] and rs[-1]["finished"] == 1 and all(r["token"] == 500 + i and r["prompt_logprobs"] == [] for r in rs)
    later = [s for s, calls in _steps(rec)[1:] if 502 in _last_tokens(calls)]      # it left the batch after the step it failed in
    assert not later
    assert not [c for _, calls in _steps(rec) for c in calls if c["call"] != "SampleTopKTopP"]


def test_old_backend_serves_a_workload_that_does_not_ask(trace):
    rec = _phase(trace, "old_backend_nobody")
    assert not [r for r in rec if "failed" in r]
    assert len([r for r in rec if "rsp" in r]) == sum(GEN.values())
