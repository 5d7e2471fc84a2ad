"""Top-N logprobs on the host side (tests/host/logprobs_trace.cc: the generator and the engine over a fake backend): a request's count
follows its batch row through admission, finish, compaction and a prefix-cache hit, the results land in the Response of the request that
asked, nobody asking means no TopLogprobs call, and a backend without TopLogprobs fails the asking request alone."""
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "logprobs_trace")
# tests/host/logprobs_trace.cc: request id runs id + 1 steps and asks for ASKED[id] (25 and -2 as the client sent them)
GEN = {i: i + 1 for i in range(1, 7)}
ASKED = {1: 0, 2: 3, 3: 25, 4: -2, 5: 1, 6: 5}
N = {i: min(max(a, 0), 20) for i, a in ASKED.items()}
FAKE_VOCAB = 18                                          # the fake backend pads with token -1 from entry 18 on


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
    """[(step record, [post-processor calls of that step])]"""
    out = []
    for r in records:
        if "phase" in r:
            out.append((r, []))
        elif "call" in r:
            out[-1][1].append(r)
    return out


@pytest.mark.parametrize("phase,sampler", [("rows_mixed", "SampleRows"), ("uniform_mixed", "SampleTopKTopP")])
def test_counts_follow_the_batch_rows_and_results_their_requests(trace, phase, sampler):
    rec = _phase(trace, phase)
    rows_seen = {i: set() for i in GEN}
    for step, calls in _steps(rec):
        assert [c["call"] for c in calls] in (["TopLogprobs", sampler], [sampler])   # in front of the sampler, once
        ids = [t - 500 for t in calls[-1]["last_tokens"]]
        assert step["num_logprobs_list"] == [N[i] for i in ids]
        for row, i in enumerate(ids):
            rows_seen[i].add(row)
        if any(N[i] for i in ids):
            top = calls[0]
            assert top["call"] == "TopLogprobs" and top["num_logprobs"] == step["num_logprobs_list"] and top["batch"] == len(ids)
            assert top["temps_null"] == 0 and top["vocab"] == top["stride"] == 1000
        else:
            assert len(calls) == 1
    assert max(len(r) for r in rows_seen.values()) > 1                       # compaction moved somebody, and its count with it
    rsp = {i: [r for r in rec if r.get("rsp") == i] for i in GEN}
    for i, rs in rsp.items():
        assert len(rs) == GEN[i] and [r["finished"] for r in rs] == [0] * (GEN[i] - 1) + [1]
        n = min(N[i], FAKE_VOCAB)
        for r in rs:
            assert r["token"] == 500 + i
            assert r["top_tokens"] == [500 + i + e for e in range(n)], (i, r)       # this request's row of the compact results
            assert r["top_logprobs"] == [-e for e in range(n)]
            assert not n or r["top_tokens"][0] == r["token"]
    assert not [r for r in rec if "failed" in r]


def test_count_survives_a_prefix_cache_hit(trace):
    cold, hit = _phase(trace, "prefix_cold"), _phase(trace, "prefix_hit")
    assert [s["num_logprobs_list"] for s, _ in _steps(cold)] == [[2]] * 3
    steps = _steps(hit)
    assert steps[0][0]["prefix_hit"] == 1 and steps[0][0]["start_pos"] == [12]
    assert [s["num_logprobs_list"] for s, _ in steps] == [[4]] * 3
    assert all(c[0]["call"] == "TopLogprobs" and c[0]["num_logprobs"] == [4] for _, c in steps)
    assert [r["top_tokens"] for r in hit if r.get("rsp") == 12] == [[512, 513, 514, 515]] * 3
    assert [r["top_tokens"] for r in cold if r.get("rsp") == 11] == [[511, 512]] * 3


def test_nobody_asks_nothing_is_called(trace):
    rec = _phase(trace, "nobody")
    steps = _steps(rec)
    assert steps and all([c["call"] for c in calls] == ["SampleRows"] for _, calls in steps)
    assert all(not any(s["num_logprobs_list"]) for s, _ in steps)
    rs = [r for r in rec if "rsp" in r]
    assert len(rs) == sum(GEN.values()) and all(r["top_tokens"] == [] and r["top_logprobs"] == [] for r in rs)


@pytest.mark.parametrize("phase", ["old_backend_rows", "old_backend_uniform"])
def test_backend_without_top_logprobs_fails_the_asking_request_only(trace, phase):
    rec = _phase(trace, phase)
    failed = [r for r in rec if "failed" in r]
    assert [(r["failed"], r["unsupported"]) for r in failed] == [(2, 1)]
    assert not [r for r in rec if r.get("rsp") == 2]
    for i in (1, 3, 4, 5, 6):
        rs = [r for r in rec if r.get("rsp") == i]
        assert len(rs) == GEN[i] and rs[-1]["finished"] == 1 and all(r["token"] == 500 + i and r["top_tokens"] == [] for r in rs)
    # the failed request left the batch after the step it failed in
    later = [s for s, calls in _steps(rec)[1:] if 502 in calls[-1]["last_tokens"]]
    assert not later


def test_old_backend_serves_a_workload_that_does_not_ask(trace):
    rec = _phase(trace, "old_backend_nobody")
    assert not [r for r in rec if "failed" in r]
    assert len([r for r in rec if "rsp" in r]) == sum(GEN.values())
    assert all(c["call"] == "SampleTopKTopP" for _, calls in _steps(rec) for c in calls)
