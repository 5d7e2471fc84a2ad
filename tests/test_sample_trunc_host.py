"""min_p / typical_p on the host side (tests/host/trunc_trace.cc: the generator and the engine over a fake backend): the two per-row lists
follow their requests through joins and leaves, a step without a truncating row takes today's SampleRows call, and a request that asks
fails alone where it cannot be served -- per_request_sampling off, or a backend without SampleRowsTrunc."""
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "trunc_trace")
# tests/host/trunc_trace.cc: request id runs id + 1 steps; ids 2 and 4 set min_p, ids 3 and 4 typical_p; id 5 is greedy
GEN = {i: i + 1 for i in range(1, 7)}
MIN_P = {i: 0.01 * i if i in (2, 4) else 0.0 for i in GEN}
TYPICAL_P = {i: 0.5 + 0.05 * i if i in (3, 4) else 1.0 for i in GEN}
TOP_K = {i: 1 if i == 5 else 10 * i for i in GEN}
ASKING = (2, 3, 4)


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _phase(trace, phase):
    """(step records, sampling calls, failures, finished ids) of a phase: every step record is followed by its call"""
    steps, calls, failed, finished, inside = [], [], [], [], False
    for r in trace:
        if "begin" in r:
            inside = r["begin"] == phase
        elif inside and "phase" in r:
            assert r["phase"] == phase
            steps.append(r)
        elif inside and "call" in r:
            calls.append(r)
        elif inside and "failed" in r:
            failed.append(r)
        elif inside and "finished" in r:
            finished.append(r["finished"])
    return steps, calls, failed, finished


def test_both_lists_follow_joins_and_leaves(trace):
    steps, calls, failed, finished = _phase(trace, "trunc")
    assert not failed and sorted(finished) == list(GEN) and len(steps) == len(calls)
    produced = {i: 0 for i in GEN}
    rows_seen = {i: set() for i in GEN}
    for s, c in zip(steps, calls):
        ids = [t - 500 for t in c["last_tokens"]]
        assert len(ids) == c["batch"] == len(s["min_p_list"]) == len(s["typical_p_list"]) <= 4
        for row, i in enumerate(ids):                                        # what the generator packed, row by row
            assert abs(s["min_p_list"][row] - MIN_P[i]) < 1e-6 and abs(s["typical_p_list"][row] - TYPICAL_P[i]) < 1e-6, (i, row)
            assert s["top_k_list"][row] == TOP_K[i]
            produced[i] += 1
            rows_seen[i].add(row)
        if c["call"] == "SampleRowsTrunc":                                   # and what the backend got
            assert c["min_p"] == s["min_p_list"] and c["typical_p"] == s["typical_p_list"] and c["top_k"] == s["top_k_list"]
            assert c["draws"] == [produced[i] - 1 for i in ids] and c["seeds"] == [1000 + i for i in ids]
            assert c["temps_null"] == 0 and c["stride"] == c["vocab"] == 1000
    assert produced == GEN
    assert max(len(r) for r in rows_seen.values()) > 1                       # compaction moved somebody, and its two values with it


def test_a_step_without_a_truncating_row_calls_sample_rows(trace):
    steps, calls, _, _ = _phase(trace, "trunc")
    kinds = set()
    for c in calls:
        ids = [t - 500 for t in c["last_tokens"]]
        want = "SampleRowsTrunc" if any(i in ASKING for i in ids) else "SampleRows"
        assert c["call"] == want, (ids, c["call"])
        kinds.add(c["call"])
    assert kinds == {"SampleRowsTrunc", "SampleRows"}                        # requests 5 and 6 outlive every asking one


def test_a_request_fails_alone_without_per_request_sampling(trace):
    steps, calls, failed, finished = _phase(trace, "switch_off")
    assert sorted(f["failed"] for f in failed) == list(ASKING) and sorted(finished) == [1, 5, 6]
    assert all(f["unsupported"] == 1 and "per_request_sampling" in f["msg"] for f in failed)
    assert calls and all(c["call"] == "SampleTopKTopP" for c in calls)
    assert all(t - 500 not in ASKING for c in calls for t in c["last_tokens"])


def test_a_request_fails_alone_on_a_backend_without_sample_rows_trunc(trace):
    steps, calls, failed, finished = _phase(trace, "no_backend")
    assert sorted(f["failed"] for f in failed) == list(ASKING) and sorted(finished) == [1, 5, 6]
    assert all(f["unsupported"] == 1 and "SampleRowsTrunc" in f["msg"] for f in failed)
    assert calls and all(c["call"] == "SampleRows" for c in calls)
