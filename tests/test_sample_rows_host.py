"""The per-request sampler on the host side (tests/host/sample_trace.cc: the generator and the engine over a fake backend): a request's seed
and draw count follow its batch row through admission, finish and compaction, draws count 0, 1, 2 ... per request (a prefix-cache hit
included), unseeded requests get the splitmix64 sequence of the sampling seed, and with the switch off the backend sees today's call."""
import json
import os
import subprocess

import pytest

from tests import sample_rows as S
from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "sample_trace")
SAMPLING_SEED = 0x1234567890ABCDEF
# tests/host/sample_trace.cc: request id runs id + 1 steps; even ids bring seed 1000 + id; ids 2 and 5 are greedy
GEN = {i: i + 1 for i in range(1, 7)}
TOP_K = {i: 1 if i in (2, 5) else 10 * i for i in range(1, 7)}
UNSEEDED = [1, 3, 5]                                     # in the order they are parsed


def want_seed(i):
    if i % 2 == 0:
        return 1000 + i
    return S.splitmix64((SAMPLING_SEED + UNSEEDED.index(i) + 1) & (2 ** 64 - 1))


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN, hex(SAMPLING_SEED)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _calls_of_phase(trace, phase):
    """the sampling calls between the first and the last step record of a phase (every step record is followed by its call)"""
    out, inside = [], False
    for r in trace:
        if "phase" in r:
            inside = r["phase"] == phase
        elif inside and "call" in r:
            out.append(r)
    return out


def test_seeds_and_draws_follow_the_batch_rows(trace):
    calls = _calls_of_phase(trace, "rows_batch_order")
    assert calls and all(c["call"] == "SampleRows" for c in calls)
    produced = {i: 0 for i in GEN}
    rows_seen = {i: set() for i in GEN}
    for c in calls:
        ids = [t - 500 for t in c["last_tokens"]]
        assert len(ids) == c["batch"] == len(c["seeds"]) == len(c["draws"]) == len(c["top_k"]) <= 4
        for row, i in enumerate(ids):
            assert c["seeds"][row] == want_seed(i), (i, row)
            assert c["draws"][row] == produced[i], (i, row)                 # 0 on the step that ends the prefill, then 1, 2, ...
            assert c["top_k"][row] == TOP_K[i]
            assert abs(c["top_p"][row] - (0.5 + 0.01 * i)) < 1e-6 and abs(c["temperatures"][row] - (1 + 0.25 * i)) < 1e-6
            produced[i] += 1
            rows_seen[i].add(row)
        assert c["temps_null"] == 0
    assert produced == GEN                                                   # every request sampled once per token, none after it left
    assert max(len(r) for r in rows_seen.values()) > 1                       # compaction moved somebody, and its seed and draws with it
    # a later request moved in beside running ones: one call with draw counts that differ
    assert any(min(c["last_tokens"]) <= 504 and max(c["last_tokens"]) >= 505 and len(set(c["draws"])) > 1 for c in calls)


def test_generator_packs_what_the_backend_gets(trace):
    steps = [r for r in trace if r.get("phase") == "rows_batch_order"]
    calls = _calls_of_phase(trace, "rows_batch_order")
    assert len(steps) == len(calls)
    for s, c in zip(steps, calls):
        assert s["seed_list"] == c["seeds"] and s["draw_list"] == c["draws"] and s["top_k_list"] == c["top_k"]


def test_draws_start_at_zero_on_a_prefix_cache_hit(trace):
    cold = [r for r in trace if r.get("phase") == "rows_prefix_cold"]
    hit = [r for r in trace if r.get("phase") == "rows_prefix_hit"]
    assert [r["draw_list"] for r in cold] == [[0], [1], [2]] and all(r["seed_list"] == [77] for r in cold)
    assert hit[0]["prefix_hit"] == 1 and hit[0]["start_pos"] == [12]         # three cached pages: only the 13th token is fed
    assert [r["draw_list"] for r in hit] == [[0], [1], [2]]
    first_unseeded = S.splitmix64((SAMPLING_SEED + 1) & (2 ** 64 - 1))       # a new generator counts its unseeded requests from 1
    assert all(r["seed_list"] == [first_unseeded] for r in hit)
    calls = _calls_of_phase(trace, "rows_prefix_hit")
    assert [c["draws"] for c in calls] == [[0], [1], [2]] and all(c["call"] == "SampleRows" for c in calls)


def test_switch_off_is_todays_call(trace):
    calls = _calls_of_phase(trace, "uniform_batch_order")
    steps = [r for r in trace if r.get("phase") == "uniform_batch_order"]
    assert calls and len(calls) == len(steps)
    assert all(c["call"] == "SampleTopKTopP" for c in calls)
    n_rows_calls = sum(1 for r in trace if r.get("call") == "SampleRows")
    assert n_rows_calls == len(_calls_of_phase(trace, "rows_batch_order")) + 6   # the two prefix phases: three steps each
    for s, c in zip(steps, calls):
        ids = [t - 500 for t in c["last_tokens"]]
        assert c["top_k"] == [TOP_K[i] for i in ids]
        assert c["default_top_k"] == c["top_k"][0]                           # SURVEY.md Q3, kept: the first row's top_k for the batch
        assert c["default_top_p"] == 0 and c["enable_penalty"] == 0 and c["stride"] == c["vocab"] == 1000
        assert c["req_list_changed"] == s["req_list_changed"]
    assert calls[0]["req_list_changed"] == 1 and any(c["req_list_changed"] == 0 for c in calls)


def test_switch_on_needs_a_backend_that_can(trace):
    ev = {r["event"]: r for r in trace if "event" in r}
    assert ev["init_without_sample_rows"] == {"event": "init_without_sample_rows", "ok": 0, "unsupported": 1}
    assert ev["init_switch_off"]["ok"] == 1
