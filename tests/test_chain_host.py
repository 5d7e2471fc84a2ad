"""All per-request features in one workload on the host side (tests/host/chain_trace.cc: the generator and the engine over a fake backend):
twelve requests through four batch rows, two prefills per step, rows leaving from the front, the middle and the end of the batch.  Every
request carries its own subset of seed, top-N logprobs, prompt logprobs, logit rule with min_new_tokens, guide and adapter, each a function
of its id, and the last token of a row names its request: at every step every per-row list must hold, in every row, what that row's request
carries; the results of the compact lists (top-N by list place, prompt logprobs by position) must reach the request they were made for; and
the requests that fail must fail alone.

The defect this file found: a request that failed on a step (llm_generator.cc, the `continue` behind NotifyFailure) passed its prompt
positions but not its top-N entry, so every asking row behind it in the batch was answered with the entry of the row in front -- request 7
received request 6's top-N list on the step in which request 6's rule was refused by the backend."""
import json
import os
import subprocess

import pytest

from tests import guide as G
from tests import sample_rows as S
from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "chain_trace")
IDS = range(1, 13)
GEN = {1: 3, 2: 1, 3: 5, 4: 2, 5: 4, 6: 3, 7: 6, 8: 2, 9: 3, 10: 2, 11: 4, 12: 3}
GUIDED = (3, 7, 10)
REFUSED, BACKEND_REFUSES = 9, 6
SAMPLING_SEED = 42


# ---- what request i carries (tests/host/chain_trace.cc Spec) ----------------------------------------------------------------------------
def prompt(i):
    return [10 * i + k for k in range(1, 2 + i % 3)] + [500 + i]


def nlp(i):
    return i * 7 % 5


def plp(i):
    return -1 if i % 4 == 0 else i % 4 - 1


def min_new(i):
    return 1 + i % 2 if i % 3 == 2 else 0


def flags_of(i, produced):
    if i == BACKEND_REFUSES:
        return 0                                         # its rule never reached the backend: nothing to apply
    f = 1 if (i % 3 == 2 or i == 7) else 0
    if min_new(i) and produced < min_new(i):
        f |= 2
    return f


def regex(i):
    return chr(ord("a") + i) + "{1,20}"


PER_ROW = {   # ModelInput list -> the value request i carries (constant over its life)
    "temperatures": lambda i: 0.5 + i / 16, "top_p_list": lambda i: i / 16, "top_k_list": lambda i: 1 + i,
    "repetition_penalty_list": lambda i: 1 + i / 8, "presence_penalty_list": lambda i: i / 4, "frequency_penalty_list": lambda i: i / 32,
    "lora_slots": lambda i: i % 3 - 1, "num_logprobs_list": nlp,
}


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.fixture(scope="module")
def dfas():
    return {i: G.compile_regex(regex(i)) for i in GUIDED}


def _phase(trace, phase):
    first = next(k for k, r in enumerate(trace) if r.get("begin") == phase)
    out = []
    for r in trace[first + 1:]:
        if "begin" in r:
            break
        out.append(r)
    return out


def _steps(records):
    return [r for r in records if "phase" in r]


def _ids(step):
    return [t - 500 for t in step["last_tokens"]]


def _seeds(records):
    """the seed of every request: its own (odd ids) or splitmix64(sampling_seed + n) for the n-th request that is started without one"""
    out, n = {}, 0
    order = []
    for st in _steps(records):
        for i in _ids(st):
            if i not in order:
                order.append(i)
    for i in order:
        if i % 2:
            out[i] = 1000 + i
        else:
            n += 1
            out[i] = S.splitmix64(SAMPLING_SEED + n)
    return out


@pytest.mark.parametrize("phase", ["all", "no_top"])
def test_every_list_entry_of_a_row_belongs_to_the_rows_request(trace, dfas, phase):
    records = _phase(trace, phase)
    steps = _steps(records)
    seeds = _seeds(records)
    uploads = {r["bias_tokens"][0]: r["slot"] for r in records if r.get("call") == "SetLogitRule"}    # first bias token -> slot
    guide_slot = {}
    for r in records:
        if r.get("call") == "LoadGuide":
            i = next(i for i in GUIDED if r["trans"] == dfas[i][0].reshape(-1).tolist())
            assert r["accept"] == dfas[i][1].tolist() and r["ends"] == [2, 901]
            guide_slot[i] = r["slot"]
    produced, slot_of, seen = {}, {}, set()
    shapes = set()
    for st in steps:
        ids = _ids(st)
        B = len(ids)
        shapes.add(B)
        assert len(set(ids)) == B and all(i in IDS for i in ids)
        for key, f in PER_ROW.items():
            assert st[key] == [f(i) for i in ids], (st["step"], key)
        assert st["seed_list"] == [seeds[i] for i in ids], st["step"]
        assert st["draw_list"] == [produced.get(i, 0) for i in ids], st["step"]       # draws count per request
        assert st["prompt_logprobs_list"] == [plp(i) if i not in produced else -1 for i in ids], st["step"]
        assert st["logit_flags"] == [flags_of(i, produced.get(i, 0)) for i in ids], st["step"]
        assert len(set(st["batch_slots"])) == B
        for b, i in enumerate(ids):
            assert slot_of.setdefault(i, st["batch_slots"][b]) == st["batch_slots"][b], (st["step"], i)      # a request keeps its slot
            if i in produced:
                assert st["seq_starts"][b + 1] - st["seq_starts"][b] == 1 and st["start_pos"][b] == len(prompt(i)) + produced[i] - 1
                assert b < st["decoding_batches"]
            else:
                assert st["seq_starts"][b + 1] - st["seq_starts"][b] == len(prompt(i)) and st["start_pos"][b] == 0
                assert b >= st["decoding_batches"]
            if i in GUIDED:
                trans = dfas[i][0]
                want = G.walk(trans, 0, bytes([ord("a") + i]) * produced.get(i, 0))
                assert st["guide_slots"][b] == guide_slot[i] and st["guide_states"][b] == want != G.DEAD, (st["step"], i)
            else:
                assert st["guide_slots"][b] == -1
        for i in ids:
            produced[i] = produced.get(i, 0) + 1
            seen.add(i)
    assert seen == set(IDS) - {REFUSED}
    assert shapes >= ({1, 2, 3, 4} if phase == "all" else {2, 3})
    # rows left from the front, from the middle and from the end of the batch while others stayed
    left = set()
    for a, b in zip(steps, steps[1:]):
        ia, ib = _ids(a), _ids(b)
        for k, i in enumerate(ia):
            if i not in ib and any(j in ib for j in ia):
                left.add("front" if k == 0 else "end" if k == len(ia) - 1 else "middle")
        kept = [i for i in ia if i in ib]
        assert ib[:len(kept)] == kept                    # the stayers keep their order, the joiners stand behind them
    assert left == {"front", "middle", "end"} if phase == "all" else left, left
    # every rule went up once, into the slot its request then ran in; the stop-suppress bit left exactly at min_new_tokens (flags_of above)
    for i in IDS:
        if (i % 3 == 2 or i in (7, BACKEND_REFUSES)) and i != REFUSED:
            first = 999 if i == BACKEND_REFUSES else i
            assert uploads[first] == slot_of[i], i
    assert sum(1 for r in records if r.get("call") == "SetLogitRule") == 6
    if phase == "all":
        for i in (5, 11):                                # min_new_tokens 2 and a life long enough to see the bit leave
            fl = [st["logit_flags"][_ids(st).index(i)] for st in steps if i in _ids(st)]
            assert fl[:3] == [3, 3, 1], (i, fl)


@pytest.mark.parametrize("phase", ["all", "no_top"])
def test_the_backend_calls_carry_the_steps_lists(trace, phase):
    """every post-processor call of a step received the step's own lists, in the engine's order, with the temperature only in the penalty"""
    records = _phase(trace, phase)
    k = 0
    n_steps = 0
    while k < len(records):
        st = records[k]
        k += 1
        if "phase" not in st:
            continue
        n_steps += 1
        calls = []
        while k < len(records) and "phase" not in records[k]:
            if "call" in records[k] and records[k]["call"] not in ("SetLogitRule", "LoadGuide", "UnloadGuide", "SetGuideVocab"):
                calls.append(records[k])
            k += 1
        names = [c["call"] for c in calls]
        want = ["SetInputs"]
        if any(a >= 0 for a in st["prompt_logprobs_list"]):
            want.append("SetPromptLogprobs")
        if any(g >= 0 for g in st["guide_slots"]):
            want.append("GuideEdit")
        if any(st["logit_flags"]):
            want.append("EditLogits")
        want.append("ApplyPenalty")
        if any(st["num_logprobs_list"]):
            want.append("TopLogprobs")
        want.append("SampleRows")
        if any(a >= 0 for a in st["prompt_logprobs_list"]):
            want.append("GetPromptLogprobs")
        assert names == want, (st["step"], names, want)
        by = {c["call"]: c for c in calls}
        for c in calls:
            if "last_tokens" in c:
                assert c["last_tokens"] == st["last_tokens"], (st["step"], c["call"])
        # (a step without an adapter row hands the runtime no adapter list at all)
        assert by["SetInputs"]["lora_slots"] == (st["lora_slots"] if any(a >= 0 for a in st["lora_slots"]) else [])
        assert by["SetInputs"]["decoding_batches"] == st["decoding_batches"]
        assert by["ApplyPenalty"]["temperatures"] == st["temperatures"] and by["ApplyPenalty"]["repetition"] == st["repetition_penalty_list"]
        assert by["ApplyPenalty"]["slots"] == st["batch_slots"]
        s = by["SampleRows"]
        assert s["temps_null"] == 1 and s["top_k"] == st["top_k_list"] and s["top_p"] == st["top_p_list"]
        assert s["seeds"] == st["seed_list"] and s["draws"] == st["draw_list"]
        if "TopLogprobs" in by:
            assert by["TopLogprobs"]["temps_null"] == 1 and by["TopLogprobs"]["num_logprobs"] == st["num_logprobs_list"]
        if "EditLogits" in by:
            assert by["EditLogits"]["slots"] == st["batch_slots"] and by["EditLogits"]["flags"] == st["logit_flags"]
        if "GuideEdit" in by:
            assert by["GuideEdit"]["slots"] == st["guide_slots"] and by["GuideEdit"]["states"] == st["guide_states"]
        if "SetPromptLogprobs" in by:
            assert by["SetPromptLogprobs"]["ask"] == st["prompt_logprobs_list"]
    assert n_steps >= (8 if phase == "all" else 5)


def _responses(records):
    out = {}
    for r in records:
        if "rsp" in r:
            out.setdefault(r["rsp"], []).append(r)
    return out


def _check_survivor(i, rsps, n_tokens):
    """the responses of request i: one per step it ran, each with ITS top-N entry of THAT step, the first with ITS prompt positions"""
    assert len(rsps) == n_tokens, (i, len(rsps))
    assert [r["token"] for r in rsps] == [500 + i] * n_tokens
    assert [r["finished"] for r in rsps] == [0] * (n_tokens - 1) + [1]
    p = prompt(i)
    for k, r in enumerate(rsps):
        step = -r["logprob"]                             # the fake sampler answers with the engine step
        n = nlp(i)
        assert r["top_tokens"] == [i * 10000 + step * 100 + e for e in range(n)], (i, k, r["top_tokens"])
        assert r["top_logprobs"] == [-e for e in range(n)], (i, k)
        if k == 0 and plp(i) >= 0:
            assert r["prompt_logprobs"] == [-t for t in p[1:]] and r["prompt_ranks"] == list(range(len(p) - 1)), (i, r)
            assert r["prompt_top_tokens"] == [t + e for t in p[1:] for e in range(plp(i))], (i, r)
            assert r["prompt_top_logprobs"] == [-e for _ in p[1:] for e in range(plp(i))], (i, r)
        else:
            assert r["prompt_logprobs"] == [] and r["prompt_ranks"] == [] and r["prompt_top_tokens"] == [] and r["prompt_top_logprobs"] == []
    steps = [-r["logprob"] for r in rsps]
    assert steps == list(range(steps[0], steps[0] + n_tokens))


def test_results_reach_their_request_and_the_failing_requests_fail_alone(trace):
    records = _phase(trace, "all")
    failed = {r["failed"]: r for r in records if "failed" in r}
    assert sorted(failed) == [BACKEND_REFUSES, REFUSED]
    assert failed[REFUSED]["code"] == "invalid" and "logit_bias" in failed[REFUSED]["msg"]
    assert failed[BACKEND_REFUSES]["code"] == "other" and "logit rules" in failed[BACKEND_REFUSES]["msg"]
    rsps = _responses(records)
    assert sorted(rsps) == [i for i in IDS if i not in failed]
    for i, rs in rsps.items():
        _check_survivor(i, rs, GEN[i])
    # the step request 6 failed on: it stood in front of request 7, which asked for top-N and prompt logprobs on the same step, and behind
    # request 3, which received top-N; 6 itself asked for both, so both cursors had to pass its results
    steps = _steps(records)
    st = next(s for s in steps if BACKEND_REFUSES in _ids(s))
    ids = _ids(st)
    assert ids.index(3) < ids.index(6) < ids.index(7) and nlp(3) > 0 and nlp(6) > 0 and plp(6) >= 0 and nlp(7) > 0 and plp(7) >= 0
    assert st["prompt_logprobs_list"][ids.index(7)] >= 0
    assert sum(1 for s in steps if BACKEND_REFUSES in _ids(s)) == 1        # it left after that step
    assert REFUSED not in {i for s in steps for i in _ids(s)}              # and 9 never got a row


def test_a_backend_without_top_logprobs_fails_the_asking_requests_alone(trace):
    """every request that asks for top-N fails on its first step; the others are served, and the prompt logprobs of a request that stands
    behind a failing one that asked for them too are its own"""
    records = _phase(trace, "no_top")
    failed = {r["failed"]: r for r in records if "failed" in r}
    asking = [i for i in IDS if nlp(i) > 0 and i not in (REFUSED, BACKEND_REFUSES)]
    assert sorted(failed) == sorted(asking + [REFUSED, BACKEND_REFUSES])
    for i in asking:
        assert failed[i]["code"] == "unsupported" and "num_logprobs" in failed[i]["msg"]
    steps = _steps(records)
    for i in asking + [BACKEND_REFUSES]:
        assert sum(1 for s in steps if i in _ids(s)) == 1
    rsps = _responses(records)
    assert sorted(rsps) == [5, 10]
    for i, rs in rsps.items():
        _check_survivor(i, rs, GEN[i])
    # both were prefilled on a step with a failing neighbour IN FRONT of them that asked for prompt logprobs too: the prompt cursor had to
    # pass the neighbour's positions
    for i in (5, 10):
        st = next(s for s in steps if i in _ids(s) and s["prompt_logprobs_list"][_ids(s).index(i)] >= 0)
        ids = _ids(st)
        front = [j for j in ids[:ids.index(i)] if j in failed and st["prompt_logprobs_list"][ids.index(j)] >= 0 and len(prompt(j)) > 1]
        assert front, (i, ids, st["prompt_logprobs_list"])
